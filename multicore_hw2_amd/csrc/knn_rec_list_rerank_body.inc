// knn_rec_list_rerank_body.inc — the cell-pruned list's re-rank, the one walk of knn_list_rerank_kernel, knn_list_each_rerank_kernel,
// knn_list_self_rerank_kernel and knn_list_masked_rerank_kernel (FORM and the names: as knn_rec_count_rerank_body.inc).
//
// knn_rec_count_rerank_body.inc's walk and hit rule (one block per list, positions whose layout norm is +INF skipped), and a hit
// reserves in its query's scratch cursor and stores its key.  base / gids as in the exact list.  The scalar and each forms let
// rerank_pair add base and put gids in the finished key's place; SELF needs the LOCAL row for the own-row compare and MASKED for the
// row's mask bit, so they re-rank with base 0 and make the number the key carries themselves.
    const unsigned list_id = blockIdx.x;
    if (ctl[KNN_CTL_FALLBACK] != 0u || list_id >= nlists)
        return;
    const unsigned want = counts[list_id];
    const unsigned nrec = min(want, slice);
    if (threadIdx.x == 0 && want > slice)
        ctl[KNN_CTL_FALLBACK] = 1u;
    const u64 *__restrict__ list = rec + (size_t)list_id * slice;
    for (unsigned c = threadIdx.x; c < nrec * 16u; c += KNN_BLOCK) {
        unsigned qi = 0u;
        const u64 e = list[c >> 4];
        const unsigned lo = (unsigned)e, reg = c & 15u;
        const long long pos = (long long)(lo >> 1) * 32 + 8 * (reg >> 2) + 4 * (lo & 1u) + (reg & 3u);   // (rerank_pair's)
        const unsigned rmask = pos < n && norms[pos] < INFINITY ? 0xFFFFu : 0u;
        constexpr bool LOCAL = FORM == KNN_REC_SELF || FORM == KNN_REC_MASKED;
        const u64 key = rerank_pair<0>(Q, R, k, n, LOCAL ? 0ll : base, e, reg, rmask, 0u, perm, qi);
        if (key == ~0ull)   // nothing there, or not finite
            continue;
        const unsigned row = (unsigned)key;   // (SELF, MASKED: the LOCAL row; else base + row)
        const float d = __uint_as_float((unsigned)(key >> 32));
        const float rad = KNN_REC_RADIUS(qi);
        if (d <= rad && d <= cap && (FORM != KNN_REC_SELF || row != first + qi) && (FORM != KNN_REC_MASKED || KNN_REC_ADMITS(row))) {
            u64 off;
            const unsigned room = list_room(offsets, qi, off);
            if (LOCAL)
                list_put(&cursor[qi], keys, off, room,
                         (key & 0xFFFFFFFF00000000ull) | (u64)(gids ? gids[row] : (unsigned)(base + (long long)row)));
            else
                list_put(&cursor[qi], keys, off, room, gids ? (key & 0xFFFFFFFF00000000ull) | (u64)gids[row] : key);
        }
    }
