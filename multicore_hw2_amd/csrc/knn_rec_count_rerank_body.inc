// knn_rec_count_rerank_body.inc — the cell-pruned count's re-rank (knn_cells_query_count), the one walk of
// knn_count_rerank_kernel (knn_exact.hip), knn_count_each_rerank_kernel (knn_each.hip), knn_count_self_rerank_kernel
// (knn_self_routed.hip) and knn_count_masked_rerank_kernel (knn_masked_routed.hip).  The including kernel fixes FORM
// (knn_exact_dev.h: KNN_REC_SCALAR, _EACH, _SELF, _MASKED) and provides the scalar kernel's arguments by their names, with cap for
// the radius, and radii, first and mask as arguments or as null / zero constants.
//
// Every row of every record with v0's arithmetic through perm, as knn_topk_rerank_gated_kernel walks them — one block per list,
// positions whose layout norm is +INF (padding, rows outside the robust box) skipped —, and a hit adds one to its query's scratch
// count.  A hit: the distance finite (rerank_pair gives ~0 otherwise), <= the query's radius (KNN_REC_RADIUS) and <= cap; SELF: and
// the LOCAL row — the key's low word, base 0 — not first + qi, the query's own; MASKED: and the LOCAL row's bit set in mask, read
// behind the distance compares (the records name masked-out rows too: the pass's front knows no mask).  qi is the pass's query
// number, and radii the pass's; mask is the shard's, the same for every pass.  The 16 rows of a record sit on 16 neighbouring
// lanes and belong to one query: their hits are summed from one ballot and the record's first lane adds them.
    const unsigned list_id = blockIdx.x;
    if (ctl[KNN_CTL_FALLBACK] != 0u || list_id >= nlists)
        return;
    const unsigned want = counts[list_id];
    const unsigned nrec = min(want, slice);
    if (threadIdx.x == 0 && want > slice)
        ctl[KNN_CTL_FALLBACK] = 1u;
    const u64 *__restrict__ list = rec + (size_t)list_id * slice;
    const unsigned lane = threadIdx.x & 63u;
    // (every wave runs the same number of rounds: the ballot below is taken by all 64 lanes)
    for (unsigned c0 = 0u; c0 < nrec * 16u; c0 += KNN_BLOCK) {
        const unsigned c = c0 + threadIdx.x;
        bool hit = false;
        unsigned qi = 0u;
        if (c < nrec * 16u) {
            const u64 e = list[c >> 4];
            const unsigned lo = (unsigned)e, reg = c & 15u;
            const long long pos = (long long)(lo >> 1) * 32 + 8 * (reg >> 2) + 4 * (lo & 1u) + (reg & 3u);   // (rerank_pair's)
            const unsigned rmask = pos < n && norms[pos] < INFINITY ? 0xFFFFu : 0u;
            const u64 key = rerank_pair<0>(Q, R, k, n, 0ll, e, reg, rmask, 0u, perm, qi);   // ~0: nothing there, or not finite
            if (key != ~0ull) {
                const float d = __uint_as_float((unsigned)(key >> 32));
                const float rad = KNN_REC_RADIUS(qi);
                hit = d <= rad && d <= cap && (FORM != KNN_REC_SELF || (unsigned)key != first + qi);
                if (FORM == KNN_REC_MASKED)   // (inside the lane's own branch: every lane still reaches the ballot)
                    hit = hit && KNN_REC_ADMITS((unsigned)key);
            }
        }
        const u64 hits = __ballot(hit);
        const unsigned mine = (unsigned)__popcll((hits >> (lane & 48u)) & 0xFFFFull);
        if ((lane & 15u) == 0u && mine != 0u)
            atomicAdd(&qcount[qi], mine);
    }
