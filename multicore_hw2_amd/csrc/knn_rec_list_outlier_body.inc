// knn_rec_list_outlier_body.inc — the cell-pruned list's out-of-box rows, the one walk of knn_list_outlier_kernel,
// knn_list_each_outlier_kernel, knn_list_self_outlier_kernel and knn_list_masked_outlier_kernel (FORM and the names: as
// knn_rec_count_rerank_body.inc).
//
// knn_rec_count_outlier_body.inc's walk — every (query, listed row) pair once, with v0's arithmetic; grid (row blocks, queries) —,
// and a hit reserves in its query's scratch cursor and stores its key.  MASKED: a listed row whose bit is clear is passed over
// before its distance is accumulated.
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    const float rad = KNN_REC_RADIUS(q);
    const unsigned own = first + q;
    u64 off;
    const unsigned room = list_room(offsets, q, off);
    for (unsigned j = blockIdx.x * KNN_BLOCK + threadIdx.x; j < count; j += gridDim.x * KNN_BLOCK) {
        const unsigned row = list[j];
        if (FORM == KNN_REC_MASKED && !KNN_REC_ADMITS(row))
            continue;
        const float *__restrict__ r = R + (size_t)row * k;
        float acc = 0.0f;
        for (int d = 0; d < k; ++d) {
            const float diff = qp[d] - r[d];
            const float sq = diff * diff;
            acc = acc + sq;
        }
        if (acc < INFINITY && acc <= rad && acc <= cap && (FORM != KNN_REC_SELF || row != own))
            list_put(&cursor[q], keys, off, room, pack_key(acc, gids ? gids[row] : (unsigned)(base + (long long)row)));
    }
