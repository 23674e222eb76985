// knn_rec_count_outlier_body.inc — the cell-pruned count's out-of-box rows, the one walk of knn_count_outlier_kernel,
// knn_count_each_outlier_kernel, knn_count_self_outlier_kernel and knn_count_masked_outlier_kernel (FORM and the names: as
// knn_rec_count_rerank_body.inc).
//
// Rows outside the filter's robust box never enter the scan: every (query, listed row) pair once, with v0's arithmetic.
// grid (row blocks, queries); one add per wave.  SELF: the listed row first + q, the query's own, is no hit.  MASKED: a listed row
// whose bit is clear is passed over before its distance is accumulated.
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    const float rad = KNN_REC_RADIUS(q);
    const unsigned own = first + q;
    unsigned cnt = 0u;
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
        cnt += acc < INFINITY && acc <= rad && acc <= cap && (FORM != KNN_REC_SELF || row != own) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        cnt += (unsigned)__shfl_xor((int)cnt, off, KNN_WAVE);
    if ((threadIdx.x & 63u) == 0u && cnt != 0u)
        atomicAdd(&qcount[q], cnt);
