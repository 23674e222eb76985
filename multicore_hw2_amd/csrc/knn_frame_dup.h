// knn_frame_dup.h — a seed score of a cell in per-cell frames as a FRAME-FREE bound (knn_cells_prep_kernel<.., CTR = true, TK = true>),
// and the host hook that runs the same lines (knn_debug_frame_dup; tests/test_frames_topk_logic.py).
//
// A cell in per-cell frames (knn_cells_recentre) has its own centre and scale: frame = { centre[16], scale_c, ratio = scale_c /
// sigma (a power of two), bmax_c, nmax_c }.  A query is rounded in THAT frame — fp32 subtract, exact power-of-two scale, fp16 to
// nearest even, times -2 — and the cell's rows are scored against it, so scores of different cells are not comparable.  What is
// comparable is the bound each score implies on its own row's real distance: knn_threshold's Dup with the cell's constants
// (knn_bound_consts(k, 1, scale_c, amax, bmax_c, nmax_c)), a squared distance in the cell's units, divided by ratio^2 into the
// shard's.  Dup_c(u) is non-decreasing in u (knn_threshold is), and for the row that scored u it bounds the real scaled distance:
// D_row <= D0up <= Dup.  DESIGN §4.6, "Per-cell frames".
//
// The far branch: a query that does not fit the frame (a coordinate beyond CELL_FRAME_AMAX cell units, or not an fp16 number at
// all) gets a zero B operand — the scores are the rows' norms, finite exactly for real in-box rows — and the triangle
// inequality's bound: every row of the cell is within sqrt(k) bmax_c (1 + 2^-10) of the centre, the query sqrt(n32) from it.
#pragma once

#include "knn_filter_dev.h"

#define KNN_FRAME_AMAX 16384.0f   // = CELL_FRAME_AMAX (knn_cells.hip)

// A query row in one cell's frame: the B operand (16 values, zero beyond k and when far), and what the bound needs of it.
struct KnnFrameQuery {
    float amax;   // largest |rounded coordinate|
    float nrm;    // computed norm of the rounded row (exact products, fp32 sum in dimension order)
    float n32;    // the same of the unrounded fp32 coordinates (the far branch's distance to the centre)
    bool far;     // the query does not fit the frame
};

__host__ __device__ __attribute__((always_inline)) inline KnnFrameQuery knn_frame_query(int k, const float (&fr)[KNN_CELL_FRAME_WORDS],
                                                                                        const float *__restrict__ qrow, _Float16 (&b)[16])
{
#pragma clang fp contract(off)
    KnnFrameQuery fq;
    fq.amax = fq.nrm = fq.n32 = 0.0f;
    bool bad = false;
    const float scale = fr[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        float sc = 0.0f;
        if (d < k)
            sc = (qrow[d] - fr[d]) * scale;
        fq.n32 = fq.n32 + sc * sc;
        const _Float16 hval = (_Float16)sc;
        const float back = (float)hval;
        bad = bad || !(fabsf(back) < INFINITY);
        fq.amax = fmaxf(fq.amax, fabsf(back));
        fq.nrm = fq.nrm + back * back;
        b[d] = (_Float16)(back * -2.0f);
        bad = bad || !(fabsf((float)b[d]) < INFINITY);
    }
    fq.far = bad || !(fq.amax <= KNN_FRAME_AMAX);
    if (fq.far) {
#pragma unroll
        for (int d = 0; d < 16; ++d)
            b[d] = (_Float16)0.0f;
    }
    return fq;
}

// Seed score u (FINITE — the callers see to it: a real in-box row of the cell) -> Dup in the SHARD's scaled units, fp32 rounded up; +INF: no bound.
// Shared by both per-cell-frame forms of the prep kernel (the 1-NN form's cell_bound converts the cell's smallest score, the top-K
// form a list entry per lane): knn_threshold's Dup or the far branch's reach, over ratio^2, times 1 + 1e-6 for the double
// arithmetic, rounded up.
__host__ __device__ inline float knn_frame_dup(int k, float scale, float ratio, float bmaxc, float nmaxc, const KnnFrameQuery &fq, float u)
{
    const BoundConsts cst = knn_bound_consts(k, 1, scale, fq.far ? 0.0f : fq.amax, bmaxc, nmaxc);
    double dup = 0.0;
    if (fq.far) {
        const double reach = sqrt((double)fq.n32) * (1.0 + 1e-6) + sqrt((double)k) * (double)bmaxc * 1.001 + 0.001;
        dup = reach * reach * (1.0 + 1e-5) * (1.0 + cst.g2) * (1.0 + cst.g2) + cst.sigma2 * cst.tau;
        if (!(dup < 1e300))
            return INFINITY;
    } else {
        const float t = knn_threshold(cst, u, fq.nrm, &dup);
        if (!(t < INFINITY))
            return INFINITY;
    }
    dup = dup / ((double)ratio * (double)ratio) * (1.0 + 1e-6);
    float df = (float)dup;
    if ((double)df < dup)
        df = nextafterf(df, INFINITY);
    return df;
}
