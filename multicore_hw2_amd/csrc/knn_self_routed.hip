// knn_self_routed.hip — the radius graph on the cell-pruned way (include/knn_mi355x.h 2k; DESIGN §4.6 "The radius graph on the
// pruned ways"): the kernels behind a pass's record-only scan that turn records into hits, in the form that knows the query is a
// row of the shard.  (The grid way's self forms live beside their twins in knn_grid.hip, the gated self-scans in knn_self.hip.)
//
// The pass's front — prep, match, record-only scan — is the plain count pass's, launched with Q = R + first * k: it neither knows
// nor needs to know that a query is a row.  Its records name every row that may lie within the query's bound, the query's own row
// among them.  The four kernels here are knn_each.hip's — the same body files (knn_rec_*_body.inc; knn_exact_dev.h), FORM =
// KNN_REC_SELF — with one compare more on the hit side, behind the
// distance: a candidate whose LOCAL row is first + qi (qi: the pass's query number, first: the pass's first own row) is dropped.
// Identity is by local row number, so another copy of the row stays a hit at distance 0.  radii null is the scalar form: every
// query's radius is the cap.  A hit: E finite, E <= radius and E <= cap, two fp32 compares (knn_each_radius.h says the same of the
// bound); a NaN or negative radius fails the first for every row.
#include "knn_exact_dev.h"

#include <math.h>

#define KNN_REC_SELF_FORM /* what a self form lacks: a row mask */ \
    constexpr int FORM = KNN_REC_SELF;                             \
    constexpr const unsigned *mask = nullptr

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_self_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         long long n, const u64 *__restrict__ rec,
                                                                         const unsigned *__restrict__ counts, unsigned nlists,
                                                                         unsigned slice, unsigned *__restrict__ ctl,
                                                                         const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                         const float *__restrict__ radii, float cap, unsigned first,
                                                                         unsigned *__restrict__ qcount)
{
    KNN_REC_SELF_FORM;
#include "knn_rec_count_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_self_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                          unsigned count, const unsigned *__restrict__ list,
                                                                          const unsigned *__restrict__ ctl,
                                                                          const float *__restrict__ radii, float cap, unsigned first,
                                                                          unsigned *__restrict__ qcount)
{
#pragma clang fp contract(off)
    KNN_REC_SELF_FORM;
#include "knn_rec_count_outlier_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_self_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                        long long n, long long base, const u64 *__restrict__ rec,
                                                                        const unsigned *__restrict__ counts, unsigned nlists,
                                                                        unsigned slice, unsigned *__restrict__ ctl,
                                                                        const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                        const float *__restrict__ radii, float cap, unsigned first,
                                                                        const unsigned *__restrict__ gids,
                                                                        const u64 *__restrict__ offsets, unsigned *__restrict__ cursor,
                                                                        u64 *__restrict__ keys)
{
    KNN_REC_SELF_FORM;
#include "knn_rec_list_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_self_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         unsigned count, long long base, const unsigned *__restrict__ list,
                                                                         const unsigned *__restrict__ ctl,
                                                                         const float *__restrict__ radii, float cap, unsigned first,
                                                                         const unsigned *__restrict__ gids, const u64 *__restrict__ offsets,
                                                                         unsigned *__restrict__ cursor, u64 *__restrict__ keys)
{
#pragma clang fp contract(off)
    KNN_REC_SELF_FORM;
#include "knn_rec_list_outlier_body.inc"
}
#undef KNN_REC_SELF_FORM

// knn_count_each_records_finish for a pass of a routed self call (c: the pass — c.self_first its first own row, c.q the rows
// themselves; the caller has checked rs): the same launches (knn_records_finish_launches) of the self forms.
hipError_t knn_count_self_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount)
{
    hipStream_t s = c.stream;
    if (c.mask || c.self_first < 0 || c.self_first + c.m > c.n || c.q != c.r + (size_t)c.self_first * c.k)
        return hipErrorInvalidValue;
    const unsigned first = (unsigned)c.self_first;
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_count_self_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rec, counts, nlists,
                               slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, first, qcount);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_count_self_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, rs.outliers,
                               (const unsigned *)rs.ctl, c.radii, c.max_dist2, first, qcount);
        },
        [&] { return knn_count_commit_launch(c.m, qcount, c.counts, rs.ctl + KNN_CTL_FALLBACK, s); });
}

// knn_list_each_records_finish for a pass of a routed self call.
hipError_t knn_list_self_records_finish(const ListCall &c, const TopkRecords &rs)
{
    hipStream_t s = c.stream;
    if (c.mask || c.self_first < 0 || c.self_first + c.m > c.n || c.q != c.r + (size_t)c.self_first * c.k)
        return hipErrorInvalidValue;
    const unsigned first = (unsigned)c.self_first;
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_list_self_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rec, counts,
                               nlists, slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, first, c.gids, c.offsets, c.scratch,
                               c.keys);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_list_self_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, c.base, rs.outliers,
                               (const unsigned *)rs.ctl, c.radii, c.max_dist2, first, c.gids, c.offsets, c.scratch, c.keys);
        },
        [&] { return knn_list_commit_launch(c.m, c.scratch, c.fill, rs.ctl + KNN_CTL_FALLBACK, s); });
}
