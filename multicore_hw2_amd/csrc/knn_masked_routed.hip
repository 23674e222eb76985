// knn_masked_routed.hip — counts and lists within a radius over a subset of the rows on the cell-pruned way (include/knn_mi355x.h
// 2l; DESIGN §4.6 "Over a subset of the rows, on the pruned ways"): the kernels behind a pass's record-only scan that turn records
// into hits, in the form that knows of a row mask.  (The grid way's masked forms live beside their twins in knn_grid.hip, the gated
// masked scans in knn_masked.hip and knn_masked_lists.hip.)
//
// The pass's front — prep, match, record-only scan — is the plain count pass's, untouched: it neither knows nor needs to know of
// the mask, and its records name every row that may lie within the radius, the masked-out ones among them.  The four kernels
// here are knn_exact.hip's scalar forms — the same body files (knn_rec_*_body.inc; knn_exact_dev.h), FORM = KNN_REC_MASKED — with
// one bit test more: a candidate whose LOCAL row's bit in the mask is clear is dropped.  The re-rank kernels test behind the
// distance compares, so only rows inside the radius pay the gather; the out-of-box kernels test before the distance is accumulated
// (they hold the row number first).  The mask is the caller's, in the shard's local row order whatever the layout's order is: the
// records reach a row through perm, which gives that number.  It is the same for every pass of a call.
#include "knn_exact_dev.h"

#include <math.h>

#define KNN_REC_MASKED_FORM /* what a masked form lacks: radii, an own row */ \
    constexpr int FORM = KNN_REC_MASKED;                                      \
    constexpr const float *radii = nullptr;                                   \
    constexpr unsigned first = 0u;                                            \
    const float cap = max_dist2

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_masked_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                           long long n, const u64 *__restrict__ rec,
                                                                           const unsigned *__restrict__ counts, unsigned nlists,
                                                                           unsigned slice, unsigned *__restrict__ ctl,
                                                                           const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                           float max_dist2, const unsigned *__restrict__ mask,
                                                                           unsigned *__restrict__ qcount)
{
    KNN_REC_MASKED_FORM;
#include "knn_rec_count_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_masked_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                            unsigned count, const unsigned *__restrict__ list,
                                                                            const unsigned *__restrict__ ctl, float max_dist2,
                                                                            const unsigned *__restrict__ mask, unsigned *__restrict__ qcount)
{
#pragma clang fp contract(off)
    KNN_REC_MASKED_FORM;
#include "knn_rec_count_outlier_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_masked_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                          long long n, long long base, const u64 *__restrict__ rec,
                                                                          const unsigned *__restrict__ counts, unsigned nlists,
                                                                          unsigned slice, unsigned *__restrict__ ctl,
                                                                          const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                          float max_dist2, const unsigned *__restrict__ mask,
                                                                          const unsigned *__restrict__ gids,
                                                                          const u64 *__restrict__ offsets, unsigned *__restrict__ cursor,
                                                                          u64 *__restrict__ keys)
{
    KNN_REC_MASKED_FORM;
#include "knn_rec_list_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_masked_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                           unsigned count, long long base, const unsigned *__restrict__ list,
                                                                           const unsigned *__restrict__ ctl, float max_dist2,
                                                                           const unsigned *__restrict__ mask,
                                                                           const unsigned *__restrict__ gids, const u64 *__restrict__ offsets,
                                                                           unsigned *__restrict__ cursor, u64 *__restrict__ keys)
{
#pragma clang fp contract(off)
    KNN_REC_MASKED_FORM;
#include "knn_rec_list_outlier_body.inc"
}
#undef KNN_REC_MASKED_FORM

// knn_count_records_finish for a pass of a routed masked call (c: the pass — c.mask the shard's mask, the same for every pass;
// the caller has checked rs): the same launches (knn_records_finish_launches) of the masked forms.
hipError_t knn_count_masked_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount)
{
    hipStream_t s = c.stream;
    if (!c.mask || c.radii || c.self_first >= 0)
        return hipErrorInvalidValue;
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_count_masked_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rec, counts, nlists,
                               slice, rs.ctl, rs.perm, rs.pos_norms, c.max_dist2, c.mask, qcount);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_count_masked_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, rs.outliers,
                               (const unsigned *)rs.ctl, c.max_dist2, c.mask, qcount);
        },
        [&] { return knn_count_commit_launch(c.m, qcount, c.counts, rs.ctl + KNN_CTL_FALLBACK, s); });
}

// knn_list_records_finish for a pass of a routed masked call.
hipError_t knn_list_masked_records_finish(const ListCall &c, const TopkRecords &rs)
{
    hipStream_t s = c.stream;
    if (!c.mask || c.radii || c.self_first >= 0)
        return hipErrorInvalidValue;
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_list_masked_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rec, counts,
                               nlists, slice, rs.ctl, rs.perm, rs.pos_norms, c.max_dist2, c.mask, c.gids, c.offsets, c.scratch, c.keys);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_list_masked_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, c.base,
                               rs.outliers, (const unsigned *)rs.ctl, c.max_dist2, c.mask, c.gids, c.offsets, c.scratch, c.keys);
        },
        [&] { return knn_list_commit_launch(c.m, c.scratch, c.fill, rs.ctl + KNN_CTL_FALLBACK, s); });
}
