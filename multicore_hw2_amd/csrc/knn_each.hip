// knn_each.hip — a radius per query (include/knn_mi355x.h 2j; DESIGN §4.6 "A radius per query"): the kernels of such a call that
// are not forms of a scan.  (The scans' each-forms live beside their scalar twins: knn_exact.hip, knn_self.hip, knn_grid.hip, and
// the cell-pruned way's preparation form in knn_cells.hip.)
//
// A row is a hit for query j when its v0 distance E is finite, E <= radii[j] and E <= cap: two fp32 compares, equality inside; a
// NaN or negative radius fails the first for every row.
#include "knn_exact_dev.h"

#include <math.h>

// The cell-pruned way's re-rank and out-of-box kernels with the radius of the record's (the block's) own query: the walks of
// knn_count_rerank_kernel, knn_count_outlier_kernel, knn_list_rerank_kernel and knn_list_outlier_kernel — the same body files
// (knn_rec_*_body.inc; knn_exact_dev.h) — in the form that reads radii.  qi is the pass's query number, and radii the pass's
// (CountCall::pass advances it with the queries).
#define KNN_REC_EACH_FORM /* what an each-form lacks: an own row */ \
    constexpr int FORM = KNN_REC_EACH;                              \
    constexpr const unsigned *mask = nullptr;                       \
    constexpr unsigned first = 0u
__global__ __launch_bounds__(KNN_BLOCK) void knn_count_each_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         long long n, const u64 *__restrict__ rec,
                                                                         const unsigned *__restrict__ counts, unsigned nlists,
                                                                         unsigned slice, unsigned *__restrict__ ctl,
                                                                         const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                         const float *__restrict__ radii, float cap,
                                                                         unsigned *__restrict__ qcount)
{
    KNN_REC_EACH_FORM;
#include "knn_rec_count_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_each_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                          unsigned count, const unsigned *__restrict__ list,
                                                                          const unsigned *__restrict__ ctl,
                                                                          const float *__restrict__ radii, float cap,
                                                                          unsigned *__restrict__ qcount)
{
#pragma clang fp contract(off)
    KNN_REC_EACH_FORM;
#include "knn_rec_count_outlier_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_each_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                        long long n, long long base, const u64 *__restrict__ rec,
                                                                        const unsigned *__restrict__ counts, unsigned nlists,
                                                                        unsigned slice, unsigned *__restrict__ ctl,
                                                                        const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                        const float *__restrict__ radii, float cap,
                                                                        const unsigned *__restrict__ gids,
                                                                        const u64 *__restrict__ offsets, unsigned *__restrict__ cursor,
                                                                        u64 *__restrict__ keys)
{
    KNN_REC_EACH_FORM;
#include "knn_rec_list_rerank_body.inc"
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_each_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         unsigned count, long long base, const unsigned *__restrict__ list,
                                                                         const unsigned *__restrict__ ctl,
                                                                         const float *__restrict__ radii, float cap,
                                                                         const unsigned *__restrict__ gids, const u64 *__restrict__ offsets,
                                                                         unsigned *__restrict__ cursor, u64 *__restrict__ keys)
{
#pragma clang fp contract(off)
    KNN_REC_EACH_FORM;
#include "knn_rec_list_outlier_body.inc"
}
#undef KNN_REC_EACH_FORM

// dist2[j] = the distance half of keys[j * K + column]; a padding key (KNN_KEY_INIT: +INF's bits) gives +INF by itself, and any
// other high word at or above +INF's bits — no call writes one — is read as +INF too, so the result is a radius or +INF, never NaN.
__global__ __launch_bounds__(KNN_BLOCK) void knn_keys_column_dist2_kernel(const u64 *__restrict__ keys, int m, int K, int column,
                                                                         float *__restrict__ dist2)
{
    const int j = blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (j >= m)
        return;
    const unsigned hi = (unsigned)(keys[(size_t)j * (size_t)K + (size_t)column] >> 32);
    dist2[j] = hi < 0x7F800000u ? __uint_as_float(hi) : INFINITY;
}

hipError_t knn_keys_column_dist2_launch(const u64 *keys, int m, int K, int column, float *dist2, hipStream_t s)
{
    if (m <= 0 || K < 1 || column < 0 || column >= K || !keys || !dist2)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_keys_column_dist2_kernel, dim3((unsigned)knn_divup(m, KNN_BLOCK)), dim3(KNN_BLOCK), 0, s, keys, m, K, column, dist2);
    return hipGetLastError();
}

// knn_count_records_finish for a pass with radii (c: the pass — its queries, its radii; the caller has checked rs): the same
// launches (knn_records_finish_launches) of the each-forms.
hipError_t knn_count_each_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount)
{
    hipStream_t s = c.stream;
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_count_each_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rec, counts, nlists,
                               slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, qcount);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_count_each_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, rs.outliers,
                               (const unsigned *)rs.ctl, c.radii, c.max_dist2, qcount);
        },
        [&] { return knn_count_commit_launch(c.m, qcount, c.counts, rs.ctl + KNN_CTL_FALLBACK, s); });
}

// knn_list_records_finish for a pass with radii.
hipError_t knn_list_each_records_finish(const ListCall &c, const TopkRecords &rs)
{
    hipStream_t s = c.stream;
    return knn_records_finish_launches(
        rs, c.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_list_each_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rec, counts,
                               nlists, slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, c.gids, c.offsets, c.scratch, c.keys);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_list_each_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, c.base, rs.outliers,
                               (const unsigned *)rs.ctl, c.radii, c.max_dist2, c.gids, c.offsets, c.scratch, c.keys);
        },
        [&] { return knn_list_commit_launch(c.m, c.scratch, c.fill, rs.ctl + KNN_CTL_FALLBACK, s); });
}
