// knn_each.hip — a radius per query (include/knn_mi355x.h 2j; DESIGN §4.6 "A radius per query"): the kernels of such a call that
// are not forms of a scan.  (The scans' each-forms live beside their scalar twins: knn_exact.hip, knn_self.hip, knn_grid.hip, and
// the cell-pruned way's preparation form in knn_cells.hip.)
//
// A row is a hit for query j when its v0 distance E is finite, E <= radii[j] and E <= cap: two fp32 compares, equality inside; a
// NaN or negative radius fails the first for every row.
#include "knn_exact_dev.h"

#include <math.h>

// The cell-pruned way's re-rank and out-of-box kernels with the radius of the record's (the block's) own query: the walks of
// knn_count_rerank_kernel, knn_count_outlier_kernel, knn_list_rerank_kernel and knn_list_outlier_kernel, line for line.  qi is the
// pass's query number, and radii the pass's (CountCall::pass advances it with the queries).
__global__ __launch_bounds__(KNN_BLOCK) void knn_count_each_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         long long n, const u64 *__restrict__ rec,
                                                                         const unsigned *__restrict__ counts, unsigned nlists,
                                                                         unsigned slice, unsigned *__restrict__ ctl,
                                                                         const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                         const float *__restrict__ radii, float cap,
                                                                         unsigned *__restrict__ qcount)
{
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
                hit = d <= radii[qi] && d <= cap;
            }
        }
        const u64 hits = __ballot(hit);
        const unsigned mine = (unsigned)__popcll((hits >> (lane & 48u)) & 0xFFFFull);
        if ((lane & 15u) == 0u && mine != 0u)
            atomicAdd(&qcount[qi], mine);
    }
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_each_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                          unsigned count, const unsigned *__restrict__ list,
                                                                          const unsigned *__restrict__ ctl,
                                                                          const float *__restrict__ radii, float cap,
                                                                          unsigned *__restrict__ qcount)
{
#pragma clang fp contract(off)
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    const float rad = radii[q];
    unsigned cnt = 0u;
    for (unsigned j = blockIdx.x * KNN_BLOCK + threadIdx.x; j < count; j += gridDim.x * KNN_BLOCK) {
        const float *__restrict__ r = R + (size_t)list[j] * k;
        float acc = 0.0f;
        for (int d = 0; d < k; ++d) {
            const float diff = qp[d] - r[d];
            const float sq = diff * diff;
            acc = acc + sq;
        }
        cnt += acc < INFINITY && acc <= rad && acc <= cap ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        cnt += (unsigned)__shfl_xor((int)cnt, off, KNN_WAVE);
    if ((threadIdx.x & 63u) == 0u && cnt != 0u)
        atomicAdd(&qcount[q], cnt);
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
        const u64 key = rerank_pair<0>(Q, R, k, n, base, e, reg, rmask, 0u, perm, qi);   // ~0: nothing there, or not finite
        if (key == ~0ull)
            continue;
        const float d = __uint_as_float((unsigned)(key >> 32));
        if (d <= radii[qi] && d <= cap) {
            u64 off;
            const unsigned room = list_room(offsets, qi, off);
            list_put(&cursor[qi], keys, off, room, gids ? (key & 0xFFFFFFFF00000000ull) | (u64)gids[(unsigned)key] : key);
        }
    }
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_each_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         unsigned count, long long base, const unsigned *__restrict__ list,
                                                                         const unsigned *__restrict__ ctl,
                                                                         const float *__restrict__ radii, float cap,
                                                                         const unsigned *__restrict__ gids, const u64 *__restrict__ offsets,
                                                                         unsigned *__restrict__ cursor, u64 *__restrict__ keys)
{
#pragma clang fp contract(off)
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    const float rad = radii[q];
    u64 off;
    const unsigned room = list_room(offsets, q, off);
    for (unsigned j = blockIdx.x * KNN_BLOCK + threadIdx.x; j < count; j += gridDim.x * KNN_BLOCK) {
        const unsigned row = list[j];
        const float *__restrict__ r = R + (size_t)row * k;
        float acc = 0.0f;
        for (int d = 0; d < k; ++d) {
            const float diff = qp[d] - r[d];
            const float sq = diff * diff;
            acc = acc + sq;
        }
        if (acc < INFINITY && acc <= rad && acc <= cap)
            list_put(&cursor[q], keys, off, room, pack_key(acc, gids ? gids[row] : (unsigned)(base + (long long)row)));
    }
}

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

// knn_count_records_finish for a pass with radii (c: the pass — its queries, its radii; the caller has checked rs): the same walks,
// then the same commit.
hipError_t knn_count_each_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount)
{
    hipStream_t s = c.stream;
    if (rs.nlists)
        hipLaunchKernelGGL(knn_count_each_rerank_kernel, dim3(rs.nlists), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rs.rec,
                           rs.counts, rs.nlists, rs.slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, qcount);
    if (rs.ovf_rec && rs.ovf_count)   // the shared overflow area as a list of one
        hipLaunchKernelGGL(knn_count_each_rerank_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rs.ovf_rec,
                           rs.ovf_count, 1u, rs.ovf_slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, qcount);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (rs.n_outliers) {
        const unsigned gx = (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK < 64u ? (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK : 64u;
        hipLaunchKernelGGL(knn_count_each_outlier_kernel, dim3(gx, (unsigned)c.m), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers,
                           rs.outliers, (const unsigned *)rs.ctl, c.radii, c.max_dist2, qcount);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return knn_count_commit_launch(c.m, qcount, c.counts, rs.ctl + KNN_CTL_FALLBACK, s);
}

// knn_list_records_finish for a pass with radii.
hipError_t knn_list_each_records_finish(const ListCall &c, const TopkRecords &rs)
{
    hipStream_t s = c.stream;
    if (rs.nlists)
        hipLaunchKernelGGL(knn_list_each_rerank_kernel, dim3(rs.nlists), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rs.rec,
                           rs.counts, rs.nlists, rs.slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, c.gids, c.offsets, c.scratch,
                           c.keys);
    if (rs.ovf_rec && rs.ovf_count)   // the shared overflow area as a list of one
        hipLaunchKernelGGL(knn_list_each_rerank_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rs.ovf_rec,
                           rs.ovf_count, 1u, rs.ovf_slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, c.gids, c.offsets, c.scratch,
                           c.keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (rs.n_outliers) {
        const unsigned gx = (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK < 64u ? (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK : 64u;
        hipLaunchKernelGGL(knn_list_each_outlier_kernel, dim3(gx, (unsigned)c.m), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, c.base,
                           rs.outliers, (const unsigned *)rs.ctl, c.radii, c.max_dist2, c.gids, c.offsets, c.scratch, c.keys);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return knn_list_commit_launch(c.m, c.scratch, c.fill, rs.ctl + KNN_CTL_FALLBACK, s);
}
