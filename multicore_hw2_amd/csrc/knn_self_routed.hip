// knn_self_routed.hip — the radius graph on the cell-pruned way (include/knn_mi355x.h 2k; DESIGN §4.6 "The radius graph on the
// pruned ways"): the kernels behind a pass's record-only scan that turn records into hits, in the form that knows the query is a
// row of the shard.  (The grid way's self forms live beside their twins in knn_grid.hip, the gated self-scans in knn_self.hip.)
//
// The pass's front — prep, match, record-only scan — is the plain count pass's, launched with Q = R + first * k: it neither knows
// nor needs to know that a query is a row.  Its records name every row that may lie within the query's bound, the query's own row
// among them.  The four kernels here are knn_each.hip's — the walks of knn_count_each_rerank_kernel, knn_count_each_outlier_kernel,
// knn_list_each_rerank_kernel and knn_list_each_outlier_kernel, line for line — with one compare more on the hit side, behind the
// distance: a candidate whose LOCAL row is first + qi (qi: the pass's query number, first: the pass's first own row) is dropped.
// Identity is by local row number, so another copy of the row stays a hit at distance 0.  radii null is the scalar form: every
// query's radius is the cap.  A hit: E finite, E <= radius and E <= cap, two fp32 compares (knn_each_radius.h says the same of the
// bound); a NaN or negative radius fails the first for every row.
#include "knn_exact_dev.h"

#include <math.h>

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_self_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         long long n, const u64 *__restrict__ rec,
                                                                         const unsigned *__restrict__ counts, unsigned nlists,
                                                                         unsigned slice, unsigned *__restrict__ ctl,
                                                                         const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                         const float *__restrict__ radii, float cap, unsigned first,
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
            if (key != ~0ull) {   // (base 0: the key's low word is the LOCAL row)
                const float d = __uint_as_float((unsigned)(key >> 32));
                const float rad = radii ? radii[qi] : cap;
                hit = d <= rad && d <= cap && (unsigned)key != first + qi;
            }
        }
        const u64 hits = __ballot(hit);
        const unsigned mine = (unsigned)__popcll((hits >> (lane & 48u)) & 0xFFFFull);
        if ((lane & 15u) == 0u && mine != 0u)
            atomicAdd(&qcount[qi], mine);
    }
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_count_self_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                          unsigned count, const unsigned *__restrict__ list,
                                                                          const unsigned *__restrict__ ctl,
                                                                          const float *__restrict__ radii, float cap, unsigned first,
                                                                          unsigned *__restrict__ qcount)
{
#pragma clang fp contract(off)
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    const float rad = radii ? radii[q] : cap;
    const unsigned own = first + q;
    unsigned cnt = 0u;
    for (unsigned j = blockIdx.x * KNN_BLOCK + threadIdx.x; j < count; j += gridDim.x * KNN_BLOCK) {
        const unsigned row = list[j];
        const float *__restrict__ r = R + (size_t)row * k;
        float acc = 0.0f;
        for (int d = 0; d < k; ++d) {
            const float diff = qp[d] - r[d];
            const float sq = diff * diff;
            acc = acc + sq;
        }
        cnt += acc < INFINITY && acc <= rad && acc <= cap && row != own ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        cnt += (unsigned)__shfl_xor((int)cnt, off, KNN_WAVE);
    if ((threadIdx.x & 63u) == 0u && cnt != 0u)
        atomicAdd(&qcount[q], cnt);
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
        const u64 key = rerank_pair<0>(Q, R, k, n, 0ll, e, reg, rmask, 0u, perm, qi);   // ~0: nothing there, or not finite
        if (key == ~0ull)
            continue;
        const unsigned row = (unsigned)key;   // (base 0: the LOCAL row; the number the key carries is made below)
        const float d = __uint_as_float((unsigned)(key >> 32));
        const float rad = radii ? radii[qi] : cap;
        if (d <= rad && d <= cap && row != first + qi) {
            u64 off;
            const unsigned room = list_room(offsets, qi, off);
            list_put(&cursor[qi], keys, off, room,
                     (key & 0xFFFFFFFF00000000ull) | (u64)(gids ? gids[row] : (unsigned)(base + (long long)row)));
        }
    }
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_list_self_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                         unsigned count, long long base, const unsigned *__restrict__ list,
                                                                         const unsigned *__restrict__ ctl,
                                                                         const float *__restrict__ radii, float cap, unsigned first,
                                                                         const unsigned *__restrict__ gids, const u64 *__restrict__ offsets,
                                                                         unsigned *__restrict__ cursor, u64 *__restrict__ keys)
{
#pragma clang fp contract(off)
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    const float rad = radii ? radii[q] : cap;
    const unsigned own = first + q;
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
        if (acc < INFINITY && acc <= rad && acc <= cap && row != own)
            list_put(&cursor[q], keys, off, room, pack_key(acc, gids ? gids[row] : (unsigned)(base + (long long)row)));
    }
}

// knn_count_each_records_finish for a pass of a routed self call (c: the pass — c.self_first its first own row, c.q the rows
// themselves; the caller has checked rs): the same walks, then the same commit.
hipError_t knn_count_self_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount)
{
    hipStream_t s = c.stream;
    if (c.self_first < 0 || c.self_first + c.m > c.n || c.q != c.r + (size_t)c.self_first * c.k)
        return hipErrorInvalidValue;
    const unsigned first = (unsigned)c.self_first;
    if (rs.nlists)
        hipLaunchKernelGGL(knn_count_self_rerank_kernel, dim3(rs.nlists), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rs.rec,
                           rs.counts, rs.nlists, rs.slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, first, qcount);
    if (rs.ovf_rec && rs.ovf_count)   // the shared overflow area as a list of one
        hipLaunchKernelGGL(knn_count_self_rerank_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, rs.ovf_rec,
                           rs.ovf_count, 1u, rs.ovf_slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, first, qcount);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (rs.n_outliers) {
        const unsigned gx = (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK < 64u ? (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK : 64u;
        hipLaunchKernelGGL(knn_count_self_outlier_kernel, dim3(gx, (unsigned)c.m), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers,
                           rs.outliers, (const unsigned *)rs.ctl, c.radii, c.max_dist2, first, qcount);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return knn_count_commit_launch(c.m, qcount, c.counts, rs.ctl + KNN_CTL_FALLBACK, s);
}

// knn_list_each_records_finish for a pass of a routed self call.
hipError_t knn_list_self_records_finish(const ListCall &c, const TopkRecords &rs)
{
    hipStream_t s = c.stream;
    if (c.self_first < 0 || c.self_first + c.m > c.n || c.q != c.r + (size_t)c.self_first * c.k)
        return hipErrorInvalidValue;
    const unsigned first = (unsigned)c.self_first;
    if (rs.nlists)
        hipLaunchKernelGGL(knn_list_self_rerank_kernel, dim3(rs.nlists), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rs.rec,
                           rs.counts, rs.nlists, rs.slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, first, c.gids, c.offsets,
                           c.scratch, c.keys);
    if (rs.ovf_rec && rs.ovf_count)   // the shared overflow area as a list of one
        hipLaunchKernelGGL(knn_list_self_rerank_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.positions, c.base, rs.ovf_rec,
                           rs.ovf_count, 1u, rs.ovf_slice, rs.ctl, rs.perm, rs.pos_norms, c.radii, c.max_dist2, first, c.gids, c.offsets,
                           c.scratch, c.keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (rs.n_outliers) {
        const unsigned gx = (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK < 64u ? (rs.n_outliers + KNN_BLOCK - 1) / KNN_BLOCK : 64u;
        hipLaunchKernelGGL(knn_list_self_outlier_kernel, dim3(gx, (unsigned)c.m), dim3(KNN_BLOCK), 0, s, c.q, c.r, c.k, rs.n_outliers, c.base,
                           rs.outliers, (const unsigned *)rs.ctl, c.radii, c.max_dist2, first, c.gids, c.offsets, c.scratch, c.keys);
        e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return knn_list_commit_launch(c.m, c.scratch, c.fill, rs.ctl + KNN_CTL_FALLBACK, s);
}
