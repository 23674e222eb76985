// knn_cluster_routed.hip — the link sweep of a cluster call on the cell-pruned way (include/knn_mi355x.h 2n; DESIGN §4.6 "Clusters
// on the cell-pruned way"): the two kernels behind a pass's record-only scan that turn its records and the layout's out-of-box
// rows into unite calls and border keys.  (knn_cluster.hip describes the call, its exact link sweep and the gated twin that runs
// behind these two; knn_cluster_uf.h the union-find; knn_cluster_pair.h the decision per hit.)
//
// The pass's front — prep, match, record-only scan — is the count pass's, launched with Q = R + first * k: its records name every
// row that may lie within max_dist2 of a query, the query's own row among them.  A pass owns the rows first .. first + m - 1 and is
// SELF-CONTAINED: it unites exactly the pairs whose larger row it owns (both core, row < own) and sets exactly its own rows'
// border keys.  The pair (row, own) with row > own is the business of the pass that owns `row`, which meets `own` among ITS
// records: E is symmetric bit for bit.  So a pass that falls back — swept whole by the gated exact twin over its own window —
// touches no other pass's work.
//
// No commit step: unite and the atomic minimum are idempotent and commute (knn_cluster.hip), so whatever these kernels did before
// one of them raised FALLBACK stays, and the twin's sweep over it gives the exact sweep's forest and keys.
//
// The re-rank walks the records as knn_rec_count_rerank_body.inc does — one block per list, rerank_pair<0> through perm, positions
// whose layout norm is +INF skipped, want > slice raises FALLBACK.  The 16 rows of a record sit on 16 neighbouring lanes and
// belong to ONE query: their border keys are reduced to the record's smallest across those lanes (four xor-shuffles, no LDS round
// trip), and the record's first lane issues one atomic minimum when something was folded.  The core bit of `row` differs per lane:
// a vector load, not the exact kernel's scalar one.  The unite is skipped when parent[row] and parent[own] load the same value —
// both then hang under one member, the pair is done; a shortcut that may miss and never lies.  Every lane of a wave reaches every
// shuffle: the hit path sits inside the lane's own branch, the reduction outside it, and every wave runs the same number of rounds.
#include "knn_exact_dev.h"
#include "knn_cluster_uf.h"
#include "knn_cluster_pair.h"

#include <math.h>

__device__ __forceinline__ bool cluster_core_bit(const unsigned *__restrict__ core, unsigned row)
{
    return ((core[row >> 5] >> (row & 31u)) & 1u) != 0u;
}

// One hit (own, row) at distance bits `key >> 32` (key: pack_key(E, row), E finite and <= max_dist2, row != own): the unite, or
// the key to fold into own's smallest (kKeyInit: nothing — a key of a finite E lies below it).
__device__ __forceinline__ u64 cluster_link_hit(int *parent, const unsigned *__restrict__ core, bool own_core, unsigned own, u64 key)
{
    const unsigned row = (unsigned)key;
    const int action = knn_cluster_pair(own_core, cluster_core_bit(core, row), (long long)row, (long long)own);
    if (action == KNN_PAIR_UNITE) {
        if (KnnUfDevice::load(&parent[row]) != KnnUfDevice::load(&parent[own]))
            (void)knn_uf_unite<KnnUfDevice>(parent, (int)row, (int)own);
        return kKeyInit;
    }
    return action == KNN_PAIR_BORDER ? key : kKeyInit;
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_cluster_link_rerank_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                           long long n, const u64 *__restrict__ rec,
                                                                           const unsigned *__restrict__ counts, unsigned nlists,
                                                                           unsigned slice, unsigned *__restrict__ ctl,
                                                                           const unsigned *__restrict__ perm, const float *__restrict__ norms,
                                                                           float cap, unsigned first, unsigned m, int *parent,
                                                                           const unsigned *__restrict__ core, u64 *__restrict__ best)
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
    // (every wave runs the same number of rounds: the shuffles below are taken by all 64 lanes)
    for (unsigned c0 = 0u; c0 < nrec * 16u; c0 += KNN_BLOCK) {
        const unsigned c = c0 + threadIdx.x;
        u64 near = kKeyInit;
        unsigned qi = 0u;
        if (c < nrec * 16u) {
            const u64 e = list[c >> 4];
            const unsigned lo = (unsigned)e, reg = c & 15u;
            const long long pos = (long long)(lo >> 1) * 32 + 8 * (reg >> 2) + 4 * (lo & 1u) + (reg & 3u);   // (rerank_pair's)
            const unsigned rmask = pos < n && norms[pos] < INFINITY ? 0xFFFFu : 0u;
            const u64 key = rerank_pair<0>(Q, R, k, n, 0ll, e, reg, rmask, 0u, perm, qi);   // ~0: nothing there, or not finite
            if (key != ~0ull) {
                const float d = __uint_as_float((unsigned)(key >> 32));
                const unsigned own = first + qi;
                if (qi < m && d <= cap && (unsigned)key != own)   // (a record names a query of the pass; the key's low word: the LOCAL row, base 0)
                    near = cluster_link_hit(parent, core, cluster_core_bit(core, own), own, key);
            }
        }
        // the record's smallest key: its 16 lanes, one query (the xor distances stay inside the 16)
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(near, off, KNN_WAVE);
            near = o < near ? o : near;
        }
        if ((lane & 15u) == 0u && near != kKeyInit)
            key_atomic_min(&best[first + qi], near);
    }
}

// The layout's out-of-box rows never enter the scan: every (query, listed row) pair once, with v0's arithmetic
// (knn_rec_count_outlier_body.inc's walk).  grid (row blocks, queries): `own` and its core bit are the block's; a thread folds its
// rows' border keys, a wave reduces them and its first lane issues the one atomic minimum.
__global__ __launch_bounds__(KNN_BLOCK) void knn_cluster_link_outlier_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                            unsigned count, const unsigned *__restrict__ list,
                                                                            const unsigned *__restrict__ ctl, float cap, unsigned first,
                                                                            int *parent, const unsigned *__restrict__ core,
                                                                            u64 *__restrict__ best)
{
#pragma clang fp contract(off)
    if (ctl[KNN_CTL_FALLBACK] != 0u)
        return;
    const unsigned q = blockIdx.y;
    const float *__restrict__ qp = Q + (size_t)q * k;
    const unsigned own = first + q;
    const bool own_core = cluster_core_bit(core, own);
    u64 near = kKeyInit;
    for (unsigned j = blockIdx.x * KNN_BLOCK + threadIdx.x; j < count; j += gridDim.x * KNN_BLOCK) {
        const unsigned row = list[j];
        const float *__restrict__ r = R + (size_t)row * k;
        float acc = 0.0f;
        for (int d = 0; d < k; ++d) {
            const float diff = qp[d] - r[d];
            const float sq = diff * diff;
            acc = acc + sq;
        }
        if (acc < INFINITY && acc <= cap && row != own) {   // (NaN fails both compares)
            const u64 key = cluster_link_hit(parent, core, own_core, own, pack_key(acc, row));
            near = key < near ? key : near;
        }
    }
    near = wave_min_u64(near);   // (behind the loop: all 64 lanes are here)
    if ((threadIdx.x & 63u) == 0u && near != kKeyInit)
        key_atomic_min(&best[own], near);
}

// The two kernels for a pass (p.first, p.m: its own rows; the caller has made rs from the pass's workspace and queues the gated
// exact twin behind): the launches of every record pass (knn_records_finish_launches) with nothing to commit.
hipError_t knn_cluster_link_records_finish(const ClusterPass &p, const TopkRecords &rs)
{
    const ClusterCall &c = p.c;
    hipStream_t s = c.stream;
    if (c.n <= 0 || c.n > 0x7FFFFFFFll || !c.r || !c.parent || !c.core || !c.best || p.first < 0 || p.m < 1 || p.first + p.m > c.n ||
        !(c.max_dist2 < INFINITY))
        return hipErrorInvalidValue;
    const float *q = c.r + (size_t)p.first * c.k;
    const unsigned first = (unsigned)p.first;
    return knn_records_finish_launches(
        rs, p.m,
        [&](dim3 grid, const u64 *rec, const unsigned *counts, unsigned nlists, unsigned slice) {
            hipLaunchKernelGGL(knn_cluster_link_rerank_kernel, grid, dim3(KNN_BLOCK), 0, s, q, c.r, c.k, rs.positions, rec, counts, nlists,
                               slice, rs.ctl, rs.perm, rs.pos_norms, c.max_dist2, first, (unsigned)p.m, c.parent, (const unsigned *)c.core,
                               c.best);
        },
        [&](dim3 grid) {
            hipLaunchKernelGGL(knn_cluster_link_outlier_kernel, grid, dim3(KNN_BLOCK), 0, s, q, c.r, c.k, rs.n_outliers, rs.outliers,
                               (const unsigned *)rs.ctl, c.max_dist2, first, c.parent, (const unsigned *)c.core, c.best);
        },
        [] { return hipSuccess; });
}
