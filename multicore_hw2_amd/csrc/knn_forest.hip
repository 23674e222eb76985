// knn_forest.hip — the minimum spanning forest of the shard's own rows on the radius graph (include/knn_mi355x.h 2o; DESIGN §4.6
// "Minimum spanning forest"): the rounds of knn_index_self_forest_within.  (The grid way's scan kernel lives in knn_grid.hip, on
// grid_walk, the ring walk of that file's kernels; the pick and the hook's decision lines in knn_forest_pick.h; the union-find in knn_cluster_uf.h.)
//
// Borůvka, ROUNDS(n) = max(1, ceil(log2 n)) rounds, all queued on one stream with no host round trip.  Every kernel of round
// t > 0 starts with "*gate == 0 -> return" on the word round t - 1's emit raises when it stores an edge: a forest that is
// finished early costs empty launches only.  One round, all in the caller's labels array and the slot's scratch:
//   1. flatten   labels[i] = root(i) in place (round 0: i), cand[i] = KNN_KEY_INIT, the pick slots empty.  A depth-1 forest is a
//                valid forest, and from here to the emit the labels are FROZEN: the scan and the pick only read them.
//   2. scan      knn_forest_scan_kernel<KC>: knn_cluster_link_kernel<KC>'s skeleton (one wave per block, lanes = own rows, row i
//                wave-uniform, self_scan_one) with the hit path "other && live && acc < INF && acc <= max_dist2 && labels[row]
//                != my label" -> fold pack_key(acc, row) into the lane's minimum; ONE key_atomic_min on cand[own] at the end,
//                only when something was folded.  For a fixed own row the smallest (E, row) key is also the smallest (E, lo, hi)
//                edge: a candidate row below own beats any above it at equal E.
//   3. pick      two launches (knn_forest_pick.h: offer 1, offer 2).  The first also marks a row WITHOUT a candidate done: it has
//                none in any later round, because components only grow.  A scan wave whose live lanes are all done returns.
//   4. hook      emit (the edge list, the next round's gate), then unite — two launches, because the unite is the first writer
//                of labels and the emit needs them frozen.
// Behind the last round one more flatten, gated on the word that round's emit raised: a hook re-parents only the larger root, so
// when the LAST queued round still added an edge (rows paired at every level: every round halves the components exactly) no
// later round's flatten would bring the labels back to depth 1.
// On the grid way step 2 is knn_grid_forest_scan_kernel followed by this file's scan gated on the round's give-up word as well:
// the atomic min is idempotent, so nothing is committed.
#include "knn_self_scan.h"
#include "knn_forest_pick.h"
#include "knn_slice_launch.h"

#define KNN_FOREST_BLOCK 256

__global__ __launch_bounds__(KNN_FOREST_BLOCK) void knn_forest_flatten_kernel(int *labels, long long n, int start, u64 *__restrict__ cand,
                                                                             u64 *__restrict__ pick1, unsigned *__restrict__ pick2,
                                                                             const unsigned *__restrict__ gate, unsigned *__restrict__ stat)
{
    if (gate && *gate == 0u)
        return;
    const long long i = (long long)blockIdx.x * KNN_FOREST_BLOCK + threadIdx.x;
    if (i == 0)
        *stat = 0u;   // (this round runs: the word speaks of it from here on)
    if (i >= n)
        return;
    if (start)
        labels[i] = (int)i;
    else
        knn_forest_flatten<KnnPickDevice>(labels, i);
    cand[i] = kKeyInit;
    knn_forest_clear(pick1, pick2, i);
}

// The call's last step: forest -> labels, behind the last round when it added an edge (*gate: the word its emit raised; had it
// added none, its own flatten left depth 1).  Writes labels alone: the statistics word still speaks of the last round that ran.
__global__ __launch_bounds__(KNN_FOREST_BLOCK) void knn_forest_labels_kernel(int *labels, long long n, const unsigned *__restrict__ gate)
{
    if (*gate == 0u)
        return;
    const long long i = (long long)blockIdx.x * KNN_FOREST_BLOCK + threadIdx.x;
    if (i < n)
        knn_forest_flatten<KnnPickDevice>(labels, i);
}

template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_forest_scan_kernel(const float *__restrict__ R, int k, long long first, int m, long long n,
                                                                  long long rows_per_slice, float max_dist2,
                                                                  const int *__restrict__ labels, const unsigned *__restrict__ done,
                                                                  u64 *__restrict__ cand, const unsigned *__restrict__ gate,
                                                                  const unsigned *__restrict__ also)
{
#pragma clang fp contract(off)
    if ((gate && *gate == 0u) || (also && *also == 0u))
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    const unsigned own = (unsigned)(first + q), owna = (unsigned)(first + qa);
    const bool live = q < m && ((done[owna >> 5] >> (owna & 31u)) & 1u) == 0u;
    if (__ballot(live) == 0ull)   // every row of the wave is done
        return;
    const float *__restrict__ qp = R + (size_t)(first + qa) * k;
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? qp[d] : 0.0f;
    const int mine = labels[owna];
    u64 near = kKeyInit;
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan_one<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned row, bool other) {
        if (other && live && acc < INFINITY && acc <= max_dist2) {   // (NaN fails both compares)
            if (labels[row] != mine) {   // (wave-uniform address; read for the rows within the radius alone)
                const u64 key = pack_key(acc, row);
                near = key < near ? key : near;
            }
        }
    });
    if (near != kKeyInit)
        key_atomic_min(&cand[own], near);
}

// offer 1, and the done bits: a wave's 64 bits are one ballot, stored by lane 0 as the two words they fill (rows at and beyond n
// vote 0).  A row that is done stays done: it was not scanned, so it has no candidate now either.
__global__ __launch_bounds__(KNN_FOREST_BLOCK) void knn_forest_offer1_kernel(const int *__restrict__ labels, long long n,
                                                                            const u64 *__restrict__ cand, u64 *pick1,
                                                                            unsigned *__restrict__ done, const unsigned *__restrict__ gate)
{
    if (gate && *gate == 0u)
        return;
    const long long i = (long long)blockIdx.x * KNN_FOREST_BLOCK + threadIdx.x;
    bool none = false;
    if (i < n) {
        none = cand[i] == kKeyInit;
        knn_forest_offer1<KnnPickDevice>(labels, cand, pick1, i);
    }
    const u64 bits = __ballot(none);
    if ((threadIdx.x & 63) == 0) {
        const long long w = (i >> 6) * 2, words = (n + 31) >> 5;
        if (w < words)
            done[w] = (unsigned)bits;
        if (w + 1 < words)
            done[w + 1] = (unsigned)(bits >> 32);
    }
}

__global__ __launch_bounds__(KNN_FOREST_BLOCK) void knn_forest_offer2_kernel(const int *__restrict__ labels, long long n,
                                                                            const u64 *__restrict__ cand, const u64 *__restrict__ pick1,
                                                                            unsigned *pick2, const unsigned *__restrict__ gate)
{
    if (gate && *gate == 0u)
        return;
    const long long i = (long long)blockIdx.x * KNN_FOREST_BLOCK + threadIdx.x;
    if (i < n)
        knn_forest_offer2<KnnPickDevice>(labels, cand, pick1, pick2, i);
}

__global__ __launch_bounds__(KNN_FOREST_BLOCK) void knn_forest_emit_kernel(const int *__restrict__ labels, long long n,
                                                                          const u64 *__restrict__ pick1, const unsigned *__restrict__ pick2,
                                                                          u64 *__restrict__ edge_keys, unsigned *__restrict__ edge_hi,
                                                                          unsigned *count, unsigned *raised, const unsigned *__restrict__ gate)
{
    if (gate && *gate == 0u)
        return;
    const long long i = (long long)blockIdx.x * KNN_FOREST_BLOCK + threadIdx.x;
    if (i < n)
        (void)knn_forest_emit<KnnPickDevice>(labels, pick1, pick2, i, n, edge_keys, edge_hi, count, raised);
}

__global__ __launch_bounds__(KNN_FOREST_BLOCK) void knn_forest_hook_kernel(int *labels, long long n, const u64 *__restrict__ pick1,
                                                                          const unsigned *__restrict__ pick2,
                                                                          const unsigned *__restrict__ gate)
{
    if (gate && *gate == 0u)
        return;
    const long long i = (long long)blockIdx.x * KNN_FOREST_BLOCK + threadIdx.x;
    if (i < n)
        knn_forest_hook<KnnPickDevice>(labels, pick1, pick2, i);
}

ForestPlan knn_forest_plan(long long n, int num_cu)
{
    ForestPlan p;
    if (n <= 0)
        return p;
    const SlicePlan sp = knn_slice_plan(n, n, num_cu, KnnCountSlices{});   // (the scan's "queries" are the shard's rows)
    p.rounds = knn_forest_rounds(n);
    p.chunks = sp.chunks;
    p.slices = sp.slices;
    p.launches_exact = (long long)p.rounds * (5 + p.chunks) + 1;   // (+ the last flatten)
    p.launches_grid = (long long)p.rounds * (6 + p.chunks) + 1;
    p.cand_off = 0;
    p.pick1_off = (size_t)n * sizeof(u64);
    p.pick2_off = p.pick1_off + (size_t)n * sizeof(u64);
    p.done_off = p.pick2_off + (size_t)n * sizeof(unsigned);
    p.words_off = p.done_off + (size_t)((n + 31) / 32) * sizeof(unsigned);
    p.zero_bytes = (size_t)((n + 31) / 32) * sizeof(unsigned) + (size_t)(2 * p.rounds + 2) * sizeof(unsigned);
    p.scratch_bytes = p.done_off + p.zero_bytes;
    return p;
}

void knn_forest_layout(ForestCall &c, const ForestPlan &p, void *scratch)
{
    unsigned char *b = (unsigned char *)scratch;
    c.rounds = p.rounds;
    c.cand = (u64 *)(b + p.cand_off);
    c.pick1 = (u64 *)(b + p.pick1_off);
    c.pick2 = (unsigned *)(b + p.pick2_off);
    c.done = (unsigned *)(b + p.done_off);
    c.words = (unsigned *)(b + p.words_off);
}

static bool forest_call_ok(const ForestCall &c, int t)
{
    return c.n > 0 && c.n <= 0x7FFFFFFFll && c.k >= 1 && c.r && c.labels && c.edge_keys && c.edge_hi && c.count && c.cand && c.pick1 &&
        c.pick2 && c.done && c.words && c.rounds == knn_forest_rounds(c.n) && t >= 0 && t < c.rounds;
}

static unsigned forest_blocks(const ForestCall &c) { return (unsigned)((c.n + KNN_FOREST_BLOCK - 1) / KNN_FOREST_BLOCK); }

hipError_t knn_forest_begin_launch(const ForestCall &c, const ForestPlan &p)
{
    if (!forest_call_ok(c, 0))
        return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(c.count, 0, 2 * sizeof(unsigned), c.stream);
    return e != hipSuccess ? e : hipMemsetAsync(c.done, 0, p.zero_bytes, c.stream);
}

hipError_t knn_forest_flatten_launch(const ForestCall &c, int t)
{
    if (!forest_call_ok(c, t))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_forest_flatten_kernel, dim3(forest_blocks(c)), dim3(KNN_FOREST_BLOCK), 0, c.stream, c.labels, c.n, t == 0 ? 1 : 0,
                       c.cand, c.pick1, c.pick2, c.gate(t), c.stat());
    return hipGetLastError();
}

hipError_t knn_forest_labels_launch(const ForestCall &c)
{
    if (!forest_call_ok(c, 0))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_forest_labels_kernel, dim3(forest_blocks(c)), dim3(KNN_FOREST_BLOCK), 0, c.stream, c.labels, c.n,
                       (const unsigned *)c.raise(c.rounds - 1));
    return hipGetLastError();
}

hipError_t knn_forest_scan_launch(const ForestCall &c, int t, const unsigned *also)
{
    if (!forest_call_ok(c, t))
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    const unsigned *gate = c.gate(t);
    return knn_slice_chunks(c.n, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0, per = ch.per;
        const dim3 grid = ch.grid, block(KNN_WAVE);
#define KNN_FOREST_SCAN(KCV)                                                                                                       \
    hipLaunchKernelGGL(knn_forest_scan_kernel<KCV>, grid, block, 0, s, c.r, c.k, c0, mc, c.n, per, c.max_dist2, (const int *)c.labels, \
                       (const unsigned *)c.done, c.cand, gate, also)
        KNN_KC_SWITCH(c.k, KNN_FOREST_SCAN)
#undef KNN_FOREST_SCAN
        return hipGetLastError();
    });
}

hipError_t knn_forest_pick_launch(const ForestCall &c, int t)
{
    if (!forest_call_ok(c, t))
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    const dim3 grid(forest_blocks(c)), block(KNN_FOREST_BLOCK);
    const unsigned *gate = c.gate(t);
    hipLaunchKernelGGL(knn_forest_offer1_kernel, grid, block, 0, s, (const int *)c.labels, c.n, (const u64 *)c.cand, c.pick1, c.done, gate);
    hipLaunchKernelGGL(knn_forest_offer2_kernel, grid, block, 0, s, (const int *)c.labels, c.n, (const u64 *)c.cand, (const u64 *)c.pick1,
                       c.pick2, gate);
    hipLaunchKernelGGL(knn_forest_emit_kernel, grid, block, 0, s, (const int *)c.labels, c.n, (const u64 *)c.pick1,
                       (const unsigned *)c.pick2, c.edge_keys, c.edge_hi, c.count, c.raise(t), gate);
    hipLaunchKernelGGL(knn_forest_hook_kernel, grid, block, 0, s, c.labels, c.n, (const u64 *)c.pick1, (const unsigned *)c.pick2, gate);
    return hipGetLastError();
}
