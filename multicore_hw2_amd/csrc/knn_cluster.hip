// knn_cluster.hip — density clustering of the shard's own rows on the radius graph (include/knn_mi355x.h 2m; DESIGN §4.6
// "Clusters of the radius graph"): knn_index_self_cluster_within behind its degree step.  (The grid way's link kernel lives
// in knn_grid.hip, on grid_walk, the ring walk of that file's kernels; the union-find itself in knn_cluster_uf.h.)
//
// The call is three steps on one stream, no host round trip between them, all in the caller's labels array:
//   1. degrees    the routed self count (2k) over the whole shard writes deg(i) into labels[i]; knn_cluster_core_kernel turns that
//                 in place into the forest's start — parent[i] = i for a core row (deg + 1 >= min_pts), -1 for every other —,
//                 writes the core bits as a 2g mask and sets best[i] to KNN_KEY_INIT;
//   2. link sweep the self scan once more with a hit path in the counter's place (below);
//   3. flatten    knn_cluster_flatten_kernel: labels[i] = find(i) for a core row, find(row of best[i]) for a border row, -1 else.
//
// The link sweep, for the query that is local row j and a hit row i (i != j, E finite, E <= max_dist2):
//   both core and i < j      unite(parent, i, j) — E(i, j) == E(j, i) bit for bit, so the pair is a hit for lane j and for lane i
//                            alike, and the lane of the larger row alone unites;
//   j not core, i core       pack_key(E, i) is folded into the lane's running minimum, and ONE atomic min on best[j] at the end
//                            of the lane's rows, only when something was folded: the nearest core row, the lower row on a tie.
// A lane keeps `croot`, a member of its row's set that was its root when last seen, and skips the find chains when parent[i]
// already is croot: then i hangs directly under a member of j's set and the pair is done.  Inside a dense cluster almost every
// pair ends there.  The skip is only ever a shortcut: a stale or superseded croot makes it miss, never lie.
// knn_cluster_link_kernel<KC> is knn_self_count_kernel<KC>'s skeleton (knn_self_scan.h: self_scan_one — one copy of the loop,
// the hit path is long): one wave per block, lanes = queries, row i wave-uniform, so its core word comes from a scalar load.
//
// Give-up needs no commit step.  unite and the atomic min are idempotent and commute: a grid batch in which some row gave up is
// swept AGAIN, whole, by knn_cluster_link_gated_kernel<KC> over whatever forest and keys the grid walk left, and the result is the
// one the exact sweep alone gives — the components of the same pairs, the minima of the same keys.  (The degree step keeps the
// routed count's own commit: counts do not add idempotently.)
//
// Flatten runs in place over the array it reads, with the read-only walk knn_uf_root: the only writes are labels.  labels[i] =
// root(i) is, for a core row, one more "replace a parent by an ancestor" — every walk that passes through i afterwards still ends
// at the same root — and nothing halves a path here, so no walk can put an older ancestor back over a label.  A border or noise
// row's slot (-1) is read by its own thread alone, before it writes it.
#include "knn_self_scan.h"
#include "knn_cluster_uf.h"
#include "knn_slice_launch.h"

#define KNN_CLUSTER_BLOCK 256

// deg -> forest start, core mask, best.  One thread per row; a wave's 64 core bits are one ballot, stored by lane 0 as the two
// words they fill (rows at and beyond n vote 0: the last word's spare bits are written 0).
__global__ __launch_bounds__(KNN_CLUSTER_BLOCK) void knn_cluster_core_kernel(int *__restrict__ parent, long long n, int min_pts,
                                                                            unsigned *__restrict__ core, u64 *__restrict__ best)
{
    const long long i = (long long)blockIdx.x * KNN_CLUSTER_BLOCK + threadIdx.x;
    bool is_core = false;
    if (i < n) {
        const unsigned deg = (unsigned)parent[i];
        is_core = deg >= (unsigned)(min_pts - 1);   // deg + 1 >= min_pts, min_pts >= 1, without the overflow
        parent[i] = is_core ? (int)i : -1;
        best[i] = kKeyInit;
    }
    const u64 bits = __ballot(is_core);
    if ((threadIdx.x & 63) == 0) {
        const long long w = (i >> 6) * 2, words = (n + 31) >> 5;
        if (w < words)
            core[w] = (unsigned)bits;
        if (w + 1 < words)
            core[w + 1] = (unsigned)(bits >> 32);
    }
}

template <int KC>
__device__ __forceinline__ void cluster_link_body(const float *__restrict__ R, int k, long long first, int m, long long n,
                                                  long long rows_per_slice, float max_dist2, int *parent,
                                                  const unsigned *__restrict__ core, u64 *__restrict__ best)
{
#pragma clang fp contract(off)
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    const float *__restrict__ qp = R + (size_t)(first + qa) * k;
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? qp[d] : 0.0f;
    const bool live = q < m;
    const unsigned own = (unsigned)(first + q), owna = (unsigned)(first + qa);
    const bool jcore = ((core[owna >> 5] >> (owna & 31u)) & 1u) != 0u;
    int croot = (int)owna;    // a member of the lane's set: its row itself to begin with
    u64 near = kKeyInit;
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan_one<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned row, bool other) {
        if (other && live && acc < INFINITY && acc <= max_dist2) {   // (NaN fails both compares)
            if (((core[row >> 5] >> (row & 31u)) & 1u) != 0u) {      // (wave-uniform address)
                if (jcore) {
                    if (row < own && KnnUfDevice::load(&parent[row]) != croot)
                        croot = knn_uf_unite<KnnUfDevice>(parent, (int)row, croot);
                } else {
                    const u64 key = pack_key(acc, row);
                    near = key < near ? key : near;
                }
            }
        }
    });
    if (near != kKeyInit)
        key_atomic_min(&best[own], near);
}

template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_cluster_link_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                   long long n, long long rows_per_slice, float max_dist2,
                                                                   int *parent, const unsigned *__restrict__ core,
                                                                   u64 *__restrict__ best)
{
    cluster_link_body<KC>(R, k, first, m, n, rows_per_slice, max_dist2, parent, core, best);
}

// The gated twin: the exact sweep behind the grid way's, run only when *gate != 0 (some row's walk gave up).
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_cluster_link_gated_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                         long long n, long long rows_per_slice, float max_dist2,
                                                                         int *parent, const unsigned *__restrict__ core,
                                                                         u64 *__restrict__ best, const unsigned *__restrict__ gate)
{
    if (*gate == 0u)
        return;
    cluster_link_body<KC>(R, k, first, m, n, rows_per_slice, max_dist2, parent, core, best);
}

// forest -> labels, in place.  parent[i] >= 0: a core row; else a key in best[i]: a border row, whose label is its nearest core
// row's (a key's row is core: its slot never holds -1).
__global__ __launch_bounds__(KNN_CLUSTER_BLOCK) void knn_cluster_flatten_kernel(int *parent, long long n, const u64 *__restrict__ best)
{
    const long long i = (long long)blockIdx.x * KNN_CLUSTER_BLOCK + threadIdx.x;
    if (i >= n)
        return;
    const int p = KnnUfDevice::load(&parent[i]);
    if (p >= 0) {
        if (p != (int)i)   // (a root's label is there already)
            KnnUfDevice::store(&parent[i], knn_uf_root<KnnUfDevice>(parent, p));
        return;
    }
    const u64 key = best[i];
    if (key != kKeyInit)
        KnnUfDevice::store(&parent[i], knn_uf_root<KnnUfDevice>(parent, (int)(unsigned)key));
}

ClusterPlan knn_cluster_plan(long long n, int num_cu, bool own_mask)
{
    ClusterPlan p;
    if (n <= 0)
        return p;
    const SlicePlan sp = knn_slice_plan(n, n, num_cu, KnnCountSlices{});   // (the sweep's "queries" are the shard's rows)
    p.chunks = sp.chunks;
    p.slices = sp.slices;
    // exact: the counts' memset is no kernel; per chunk the self count and the link sweep; core and flatten
    p.launches_exact = 2ll * p.chunks + 2;
    // grid: grid count, its commit, the gated self count per chunk; core; grid link, the gated link sweep per chunk; flatten
    p.launches_grid = 2ll * p.chunks + 5;
    p.scratch_bytes = (size_t)n * sizeof(u64) + (own_mask ? (size_t)((n + 31) / 32) * sizeof(unsigned) : 0);
    p.count_bytes = (size_t)n * sizeof(unsigned);
    return p;
}

static bool cluster_call_ok(const ClusterCall &c)
{
    return c.n > 0 && c.n <= 0x7FFFFFFFll && c.k >= 1 && c.r && c.parent && c.core && c.best && c.min_pts >= 1;
}

hipError_t knn_cluster_core_launch(const ClusterCall &c)
{
    if (!cluster_call_ok(c))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((c.n + KNN_CLUSTER_BLOCK - 1) / KNN_CLUSTER_BLOCK);
    hipLaunchKernelGGL(knn_cluster_core_kernel, dim3(blocks), dim3(KNN_CLUSTER_BLOCK), 0, c.stream, c.parent, c.n, c.min_pts, c.core,
                       c.best);
    return hipGetLastError();
}

hipError_t knn_cluster_link_launch(const ClusterCall &c, const unsigned *gate)
{
    if (!cluster_call_ok(c))
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    return knn_slice_chunks(c.n, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0, per = ch.per;
        const dim3 grid = ch.grid, block(KNN_WAVE);
#define KNN_CLUSTER_LINK(KCV)                                                                                                        \
    if (gate)                                                                                                                        \
        hipLaunchKernelGGL(knn_cluster_link_gated_kernel<KCV>, grid, block, 0, s, c.r, c.k, c0, mc, c.n, per, c.max_dist2, c.parent, \
                           (const unsigned *)c.core, c.best, gate);                                                                  \
    else                                                                                                                             \
        hipLaunchKernelGGL(knn_cluster_link_kernel<KCV>, grid, block, 0, s, c.r, c.k, c0, mc, c.n, per, c.max_dist2, c.parent,       \
                           (const unsigned *)c.core, c.best)
        KNN_KC_SWITCH(c.k, KNN_CLUSTER_LINK)
#undef KNN_CLUSTER_LINK
        return hipGetLastError();
    });
}

// The gated twin for a pass of the cell-pruned way (knn_cluster_routed.hip): the same kernel over the window's chunks.
hipError_t knn_cluster_link_window_launch(const ClusterCall &c, long long first, int m, const unsigned *gate)
{
    if (!cluster_call_ok(c) || !gate || first < 0 || m < 1 || first + m > c.n)
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    return knn_slice_chunks(m, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = first + ch.c0, per = ch.per;
        const dim3 grid = ch.grid, block(KNN_WAVE);
#define KNN_CLUSTER_LINK(KCV)                                                                                                    \
    hipLaunchKernelGGL(knn_cluster_link_gated_kernel<KCV>, grid, block, 0, s, c.r, c.k, c0, mc, c.n, per, c.max_dist2, c.parent, \
                       (const unsigned *)c.core, c.best, gate)
        KNN_KC_SWITCH(c.k, KNN_CLUSTER_LINK)
#undef KNN_CLUSTER_LINK
        return hipGetLastError();
    });
}

hipError_t knn_cluster_flatten_launch(const ClusterCall &c)
{
    if (!cluster_call_ok(c))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((c.n + KNN_CLUSTER_BLOCK - 1) / KNN_CLUSTER_BLOCK);
    hipLaunchKernelGGL(knn_cluster_flatten_kernel, dim3(blocks), dim3(KNN_CLUSTER_BLOCK), 0, c.stream, c.parent, c.n,
                       (const u64 *)c.best);
    return hipGetLastError();
}
