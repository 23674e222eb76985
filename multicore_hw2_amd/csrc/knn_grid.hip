// knn_grid.hip — spatial index for low dimensions (k <= 4): a uniform grid over the shard's bounding
// box, cells in counting-sort order, queried ring by ring with a stop rule that keeps the answer
// bit-identical to the brute-force scan (gfx950 / MI355X).
//
// The reference's counterpart is its KD-tree pair (sources/src/core.cu:960-1050 host build + recursive
// CPU query `v9`, core.cu:1051-1191 one-thread-per-query GPU traversal `v10`; README.md:339-346: it wins
// only at k = 3 and collapses at k = 16).  A tree is the wrong shape for this chip — a recursive descent
// per thread diverges in every wave and its build is a host-side nth_element pass — so the index here is
// flat: no pointers, no recursion, no host work beyond sizing the grid.
//   build  : cell of every row (one pass) -> histogram -> exclusive scan -> scatter rows into cell order
//   query  : ONE WAVE per query.  Ring r = the cells at Chebyshev distance r from the query's cell; the 64
//            lanes split the ring's cells, evaluate their rows with the exact v0 arithmetic (core.cu:44-49)
//            into packed (distance, index) keys, min-reduce across the wave.  After ring r every row not
//            yet seen lies outside the (2r+1)^k block of cells, i.e. at least LB(r) away along some axis;
//            the search stops as soon as  best < LB(r)^2 (1 - 1e-6)  — strictly below what v0 could compute
//            for any unseen row, so neither the minimum nor a tie for it can be outside (lowest index among
//            equal distances is decided by the packed key among the rows seen).
//   top-K  : the same walk with the K smallest keys seen, one per lane, in place of the minimum, and the stop rule on the
//            K-th key (knn_grid_topk_kernel; on request: KNN_QUERY_TOPK_GRID).
// Never used when the rows hold non-finite values or the grid degenerates (a cell with > 4096 rows):
// the brute-force kernels take those shards.
#include "knn_common.h"
#include "knn_cluster_uf.h"
#include "knn_each_radius.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define GRID_BLOCK 256

typedef float f4g __attribute__((ext_vector_type(4)));

struct GridGeom {
    int k;
    int g[4];            // cells per dimension
    unsigned stride[4];  // linear cell id = sum c_d * stride[d]
    float lo[4];         // lower corner of the box
    float inv_w[4];      // cells per unit length (0 when the dimension is degenerate)
    double dlo[4], w[4]; // the same corner / cell width in double, for the stop rule
    double slack[4];     // what a face gives away to the fp32 rounding of the rows' cell assignment (see the stop rule)
};

__device__ __forceinline__ unsigned grid_cell_of(const GridGeom &gg, const float *x, int c_out[4])
{
    unsigned cell = 0u;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int c = 0;
        if (d < gg.k) {
            const float t = (x[d] - gg.lo[d]) * gg.inv_w[d];
            c = t >= 0.0f ? (t < (float)gg.g[d] ? (int)t : gg.g[d] - 1) : 0;   // NaN -> 0 (queries only)
        }
        c_out[d] = c;
        cell += (unsigned)c * gg.stride[d];
    }
    return cell;
}

// ---- build ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRID_BLOCK) void grid_minmax_kernel(const float *__restrict__ R, long long n, int k,
                                                                 unsigned *__restrict__ stats)
{
    // stats[d] = ordered min, stats[4 + d] = ordered max, stats[8] = #non-finite values
    __shared__ unsigned s_lo[4], s_hi[4], s_bad;
    if (threadIdx.x < 4) {
        s_lo[threadIdx.x] = 0xFFFFFFFFu;
        s_hi[threadIdx.x] = 0u;
    }
    if (threadIdx.x == 0)
        s_bad = 0u;
    __syncthreads();
    float lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned bad = 0u;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        for (int d = 0; d < k; ++d) {
            const float v = R[(size_t)i * k + d];
            if (!(fabsf(v) < INFINITY))
                ++bad;
            lo[d] = fminf(lo[d], v);
            hi[d] = fmaxf(hi[d], v);
        }
    auto ord = [](float f) {
        const unsigned u = __float_as_uint(f);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    };
    for (int d = 0; d < k; ++d)
        if (lo[d] <= hi[d]) {
            atomicMin(&s_lo[d], ord(lo[d]));
            atomicMax(&s_hi[d], ord(hi[d]));
        }
    if (bad)
        atomicAdd(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x < (unsigned)k) {
        atomicMin(&stats[threadIdx.x], s_lo[threadIdx.x]);
        atomicMax(&stats[4 + threadIdx.x], s_hi[threadIdx.x]);
    }
    if (threadIdx.x == 0 && s_bad)
        atomicAdd(&stats[8], s_bad);
}

__global__ __launch_bounds__(GRID_BLOCK) void grid_count_kernel(const float *__restrict__ R, long long n, GridGeom gg,
                                                                unsigned *__restrict__ cell_of_row,
                                                                unsigned *__restrict__ counts)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < gg.k; ++d)
        x[d] = R[(size_t)i * gg.k + d];
    int c[4];
    const unsigned cell = grid_cell_of(gg, x, c);
    cell_of_row[i] = cell;
    atomicAdd(&counts[cell], 1u);
}

// Exclusive scan of counts[0..cells) in three steps: per-block scan (2048 entries per block) + block
// totals, scan of the totals by one block, add.  Also the largest single count (degenerate-grid guard).
#define SCAN_PER_BLOCK 2048
__global__ __launch_bounds__(GRID_BLOCK) void grid_scan_blocks_kernel(const unsigned *__restrict__ counts, unsigned cells,
                                                                      unsigned *__restrict__ start,
                                                                      unsigned *__restrict__ totals,
                                                                      unsigned *__restrict__ maxcount)
{
    __shared__ unsigned s_sum[GRID_BLOCK];
    const unsigned base = blockIdx.x * SCAN_PER_BLOCK + threadIdx.x * 8u;
    unsigned v[8], sum = 0u, mx = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = base + j < cells ? counts[base + j] : 0u;
        mx = v[j] > mx ? v[j] : mx;
        sum += v[j];
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (unsigned off = 1; off < GRID_BLOCK; off <<= 1) {   // Hillis-Steele over the 256 thread sums
        const unsigned add = threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned run = s_sum[threadIdx.x] - sum;   // exclusive prefix of this thread inside the block
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (base + j < cells)
            start[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == GRID_BLOCK - 1)
        totals[blockIdx.x] = s_sum[threadIdx.x];
    if (mx)
        atomicMax(maxcount, mx);
}

__global__ __launch_bounds__(GRID_BLOCK) void grid_scan_totals_kernel(unsigned *__restrict__ totals, unsigned nblocks)
{
    // one block: serial over chunks of 256 totals (nblocks <= 8192 for 2^24 cells)
    __shared__ unsigned s_v[GRID_BLOCK];
    __shared__ unsigned s_carry;
    if (threadIdx.x == 0)
        s_carry = 0u;
    __syncthreads();
    for (unsigned c0 = 0; c0 < nblocks; c0 += GRID_BLOCK) {
        const unsigned i = c0 + threadIdx.x;
        const unsigned v = i < nblocks ? totals[i] : 0u;
        s_v[threadIdx.x] = v;
        __syncthreads();
        for (unsigned off = 1; off < GRID_BLOCK; off <<= 1) {
            const unsigned add = threadIdx.x >= off ? s_v[threadIdx.x - off] : 0u;
            __syncthreads();
            s_v[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nblocks)
            totals[i] = s_carry + s_v[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == GRID_BLOCK - 1)
            s_carry += s_v[threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(GRID_BLOCK) void grid_scan_add_kernel(unsigned *__restrict__ start, unsigned cells,
                                                                   const unsigned *__restrict__ totals, unsigned n_rows)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells)
        start[i] += totals[i / SCAN_PER_BLOCK];
    if (i == 0)
        start[cells] = n_rows;
}

__global__ __launch_bounds__(GRID_BLOCK) void grid_scatter_kernel(const float *__restrict__ R, long long n, int k,
                                                                  const unsigned *__restrict__ cell_of_row,
                                                                  const unsigned *__restrict__ start,
                                                                  unsigned *__restrict__ fill,
                                                                  f4g *__restrict__ pts, unsigned *__restrict__ orig)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const unsigned cell = cell_of_row[i];
    const unsigned pos = start[cell] + atomicAdd(&fill[cell], 1u);   // any order inside a cell is fine
    f4g p = {0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < k; ++d)
        p[d] = R[(size_t)i * k + d];
    pts[pos] = p;
    orig[pos] = (unsigned)i;
}

// ---- query ----------------------------------------------------------------------------------------
__device__ __forceinline__ u64 grid_wave_min(u64 v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off, KNN_WAVE);
        v = o < v ? o : v;
    }
    return v;
}

// Position idx of the (2r+1)^K block of cells around the query's cell c: true when it is a cell of the grid that belongs to
// ring r (largest |offset| exactly r; `first`: rings 0 .. r together), *cell_out = its linear id.
template <int K>
__device__ __forceinline__ bool grid_ring_cell(const GridGeom &gg, const int c[4], int r, int side, int idx, bool first,
                                               unsigned *cell_out)
{
    int rem = idx, far = 0;
    bool inside = true;
    unsigned cell = 0u;
#pragma unroll
    for (int d = 0; d < K; ++d) {
        const int off = rem % side - r;
        rem /= side;
        const int cd = c[d] + off;
        far = abs(off) > far ? abs(off) : far;
        inside = inside && cd >= 0 && cd < gg.g[d];
        cell += (unsigned)(inside ? cd : 0) * gg.stride[d];
    }
    *cell_out = cell;
    return inside && !(first ? far > r : far != r);
}

// The stop rule's bound after ring r: rows not yet seen are outside the block of rings 0..r; along the axis where they leave
// it they are at least `lb` from the query (faces beyond the grid bound nothing: no rows out there).
// A row's cell comes from fp32 arithmetic, t = fl(fl(x - lo) * inv_w): a row of a cell below face F
// (an integer) has t < F, hence x < lo + F w (1 + 2^-22) — two roundings and the rounding of inv_w itself —
// and a row of a cell at or above F has x >= lo + F w (1 - 2^-21).  The error grows with the face's distance
// from the corner, at most g w 2^-21: gg.slack[d] = (1e-3 + g 2^-21) w covers it (knn_grid_build keeps
// g <= 2^19 so that this stays a quarter of a cell; the 1e-3 w alone, the round-2 form, was short of it
// from g ~ 4000 up on a single live axis).
// *covers_all: the block is the whole grid (nothing is unseen).
template <int K>
__device__ __forceinline__ double grid_face_bound(const GridGeom &gg, const int c[4], const float q[4], int r, bool *covers_all)
{
    double lb = INFINITY;
    bool all = true;
#pragma unroll
    for (int d = 0; d < K; ++d) {
        if (c[d] - r > 0) {
            all = false;
            const double face = gg.dlo[d] + (double)(c[d] - r) * gg.w[d];
            lb = fmin(lb, (double)q[d] - face - gg.slack[d]);
        }
        if (c[d] + r < gg.g[d] - 1) {
            all = false;
            const double face = gg.dlo[d] + (double)(c[d] + r + 1) * gg.w[d];
            lb = fmin(lb, face - (double)q[d] - gg.slack[d]);
        }
    }
    *covers_all = all;
    return lb;
}

// Query qi's K coordinates into q (the rest 0); false when one of them is not finite: every distance is then NaN or +INF and no
// row can be an answer.
template <int K>
__device__ __forceinline__ bool grid_query_load(const float *__restrict__ Q, int qi, float q[4])
{
    bool finite = true;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        q[d] = d < K ? Q[(size_t)qi * K + d] : 0.f;
        finite = finite && fabsf(q[d]) < INFINITY;
    }
    return finite;
}

// The ring walk of one wave for the finite query q, shared by the 1-NN, radius, link and forest kernels (the top-K kernels'
// lanes share cells and walk under a ballot: knn_grid_topk_body.inc).  Ring r's positions of the (2r+1)^K block go to the lanes 64
// at a time; the first pass takes rings 0 and 1 together (the whole 3^K block): with ~3 rows per cell the own cell alone almost
// never satisfies a stop rule, and every ring is a chain of dependent loads (cell bounds -> rows).  The forms differ in three
// places, their functors:
//   row(acc, p)   for every row position p of a taken cell, acc = its v0 distance (core.cu:44-49: search - reference, squared,
//                 summed in order); every test on acc is the form's own;
//   ring_end()    after the cells of EVERY ring, the one that ends the walk included, before the bound is made: the forms that
//                 keep a wave minimum reduce it here, and what a form keeps per ring is its own to reset here;
//   stop(reach)   the form's stop clause, asked when the block of rings 0..r is not the whole grid and lb > 0: every unseen
//                 row's computed distance is strictly above reach = lb^2 (1 - 1e-6) (grid_face_bound); true ends the walk.
// A query far outside the box, or in an empty region, would walk O(r^K) cells per ring: past rmax rings the walk ends
// unfinished.  Returns whether the wave must raise the give-up word that un-gates the exact scan queued behind the kernel:
// unfinished, and the grid has rings beyond rmax.  Wave-uniform: the query, its cell, r and what stop() says decide it.
template <int K, class Row, class RingEnd, class Stop>
__device__ __forceinline__ bool grid_walk(const GridGeom &gg, const unsigned *__restrict__ start, const f4g *__restrict__ pts,
                                          const float q[4], int lane, int rmax, Row row, RingEnd ring_end, Stop stop)
{
#pragma clang fp contract(off)
    int c[4];
    (void)grid_cell_of(gg, q, c);
    int gmax = 1;
#pragma unroll
    for (int d = 0; d < K; ++d)
        gmax = gg.g[d] > gmax ? gg.g[d] : gmax;
    bool done = false;
    bool first = true;
    for (int r = gmax > 1 ? 1 : 0; r < gmax && r <= rmax; ++r) {
        // the cells of ring r: positions of the (2r+1)^K block whose largest |offset| is exactly r
        const int side = 2 * r + 1;
        int total = 1;
#pragma unroll
        for (int d = 0; d < K; ++d)
            total *= side;
        for (int idx = lane; idx < total; idx += KNN_WAVE) {
            unsigned cell;
            if (!grid_ring_cell<K>(gg, c, r, side, idx, first, &cell))
                continue;
            const unsigned p0 = start[cell], p1 = start[cell + 1];
            for (unsigned p = p0; p < p1; ++p) {
                const f4g x = pts[p];
                float acc = 0.0f;
#pragma unroll
                for (int d = 0; d < K; ++d) {
                    const float diff = q[d] - x[d];   // v0: search - reference, squared, summed in order
                    const float sq = diff * diff;
                    acc = acc + sq;
                }
                row(acc, p);
            }
        }
        first = false;
        ring_end();
        bool covers_all;
        const double lb = grid_face_bound<K>(gg, c, q, r, &covers_all);
        if (covers_all || (lb > 0.0 && stop(lb * lb * (1.0 - 1e-6)))) {
            done = true;
            break;
        }
    }
    return !done && gmax > rmax + 1;
}

template <int K>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_query_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                    const unsigned *__restrict__ start,
                                                                    const f4g *__restrict__ pts,
                                                                    const unsigned *__restrict__ orig, long long base,
                                                                    u64 *__restrict__ keys, int rmax,
                                                                    unsigned *__restrict__ giveup,
                                                                    unsigned *__restrict__ giveup_next)
{
#pragma clang fp contract(off)
    // (the flag word of the NEXT batch on this workspace slot is cleared here: the two words of a slot alternate,
    // calls on a slot are stream-ordered, so no memset launch is needed between batches)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *giveup_next = 0u;
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (GRID_BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (qi >= m)
        return;
    float q[4];
    if (!grid_query_load<K>(Q, qi, q))
        return;   // every distance is NaN or +INF: v0 keeps (+INF, index 0) = the key's initial value
    u64 best = kKeyInit, mine = kKeyInit;   // the wave's minimum so far; the lane's of the ring at hand
    const bool gave_up = grid_walk<K>(
        gg, start, pts, q, lane, rmax,
        [&](float acc, unsigned p) {
            if (acc < INFINITY) {   // NaN / +INF never beat +INF (v0's strict >)
                const u64 key = ((u64)__float_as_uint(acc) << 32) | (u64)(unsigned)(base + orig[p]);
                mine = key < mine ? key : mine;
            }
        },
        [&] {
            mine = grid_wave_min(mine);
            best = mine < best ? mine : best;
            mine = kKeyInit;
        },
        [&](double reach) {   // no unseen row can beat or tie the best
            return (double)__uint_as_float((unsigned)(best >> 32)) < reach;
        });
    if (lane == 0) {
        if (best < kKeyInit)   // a real row's key: folding it in is right whether or not the search finished
            __hip_atomic_fetch_min(&keys[qi], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gave_up)
            *giveup = 1u;      // benign race: every writer stores 1
    }
}

// ---- top-K query (KNN_QUERY_TOPK_GRID) ------------------------------------------------------------
// Lane `src`'s value of a 64-bit register, wave-uniform.
__device__ __forceinline__ u64 grid_readlane64(u64 v, int src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | (u64)lo;
}

// The K smallest keys of a query (KK <= 64 = the wave width), the 1-NN kernel's walk with a list in place of the running
// minimum.  The sorted list lives in registers, one packed key per lane: lane t < KK holds the t-th smallest key seen
// (KNN_KEY_INIT while fewer than t + 1 rows are in), lanes >= KK hold ~0; the K-th key is lane KK - 1's, kept wave-uniform in
// `kth`.  A row is a candidate when its v0 distance is finite and its key is below the K-th; candidates are taken one at a
// time: broadcast, its place = #{list < candidate}, the lanes from that place up take their lower neighbour's key.  (Keys are
// distinct — every row is seen once and carries its own number — so places are never ambiguous.)
// A ring's cells go to the lanes as in the 1-NN kernel, 64 at a time; while a ring has at most 32 positions (the first pass of
// k <= 3) `split` = 2, 4, ... lanes share a cell and take every split-th row of it.  The row loop runs to the wave's longest
// share under a predicate, so every cross-lane step is executed by the whole wave.
// Stop rule, after ring r: the block of rings 0..r is the whole grid, or lane KK - 1 holds a real key whose distance is
// < lb^2 (1 - 1e-6) — every unseen row's computed distance is strictly above that, so none can enter the list or tie its K-th
// place.  The list goes to out[q][0 .. KK) and is never folded here: a batch that gives up is answered again by the exact
// top-K behind this kernel, and a row folded by both would stand in the caller's keys twice.
// WR (knn_index_query_topk_within): the radius form.  A row is a candidate when its key is below min(kth, lim), lim =
// (bits(max_dist2) + 1) << 32: the limit is kept apart from `kth`, which is re-read from lane KK - 1 after every insertion and is
// KNN_KEY_INIT there until the list is full — `kth < kKeyInit` stays the "K-th is a real key" test.  The stop rule gains a
// clause: done when max_dist2 < lb^2 (1 - 1e-6), the same argument with the radius in place of the K-th distance (every unseen
// row's computed distance is strictly above that bound, so none is within the radius).  A query in an empty region or outside
// the rows' box then ends after the few rings its radius spans, with a short or empty list, where the plain form gives up.
// (The body is a file of its own, knn_grid_topk_body.inc, so that the radius form can be a kernel of its own with one argument
// more: the plain form keeps its argument list, its name and its code as they are.)
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_topk_kernel(const float *__restrict__ Q, int m, int KK, GridGeom gg,
                                                                   const unsigned *__restrict__ start,
                                                                   const f4g *__restrict__ pts,
                                                                   const unsigned *__restrict__ orig, long long base,
                                                                   u64 *__restrict__ out, int rmax,
                                                                   unsigned *__restrict__ giveup,
                                                                   unsigned *__restrict__ giveup_next)
{
#pragma clang fp contract(off)
    constexpr bool WR = false;
    constexpr float max_dist2 = 0.0f;
#include "knn_grid_topk_body.inc"
}

// The radius form (knn_index_query_topk_within).
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_within_kernel(const float *__restrict__ Q, int m, int KK, GridGeom gg,
                                                                     const unsigned *__restrict__ start,
                                                                     const f4g *__restrict__ pts,
                                                                     const unsigned *__restrict__ orig, long long base,
                                                                     u64 *__restrict__ out, int rmax,
                                                                     unsigned *__restrict__ giveup,
                                                                     unsigned *__restrict__ giveup_next, float max_dist2)
{
#pragma clang fp contract(off)
    constexpr bool WR = true;
#include "knn_grid_topk_body.inc"
}

// ---- counts and lists within a radius (KNN_QUERY_COUNT_GRID) ---------------------------------------
// Eight entry points of one walk, knn_grid_radius_body.inc (the description is there): each fixes the switches LIST, EACH, SELF and MASKED
// and names, as null or zero constants, the arguments it does not take.  (A body file and not a function template over
// grid_walk: as a function template the same text compiled to 2 to 6 VGPRs more in every kernel of KD 2..4, with the first face
// of grid_face_bound held as a select: profiles/grid_walk_refactor.txt has the figures and what is supposed about the cause.)
#define GRID_RADIUS_NO_LIST /* a count form reserves and stores nothing */   \
    constexpr long long base = 0;                                            \
    constexpr const u64 *offsets = nullptr;                                  \
    constexpr unsigned *cursor = nullptr;                                    \
    constexpr u64 *keys = nullptr
#define GRID_RADIUS_NO_SELF /* no own row to drop */ constexpr unsigned first = 0u
#define GRID_RADIUS_NO_MASK /* every row admitted */ \
    constexpr bool MASKED = false;                   \
    constexpr const unsigned *mask = nullptr

// knn_index_count_within
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_count_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                    const unsigned *__restrict__ start,
                                                                    const f4g *__restrict__ pts, unsigned *__restrict__ out,
                                                                    int rmax, unsigned *__restrict__ giveup,
                                                                    unsigned *__restrict__ giveup_next, float max_dist2)
{
#pragma clang fp contract(off)
    constexpr bool LIST = false, EACH = false, SELF = false;
    constexpr const unsigned *orig = nullptr;
    constexpr const float *radii = nullptr;
    const float cap = max_dist2;
    GRID_RADIUS_NO_LIST;
    GRID_RADIUS_NO_SELF;
    GRID_RADIUS_NO_MASK;
#include "knn_grid_radius_body.inc"
}

// knn_index_list_within
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_list_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                   const unsigned *__restrict__ start,
                                                                   const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                   long long base, const u64 *__restrict__ offsets,
                                                                   unsigned *__restrict__ cursor, u64 *__restrict__ keys, int rmax,
                                                                   unsigned *__restrict__ giveup,
                                                                   unsigned *__restrict__ giveup_next, float max_dist2)
{
#pragma clang fp contract(off)
    constexpr bool LIST = true, EACH = false, SELF = false;
    constexpr unsigned *out = nullptr;
    constexpr const float *radii = nullptr;
    const float cap = max_dist2;
    GRID_RADIUS_NO_SELF;
    GRID_RADIUS_NO_MASK;
#include "knn_grid_radius_body.inc"
}

// a radius per query (include/knn_mi355x.h 2j): knn_index_count_within_each, knn_index_list_within_each
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_each_count_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                         const unsigned *__restrict__ start,
                                                                         const f4g *__restrict__ pts, unsigned *__restrict__ out,
                                                                         int rmax, unsigned *__restrict__ giveup,
                                                                         unsigned *__restrict__ giveup_next,
                                                                         const float *__restrict__ radii, float cap)
{
#pragma clang fp contract(off)
    constexpr bool LIST = false, EACH = true, SELF = false;
    constexpr const unsigned *orig = nullptr;
    GRID_RADIUS_NO_LIST;
    GRID_RADIUS_NO_SELF;
    GRID_RADIUS_NO_MASK;
#include "knn_grid_radius_body.inc"
}

template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_each_list_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                        const unsigned *__restrict__ start,
                                                                        const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                        long long base, const u64 *__restrict__ offsets,
                                                                        unsigned *__restrict__ cursor, u64 *__restrict__ keys, int rmax,
                                                                        unsigned *__restrict__ giveup,
                                                                        unsigned *__restrict__ giveup_next,
                                                                        const float *__restrict__ radii, float cap)
{
#pragma clang fp contract(off)
    constexpr bool LIST = true, EACH = true, SELF = false;
    constexpr unsigned *out = nullptr;
    GRID_RADIUS_NO_SELF;
    GRID_RADIUS_NO_MASK;
#include "knn_grid_radius_body.inc"
}

// the radius graph on the grid (include/knn_mi355x.h 2k): knn_index_self_count_within_routed, knn_index_self_list_within_routed
template <int KD, bool EACH>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_self_count_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                         const unsigned *__restrict__ start,
                                                                         const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                         unsigned first, unsigned *__restrict__ out, int rmax,
                                                                         unsigned *__restrict__ giveup,
                                                                         unsigned *__restrict__ giveup_next,
                                                                         const float *__restrict__ radii, float cap)
{
#pragma clang fp contract(off)
    constexpr bool LIST = false, SELF = true;
    GRID_RADIUS_NO_LIST;
    GRID_RADIUS_NO_MASK;
#include "knn_grid_radius_body.inc"
}

template <int KD, bool EACH>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_self_list_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                        const unsigned *__restrict__ start,
                                                                        const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                        unsigned first, long long base, const u64 *__restrict__ offsets,
                                                                        unsigned *__restrict__ cursor, u64 *__restrict__ keys, int rmax,
                                                                        unsigned *__restrict__ giveup,
                                                                        unsigned *__restrict__ giveup_next,
                                                                        const float *__restrict__ radii, float cap)
{
#pragma clang fp contract(off)
    constexpr bool LIST = true, SELF = true;
    constexpr unsigned *out = nullptr;
    GRID_RADIUS_NO_MASK;
#include "knn_grid_radius_body.inc"
}

// over a subset of the rows on the grid (include/knn_mi355x.h 2l): knn_index_count_within_masked_routed, knn_index_list_within_masked_routed
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_masked_count_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                           const unsigned *__restrict__ start,
                                                                           const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                           const unsigned *__restrict__ mask, unsigned *__restrict__ out,
                                                                           int rmax, unsigned *__restrict__ giveup,
                                                                           unsigned *__restrict__ giveup_next, float max_dist2)
{
#pragma clang fp contract(off)
    constexpr bool LIST = false, EACH = false, SELF = false, MASKED = true;
    constexpr const float *radii = nullptr;
    const float cap = max_dist2;
    GRID_RADIUS_NO_LIST;
    GRID_RADIUS_NO_SELF;
#include "knn_grid_radius_body.inc"
}

template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_masked_list_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                          const unsigned *__restrict__ start,
                                                                          const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                          const unsigned *__restrict__ mask, long long base,
                                                                          const u64 *__restrict__ offsets, unsigned *__restrict__ cursor,
                                                                          u64 *__restrict__ keys, int rmax, unsigned *__restrict__ giveup,
                                                                          unsigned *__restrict__ giveup_next, float max_dist2)
{
#pragma clang fp contract(off)
    constexpr bool LIST = true, EACH = false, SELF = false, MASKED = true;
    constexpr unsigned *out = nullptr;
    constexpr const float *radii = nullptr;
    const float cap = max_dist2;
    GRID_RADIUS_NO_SELF;
#include "knn_grid_radius_body.inc"
}
#undef GRID_RADIUS_NO_LIST
#undef GRID_RADIUS_NO_SELF
#undef GRID_RADIUS_NO_MASK

// ---- the link sweep of knn_index_self_cluster_within on the grid (include/knn_mi355x.h 2m; knn_cluster.hip describes the call) ----
// knn_grid_radius_body.inc's walk with SELF at the scalar radius — one wave per query (local row qi) on grid_walk, the same stop
// clause, ring limit and give-up word.  A hit is a row i = orig[p] != qi with E finite and E <= cap; the
// hit path is knn_cluster_link_kernel's: both rows core and i < qi — the lane unites (knn_cluster_uf.h; every lane has its own
// cached root, a member of row qi's set); row qi not core and i core — the key (E's bits, i) goes into the lane's minimum, the
// wave reduces it with shuffles and lane 0 issues one atomic min on best[qi], only when some lane folded a key.
// A wave that gives up raises the word and leaves what it has united and folded where it is: the gated exact sweep behind this
// kernel does every pair again, and unite and min are idempotent.  A row with a non-finite coordinate has no hit and walks nothing.
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_cluster_link_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                           const unsigned *__restrict__ start,
                                                                           const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                           int *parent, const unsigned *__restrict__ core,
                                                                           u64 *__restrict__ best, int rmax,
                                                                           unsigned *__restrict__ giveup,
                                                                           unsigned *__restrict__ giveup_next, float cap)
{
#pragma clang fp contract(off)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *giveup_next = 0u;   // (the slot's other word, as the 1-NN kernel)
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (GRID_BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (qi >= m)
        return;
    float q[4];
    if (!grid_query_load<KD>(Q, qi, q))   // no row can be a hit (and nothing to give up on)
        return;
    const unsigned own = (unsigned)qi;
    const bool jcore = ((core[own >> 5] >> (own & 31u)) & 1u) != 0u;   // wave-uniform
    int croot = qi;
    u64 near = kKeyInit;
    const bool gave_up = grid_walk<KD>(
        gg, start, pts, q, lane, rmax,
        [&](float acc, unsigned p) {
            if (acc < INFINITY && acc <= cap) {
                const unsigned row = orig[p];
                if (row != own && ((core[row >> 5] >> (row & 31u)) & 1u) != 0u) {
                    if (jcore) {
                        if (row < own && KnnUfDevice::load(&parent[row]) != croot)
                            croot = knn_uf_unite<KnnUfDevice>(parent, (int)row, croot);
                    } else {
                        const u64 key = ((u64)__float_as_uint(acc) << 32) | (u64)row;
                        near = key < near ? key : near;
                    }
                }
            }
        },
        [] {}, [&](double reach) { return (double)cap < reach; });   // no unseen row is within the radius
    if (!jcore)   // (wave-uniform)
        near = grid_wave_min(near);
    if (lane == 0) {
        if (near != kKeyInit)
            __hip_atomic_fetch_min(&best[qi], near, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gave_up)
            *giveup = 1u;      // benign race: every writer stores 1
    }
}

// ---- the scan step of knn_index_self_forest_within on the grid (include/knn_mi355x.h 2o; knn_forest.hip describes the round) ----
// The link kernel's SELF walk — one wave per local row qi on grid_walk — with the Borůvka hit path: a
// row i = orig[p] != qi with E finite, E <= cap and labels[i] != labels[qi] (the labels are frozen: this kernel only reads them)
// folds the key (E's bits, i) into the lane's minimum; the wave reduces it ring by ring and lane 0 stores cand[qi] once, when some
// lane folded a key.  A walk ends by the radius clause OR by the 1-NN kernel's clause on the best key so far — every unseen row
// is farther than the nearest foreign row found —, so a row whose nearest foreign row is close does not walk out to the radius.
// A row that is done (it had no candidate in an earlier round: components only grow) walks nothing.  A wave that passes rmax rings
// raises the round's give-up word (and the call's statistics word) and stores what it has: the gated exact scan of the round
// folds every candidate again with an atomic min, which is idempotent.  gate: the round's word (null: round 0).
template <int KD>
__global__ __launch_bounds__(GRID_BLOCK) void knn_grid_forest_scan_kernel(const float *__restrict__ Q, int m, GridGeom gg,
                                                                          const unsigned *__restrict__ start,
                                                                          const f4g *__restrict__ pts, const unsigned *__restrict__ orig,
                                                                          const int *__restrict__ labels,
                                                                          const unsigned *__restrict__ done_bits, u64 *__restrict__ cand,
                                                                          int rmax, const unsigned *__restrict__ gate,
                                                                          unsigned *__restrict__ giveup, unsigned *__restrict__ stat,
                                                                          float cap)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * (GRID_BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (qi >= m)
        return;
    const unsigned own = (unsigned)qi;
    if (((done_bits[own >> 5] >> (own & 31u)) & 1u) != 0u)   // wave-uniform
        return;
    float q[4];
    if (!grid_query_load<KD>(Q, qi, q))   // no row can be a hit (and nothing to give up on)
        return;
    const int mine = labels[own];
    u64 best = kKeyInit, near = kKeyInit;   // the wave's minimum so far; the lane's of the ring at hand
    const bool gave_up = grid_walk<KD>(
        gg, start, pts, q, lane, rmax,
        [&](float acc, unsigned p) {
            if (acc < INFINITY && acc <= cap) {
                const unsigned row = orig[p];
                if (row != own && labels[row] != mine) {
                    const u64 key = ((u64)__float_as_uint(acc) << 32) | (u64)row;
                    near = key < near ? key : near;
                }
            }
        },
        [&] {
            near = grid_wave_min(near);
            best = near < best ? near : best;
            near = kKeyInit;
        },
        [&](double reach) {   // no unseen row is within the radius, or none can beat or tie the best (+INF while no key is in)
            return (double)cap < reach || (double)__uint_as_float((unsigned)(best >> 32)) < reach;
        });
    if (lane == 0) {
        if (best != kKeyInit)
            cand[qi] = best;
        if (gave_up) {
            *giveup = 1u;      // benign race: every writer stores 1
            *stat = 1u;
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------
#define GTRY(call)                     \
    do {                                 \
        hipError_t e_ = (call);          \
        if (e_ != hipSuccess)            \
            return e_;                   \
    } while (0)

// The kernel form for k dimensions (1 .. 4: knn_grid_build takes no other).  LAUNCH(KD) is a statement (or an if / else chain of
// launches) that names a kernel's <KD> instance.
#define GRID_KD_SWITCH(k, LAUNCH)  \
    switch (k) {                   \
    case 1: LAUNCH(1); break;      \
    case 2: LAUNCH(2); break;      \
    case 3: LAUNCH(3); break;      \
    default: LAUNCH(4); break;     \
    }

struct GridState {
    bool usable = false;
    GridGeom geom;
    unsigned cells = 0;
    unsigned *start = nullptr;   // device [cells + 1]
    f4g *pts = nullptr;          // device [n]: rows in cell order, padded to 4 floats
    unsigned *orig = nullptr;    // device [n]: shard-local row number of pts[i]
    unsigned max_cell = 0;
    unsigned *giveup = nullptr;  // device [KNN_SLOTS][2]: != 0 after a query batch = some query left the grid search
    mutable unsigned calls[KNN_SLOTS] = {};   // batches issued per slot (picks the slot's flag word)
};

void knn_grid_free(GridState *&gs)
{
    if (!gs)
        return;
    (void)knn_dev_free(gs->start);
    (void)knn_dev_free(gs->pts);
    (void)knn_dev_free(gs->orig);
    (void)knn_dev_free(gs->giveup);
    delete gs;
    gs = nullptr;
}

static inline float grid_ord2f(unsigned o)
{
    const unsigned u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// Builds the grid for refs[0..n) (device, AoS, k <= 4).  Synchronous.  *out stays null (hipSuccess) when
// the data rules the index out: non-finite values, a degenerate box, a cell with more than 4096 rows.
hipError_t knn_grid_build(GridState **out, int k, long long n, const float *r, hipStream_t s)
{
    *out = nullptr;
    if (k < 1 || k > 4 || n < 64 || n > 0x7FFFFFFFll)
        return hipSuccess;
    unsigned hstats[9] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u};
    unsigned *dstats = nullptr;
    GTRY(knn_dev_alloc((void **)&dstats, sizeof hstats));
    hipError_t e = hipMemcpyAsync(dstats, hstats, sizeof hstats, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(grid_minmax_kernel, dim3(1024), dim3(GRID_BLOCK), 0, s, r, n, k, dstats);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(hstats, dstats, sizeof hstats, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void)knn_dev_free(dstats);
    GTRY(e);
    if (hstats[8] != 0u)
        return hipSuccess;   // NaN / Inf among the rows
    // ~3 rows per cell on average: g cells per axis over the k axes that have any extent
    GridGeom gg;
    memset(&gg, 0, sizeof gg);
    gg.k = k;
    int live = 0;
    double lo[4], hi[4];
    for (int d = 0; d < k; ++d) {
        lo[d] = grid_ord2f(hstats[d]);
        hi[d] = grid_ord2f(hstats[4 + d]);
        if (!(hi[d] - lo[d] < 1e30))
            return hipSuccess;   // the box itself overflows fp32 arithmetic
        if (hi[d] > lo[d])
            ++live;
    }
    if (live == 0)
        return hipSuccess;       // all rows identical
    int g = (int)floor(pow((double)n / 3.0, 1.0 / live));
    // <= ~4M cells; one live axis: <= 2^19 so that the stop rule's rounding slack (g 2^-21 cells) stays a quarter of a cell
    const int gcap = live == 1 ? (1 << 19) : live == 2 ? 2048 : live == 3 ? 160 : 45;
    g = g < 1 ? 1 : g > gcap ? gcap : g;
    unsigned cells = 1u;
    for (int d = 0; d < 4; ++d) {
        gg.g[d] = 1;
        gg.stride[d] = 0u;
    }
    for (int d = 0; d < k; ++d) {
        gg.g[d] = hi[d] > lo[d] ? g : 1;
        gg.stride[d] = cells;
        cells *= (unsigned)gg.g[d];
        gg.lo[d] = (float)lo[d];
        gg.dlo[d] = lo[d];
        gg.w[d] = hi[d] > lo[d] ? (hi[d] - lo[d]) / gg.g[d] : 1.0;
        gg.slack[d] = (1e-3 + (double)gg.g[d] * 0x1p-21) * gg.w[d];
        gg.inv_w[d] = hi[d] > lo[d] ? (float)((double)gg.g[d] / (hi[d] - lo[d])) : 0.0f;
        if (!(gg.inv_w[d] < INFINITY))
            return hipSuccess;
    }
    GridState *gs = new (std::nothrow) GridState();
    if (!gs)
        return hipErrorOutOfMemory;
    gs->geom = gg;
    gs->cells = cells;
    unsigned *cell_of_row = nullptr, *counts = nullptr, *totals = nullptr, *dmax = nullptr;
    const unsigned nblocks = (cells + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK;
    e = knn_dev_alloc((void **)&gs->start, ((size_t)cells + 1) * sizeof(unsigned));
    if (e == hipSuccess)
        e = knn_dev_alloc((void **)&gs->pts, (size_t)n * sizeof(f4g));
    if (e == hipSuccess)
        e = knn_dev_alloc((void **)&gs->orig, (size_t)n * sizeof(unsigned));
    if (e == hipSuccess)
        e = knn_dev_alloc((void **)&gs->giveup, 2 * KNN_SLOTS * sizeof(unsigned));
    if (e == hipSuccess)
        e = hipMemsetAsync(gs->giveup, 0, 2 * KNN_SLOTS * sizeof(unsigned), s);
    if (e == hipSuccess)
        e = knn_dev_alloc((void **)&cell_of_row, (size_t)n * sizeof(unsigned));
    if (e == hipSuccess)
        e = knn_dev_alloc((void **)&counts, ((size_t)cells + 1) * sizeof(unsigned));
    if (e == hipSuccess)
        e = knn_dev_alloc((void **)&totals, ((size_t)nblocks + 1) * sizeof(unsigned));
    if (e == hipSuccess)
        e = knn_dev_alloc((void **)&dmax, sizeof(unsigned));
    if (e == hipSuccess)
        e = hipMemsetAsync(counts, 0, ((size_t)cells + 1) * sizeof(unsigned), s);
    if (e == hipSuccess)
        e = hipMemsetAsync(dmax, 0, sizeof(unsigned), s);
    unsigned hmax = 0u;
    if (e == hipSuccess) {
        const unsigned rb = (unsigned)((n + GRID_BLOCK - 1) / GRID_BLOCK);
        hipLaunchKernelGGL(grid_count_kernel, dim3(rb), dim3(GRID_BLOCK), 0, s, r, n, gg, cell_of_row, counts);
        hipLaunchKernelGGL(grid_scan_blocks_kernel, dim3(nblocks), dim3(GRID_BLOCK), 0, s, counts, cells, gs->start, totals, dmax);
        hipLaunchKernelGGL(grid_scan_totals_kernel, dim3(1), dim3(GRID_BLOCK), 0, s, totals, nblocks);
        hipLaunchKernelGGL(grid_scan_add_kernel, dim3((cells + GRID_BLOCK - 1) / GRID_BLOCK), dim3(GRID_BLOCK), 0, s, gs->start,
                           cells, totals, (unsigned)n);
        e = hipMemsetAsync(counts, 0, ((size_t)cells + 1) * sizeof(unsigned), s);   // reused as the fill counters
        if (e == hipSuccess) {
            hipLaunchKernelGGL(grid_scatter_kernel, dim3(rb), dim3(GRID_BLOCK), 0, s, r, n, k, cell_of_row, gs->start, counts,
                               gs->pts, gs->orig);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(&hmax, dmax, sizeof hmax, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
    }
    (void)knn_dev_free(cell_of_row);
    (void)knn_dev_free(counts);
    (void)knn_dev_free(totals);
    (void)knn_dev_free(dmax);
    if (e != hipSuccess || hmax > 4096u) {
        knn_grid_free(gs);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            e = hipSuccess;
        }
        return e;
    }
    gs->max_cell = hmax;
    gs->usable = true;
    *out = gs;
    return hipSuccess;
}

// rings a 1-NN query walks before it gives up
static inline int grid_rmax_1nn(int k)
{
    return k == 1 ? 64 : k == 2 ? 16 : k == 3 ? 6 : 4;
}

// Asynchronous on `s`.  *gate_out = the device word the brute-force scan queued behind this must be gated on.
hipError_t knn_grid_query(const GridState *gs, int slot, int m, const float *q, long long base, u64 *keys,
                          const unsigned **gate_out, hipStream_t s)
{
    *gate_out = nullptr;
    if (!gs || !gs->usable || m <= 0)
        return hipSuccess;
    const unsigned call = gs->calls[slot]++;
    unsigned *giveup = gs->giveup + 2 * slot + (call & 1u);
    unsigned *giveup_next = gs->giveup + 2 * slot + ((call + 1u) & 1u);
    const int k = gs->geom.k;
    const int rmax = grid_rmax_1nn(k);
    const dim3 grid((unsigned)((m + GRID_BLOCK / 64 - 1) / (GRID_BLOCK / 64))), block(GRID_BLOCK);
#define GRID_QUERY(KDV)                                                                                                              \
    hipLaunchKernelGGL(knn_grid_query_kernel<KDV>, grid, block, 0, s, q, m, gs->geom, gs->start, gs->pts, gs->orig, base, keys, rmax, \
                       giveup, giveup_next)
    GRID_KD_SWITCH(k, GRID_QUERY)
#undef GRID_QUERY
    *gate_out = giveup;
    return hipGetLastError();
}

// Top-K on the grid (host arithmetic only).  rmax: a K-th neighbour lies deeper than the nearest — the first ring whose block
// holds 4 K rows at the build's 3 rows per cell, doubled (+ 2) for queries at a cell's edge and uneven cells; never below the
// 1-NN kernel's.
// A radius call (radius_rings > 0) walks as far as its radius spans: rmax = max(plain rmax, radius_rings) while a walk of that
// many rings stays within kGridWithinCells cells, (2 rings + 1)^k <= 2^15 — the size of the largest walk the plain plan already
// allows (k 4, K 64: 13^4), a chosen budget, not a measured one.  Beyond it the plain rmax and the give-up rule stand.
GridTopkPlan knn_grid_topk_plan(int k, int K, int m, bool has_grid, int path, bool flag, long long radius_rings)
{
    GridTopkPlan p;
    p.use = has_grid && flag && (path == 0 || path == 3);
    if (!p.use)
        return p;
    int need = 0;
    for (;; ++need) {
        long long block = 3;
        for (int d = 0; d < k; ++d)
            block *= 2 * need + 1;
        if (block >= 4ll * K)
            break;
    }
    p.rmax = std::max(grid_rmax_1nn(k), 2 * need + 2);
    if (radius_rings > p.rmax) {
        constexpr long long kGridWithinCells = 1ll << 15;
        const long long side = 2 * std::min(radius_rings, kGridWithinCells) + 1;
        long long cells = 1;
        for (int d = 0; d < k; ++d)
            cells = std::min(cells * side, kGridWithinCells + 1);
        if (cells <= kGridWithinCells)
            p.rmax = (int)radius_rings;
    }
    p.waves = GRID_BLOCK / 64;
    p.blocks = (unsigned)((m + p.waves - 1) / p.waves);
    p.scratch_bytes = (size_t)m * (size_t)K * sizeof(u64);
    p.launches = 1 + 2 * ((m + KNN_TOPK_CHUNK - 1) / KNN_TOPK_CHUNK) + 1;
    return p;
}

// What the top-K, count and list calls share around their grid kernel: the slot's two give-up words (they alternate from batch to
// batch: the kernel clears the next batch's), one block of GRID_BLOCK threads per GRID_BLOCK / 64 queries unless the plan says
// otherwise (blocks != 0), and the events ev0 / ev1 (nullable) that bracket the kernel.  grid_batch_begin comes right before the
// launch, grid_batch_end right behind it; *gate_out = the batch's give-up word once the kernel is issued.
struct GridBatch {
    unsigned *giveup, *giveup_next;
    dim3 grid, block;
};

static hipError_t grid_batch_begin(const GridState *gs, int slot, int m, unsigned blocks, hipStream_t s, hipEvent_t ev0, GridBatch *b)
{
    const unsigned call = gs->calls[slot]++;
    b->giveup = gs->giveup + 2 * slot + (call & 1u);
    b->giveup_next = gs->giveup + 2 * slot + ((call + 1u) & 1u);
    b->grid = dim3(blocks ? blocks : (unsigned)((m + GRID_BLOCK / 64 - 1) / (GRID_BLOCK / 64)));
    b->block = dim3(GRID_BLOCK);
    return ev0 ? hipEventRecord(ev0, s) : hipSuccess;
}

static hipError_t grid_batch_end(const GridBatch &b, hipStream_t s, hipEvent_t ev1, const unsigned **gate_out)
{
    GTRY(hipGetLastError());
    if (ev1)
        GTRY(hipEventRecord(ev1, s));
    *gate_out = b.giveup;
    return hipSuccess;
}

// The whole top-K call on the grid way, asynchronous on c.stream: the grid kernel writes the batch's lists [m][K] — into c.keys
// itself when the call starts them (init), else into c.cand (>= plan.scratch_bytes) —, the exact top-K behind it, gated on
// the batch's give-up word, overwrites them when some query gave up, and a folding call then merges the scratch into the keys.
// A radius call: the radius kernel and the exact top-K both carry the limit.
// c.ev0 / c.ev1 (nullable) bracket the grid kernel.  *gate_out = the give-up word (knn_index_last_stats reads it back).
hipError_t knn_grid_query_topk(const GridState *gs, const GridTopkPlan &plan, int slot, const TopkCall &c, const unsigned **gate_out)
{
    *gate_out = nullptr;
    if (!gs || !gs->usable || !plan.use || c.m <= 0 || c.K < 1 || c.K > KNN_WAVE || (!c.init && !c.cand))
        return hipErrorInvalidValue;
    u64 *lists = c.init ? c.keys : c.cand;
    hipStream_t s = c.stream;
    GridBatch b;
    GTRY(grid_batch_begin(gs, slot, c.m, plan.blocks, s, c.ev0, &b));
#define GRID_TOPK(KDV)                                                                                                               \
    if (c.within())                                                                                                                  \
        hipLaunchKernelGGL(knn_grid_within_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, c.K, gs->geom, gs->start, gs->pts, gs->orig, \
                           c.base, lists, plan.rmax, b.giveup, b.giveup_next, c.max_dist2);                                          \
    else                                                                                                                             \
        hipLaunchKernelGGL(knn_grid_topk_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, c.K, gs->geom, gs->start, gs->pts, gs->orig,  \
                           c.base, lists, plan.rmax, b.giveup, b.giveup_next)
    GRID_KD_SWITCH(gs->geom.k, GRID_TOPK)
#undef GRID_TOPK
    GTRY(grid_batch_end(b, s, c.ev1, gate_out));
    GTRY(knn_exact_topk_launch(c.writing(lists), b.giveup, true));
    if (!c.init)
        GTRY(knn_topk_merge_launch(c.m, c.K, c.cand, c.keys, s));
    return hipSuccess;
}

// The whole count call on the grid way (KNN_QUERY_COUNT_GRID), asynchronous on c.stream: the grid kernel writes every query's
// count to c.scratch [m]; the commit, gated on NO give-up, adds the scratch to c.counts; the exact count, gated on the give-up
// word, adds the batch's counts itself.  One of the two runs, so no row is counted twice.  rmax: knn_grid_topk_plan's at K = 1 with
// the rings the radius spans.  c.ev0 / c.ev1 (nullable) bracket the grid kernel.  *gate_out = the give-up word.
hipError_t knn_grid_query_count(const GridState *gs, int rmax, int slot, const CountCall &c, const unsigned **gate_out)
{
    *gate_out = nullptr;
    if (!gs || !gs->usable || c.m <= 0 || !c.scratch || !c.counts || rmax < 0 || (c.mask && (c.self_first >= 0 || c.radii)))
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    GridBatch b;
    GTRY(grid_batch_begin(gs, slot, c.m, 0u, s, c.ev0, &b));
#define GRID_COUNT_SELF(KDV, EACHV) /* the shard's own rows (2k); radii null in the scalar form */                                   \
    hipLaunchKernelGGL((knn_grid_self_count_kernel<KDV, EACHV>), b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts,      \
                       gs->orig, (unsigned)c.self_first, c.scratch, rmax, b.giveup, b.giveup_next, c.radii, c.max_dist2)
#define GRID_COUNT(KDV)                                                                                                              \
    if (c.mask)   /* over a subset of the rows (2l), scalar radius */                                                                \
        hipLaunchKernelGGL(knn_grid_masked_count_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts,         \
                           gs->orig, c.mask, c.scratch, rmax, b.giveup, b.giveup_next, c.max_dist2);                                 \
    else if (c.self_first >= 0 && c.radii)                                                                                           \
        GRID_COUNT_SELF(KDV, true);                                                                                                  \
    else if (c.self_first >= 0)                                                                                                      \
        GRID_COUNT_SELF(KDV, false);                                                                                                 \
    else if (c.radii)   /* a radius per query; c.max_dist2 is the cap */                                                             \
        hipLaunchKernelGGL(knn_grid_each_count_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts, c.scratch, \
                           rmax, b.giveup, b.giveup_next, c.radii, c.max_dist2);                                                     \
    else                                                                                                                             \
        hipLaunchKernelGGL(knn_grid_count_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts, c.scratch,     \
                           rmax, b.giveup, b.giveup_next, c.max_dist2)
    GRID_KD_SWITCH(gs->geom.k, GRID_COUNT)
#undef GRID_COUNT
#undef GRID_COUNT_SELF
    GTRY(grid_batch_end(b, s, c.ev1, gate_out));
    GTRY(knn_count_commit_launch(c.m, c.scratch, c.counts, b.giveup, s));
    return knn_gated_count_launch(c, b.giveup);   // (a routed self call: the gated self-scan; a masked one: the gated masked scan)
}

// The whole list call on the grid way (KNN_QUERY_COUNT_GRID), asynchronous on c.stream: c.scratch [m] <- c.fill, the grid kernel
// reserves in c.scratch and stores the keys into the caller's segments behind it; the commit, gated on NO give-up, copies c.scratch
// to c.fill; the exact list, gated on the give-up word, lists the batch itself from the untouched c.fill over the same places.  One
// of the two runs, so no hit is listed twice and a batch that gives up leaves no half-moved cursor.  rmax, events, *gate_out: as
// knn_grid_query_count.
hipError_t knn_grid_query_list(const GridState *gs, int rmax, int slot, const ListCall &c, const unsigned **gate_out)
{
    *gate_out = nullptr;
    if (!gs || !gs->usable || c.m <= 0 || !c.scratch || !c.fill || !c.offsets || !c.keys || c.gids || rmax < 0 ||
        (c.mask && (c.self_first >= 0 || c.radii)))
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    GTRY(hipMemcpyAsync(c.scratch, c.fill, (size_t)c.m * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    GridBatch b;
    GTRY(grid_batch_begin(gs, slot, c.m, 0u, s, c.ev0, &b));
#define GRID_LIST_SELF(KDV, EACHV) /* the shard's own rows (2k); radii null in the scalar form */                                    \
    hipLaunchKernelGGL((knn_grid_self_list_kernel<KDV, EACHV>), b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts,       \
                       gs->orig, (unsigned)c.self_first, c.base, c.offsets, c.scratch, c.keys, rmax, b.giveup, b.giveup_next,        \
                       c.radii, c.max_dist2)
#define GRID_LIST(KDV)                                                                                                               \
    if (c.mask)   /* over a subset of the rows (2l), scalar radius */                                                                \
        hipLaunchKernelGGL(knn_grid_masked_list_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts,          \
                           gs->orig, c.mask, c.base, c.offsets, c.scratch, c.keys, rmax, b.giveup, b.giveup_next, c.max_dist2);      \
    else if (c.self_first >= 0 && c.radii)                                                                                           \
        GRID_LIST_SELF(KDV, true);                                                                                                   \
    else if (c.self_first >= 0)                                                                                                      \
        GRID_LIST_SELF(KDV, false);                                                                                                  \
    else if (c.radii)   /* a radius per query; c.max_dist2 is the cap */                                                             \
        hipLaunchKernelGGL(knn_grid_each_list_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts, gs->orig,  \
                           c.base, c.offsets, c.scratch, c.keys, rmax, b.giveup, b.giveup_next, c.radii, c.max_dist2);               \
    else                                                                                                                             \
        hipLaunchKernelGGL(knn_grid_list_kernel<KDV>, b.grid, b.block, 0, s, c.q, c.m, gs->geom, gs->start, gs->pts, gs->orig,       \
                           c.base, c.offsets, c.scratch, c.keys, rmax, b.giveup, b.giveup_next, c.max_dist2)
    GRID_KD_SWITCH(gs->geom.k, GRID_LIST)
#undef GRID_LIST
#undef GRID_LIST_SELF
    GTRY(grid_batch_end(b, s, c.ev1, gate_out));
    GTRY(knn_list_commit_launch(c.m, c.scratch, c.fill, b.giveup, s));
    return knn_gated_list_launch(c, b.giveup);   // (a routed self call: the gated self-scan; a masked one: the gated masked scan)
}

// The link sweep of a cluster call on the grid way, asynchronous on c.stream: one batch of c.n queries — the shard's rows in local
// order — through knn_grid_cluster_link_kernel.  Nothing is committed behind it: the caller queues knn_cluster_link_launch gated
// on *gate_out, which does every pair again when some row gave up.
hipError_t knn_grid_cluster_link(const GridState *gs, int rmax, int slot, const ClusterCall &c, const unsigned **gate_out)
{
    *gate_out = nullptr;
    if (!gs || !gs->usable || c.n <= 0 || c.n > 0x7FFFFFFFll || c.k != gs->geom.k || !c.r || !c.parent || !c.core || !c.best || rmax < 0)
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    const int m = (int)c.n;
    GridBatch b;
    GTRY(grid_batch_begin(gs, slot, m, 0u, s, nullptr, &b));
#define GRID_CLUSTER_LINK(KDV)                                                                                                       \
    hipLaunchKernelGGL(knn_grid_cluster_link_kernel<KDV>, b.grid, b.block, 0, s, c.r, m, gs->geom, gs->start, gs->pts, gs->orig,     \
                       c.parent, (const unsigned *)c.core, c.best, rmax, b.giveup, b.giveup_next, c.max_dist2)
    GRID_KD_SWITCH(gs->geom.k, GRID_CLUSTER_LINK)
#undef GRID_CLUSTER_LINK
    return grid_batch_end(b, s, nullptr, gate_out);
}

// The scan step of round `round` of a forest call on the grid way, asynchronous on c.stream: one batch of c.n queries — the shard's
// rows in local order — through knn_grid_forest_scan_kernel.  The give-up word is the round's own (ForestCall::giveup), not the
// slot's alternating pair: a round that its gate keeps shut must leave no word behind for the next batch.  The caller queues the
// exact scan of the round gated on that word.
hipError_t knn_grid_forest_scan(const GridState *gs, int rmax, const ForestCall &c, int round)
{
    if (!gs || !gs->usable || c.n <= 0 || c.n > 0x7FFFFFFFll || c.k != gs->geom.k || !c.r || !c.labels || !c.cand || !c.done || !c.words ||
        rmax < 0 || round < 0 || round >= c.rounds)
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    const int m = (int)c.n;
    const dim3 grid((unsigned)((m + GRID_BLOCK / 64 - 1) / (GRID_BLOCK / 64))), block(GRID_BLOCK);
#define GRID_FOREST_SCAN(KDV)                                                                                                        \
    hipLaunchKernelGGL(knn_grid_forest_scan_kernel<KDV>, grid, block, 0, s, c.r, m, gs->geom, gs->start, gs->pts, gs->orig,          \
                       (const int *)c.labels, (const unsigned *)c.done, c.cand, rmax, c.gate(round), c.giveup(round), c.stat(),      \
                       c.max_dist2)
    GRID_KD_SWITCH(gs->geom.k, GRID_FOREST_SCAN)
#undef GRID_FOREST_SCAN
    return hipGetLastError();
}

long long knn_grid_radius_rings(const GridState *gs, float max_dist2)
{
    if (!gs || !gs->usable || !(max_dist2 >= 0.0f))
        return 0;
    double wmin = INFINITY;
    for (int d = 0; d < gs->geom.k; ++d)
        if (gs->geom.g[d] > 1 && gs->geom.w[d] > 0.0)
            wmin = std::min(wmin, (double)gs->geom.w[d]);
    if (!(wmin < INFINITY))
        return 0;
    const double rings = ceil(sqrt((double)max_dist2) / wmin) + 1.0;
    return rings < 0x1p30 ? (long long)rings : 1ll << 30;
}

void knn_grid_info(const GridState *gs, long long info[4])
{
    info[0] = gs ? gs->cells : 0;
    info[1] = gs ? gs->max_cell : 0;
    info[2] = gs ? gs->geom.g[0] : 0;
    info[3] = gs && gs->usable ? 1 : 0;
}
