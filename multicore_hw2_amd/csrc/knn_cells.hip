// knn_cells.hip — the cell-pruned form of the MFMA filter (k <= 16, resident shards; gfx950 / MI355X).
// knn_filter.hip holds the filter it prunes: the fp16 layouts, the error bound, the full scan, the query
// entry point that picks between the two.  Here: the cell index (build), and per batch the kernels that
// score a query only against the cells it cannot rule out.
#include "knn_filter_dev.h"
#include "knn_exact_dev.h"
#include "knn_seed_kth.h"
#include "knn_frame_dup.h"
#include "knn_each_radius.h"

#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <set>
#include <type_traits>
#include <vector>

// ------------------------------------------------------------------------------------------
// Cell-pruned scan (k <= 16, resident index).  Scoring every (query, reference) pair costs ~50 issue
// cycles per 32x32 tile pair whatever the schedule, so the only way under it is not to
// score most pairs.  The index sorts the rows into 2^B cells — every dimension cut into 2^nb[d] bins at
// sample quantiles, cell = the tuple of bin numbers — and lays the fp16 fragments out cell by cell (each
// cell padded to whole 32-row tiles, `perm` maps a layout position back to its row).  Per batch (the default chain):
//   prep    : one block of 2 or 4 waves per query (knn_cells_prep_kernel).  Rounds the query to its fp16 B operand, scores
//             the query's own cell and the 3 cells across its two nearest cuts with the MFMA (a cell of many tiles is
//             sampled) — the minimum is a score of a real reference, which is all knn_threshold needs — derives thr_q for
//             the scores and Dup_q = the largest real (scaled) squared distance any candidate for the answer can have,
//             and tabulates the separable halves of the cell lower bound: a row of cell c differs from the query by at
//             least gap_d(bin_d(c)) in every dimension, so LB(c, q) = sum_d gap_d^2 <= |q - r|^2 for every row of the
//             cell = lo_q[low bits of c] + hi_q[high bits], both rounded DOWN.  LB > Dup_q rules the whole cell out, ties
//             included (a row that ties with the answer obeys the Dup bound too).  The kernel also starts the batch's
//             keys at (+INF, 0) when asked to and clears the control words of the NEXT batch.
//   match   : cell-major (knn_cells_match_kernel): which queries cannot rule a cell out — queries on the lanes against the
//             high table, survivors against 64-byte runs of the low table — written as per-cell lists (a list longer than
//             its room marks the cell `dense`: scored against every query of the batch, which is what a list that long asks
//             for anyway).
//   scan    : knn_cells_scan_kernel.  The unit of work is an ITEM: a run of at most 18 tiles of one cell (fat cells of
//             clustered data are several items, empty cells none).  A wave loads the item's tiles once, gathers the listed
//             queries' B operands from LDS 32 at a time and runs MFMA + min3 tree + threshold test per tile; hits become
//             records (query, tile, half) in the wave's slice, overflow in a small area all waves share.
//   re-rank : knn_rerank_kernel (knn_exact.hip): v0's arithmetic on the records' 16 rows each, through `perm`.
//   gated, on the device: more candidates than the record buffers hold (rows of a cluster tighter than the fp16 step:
//             every row of a query's cells passes) -> knn_cells_exact_kernel evaluates the batch's listed (item, query) pairs
//             with the exact arithmetic — the geometry's verdict stands, it never depended on fp16; a query nothing bounds
//             (not finite, far away, no real row seen) -> the exact scan of the whole shard.  Nothing switches the cells off
//             for later batches.
// (The round-2 chain, the scan with its norm tile out of an extra MFMA and the fused match + scan + re-rank kernel of round 3
// all lost their A/B against this chain and live on as records under tools/arms/ and profiles/r03_sweep_experiments.txt.)
// Uniform data in 16 dimensions, n = 2^24: ~1600 of 65536 cells survive per query, 25 queries per cell.
// ------------------------------------------------------------------------------------------
#define CELL_MAX_BINS 16
#define CELL_TILES_PER_PASS 9                 // reference tiles a wave holds in registers at a time (one more costs the sixth wave per SIMD)

struct CellGeom {
    int k, bits, sa;                 // dimensions, total bits, bits of the low table
    unsigned char nb[16], shift[16]; // bits of dimension d (0 = not cut), position of its bin number in the cell code
    // cell-range shards: `bits` / `nb` / `shift` describe the GLOBAL grid; this index holds codes [cell_base, cell_base + ncells)
    // of it under local numbers (cell_base is a multiple of 2^sa), nh = its entries of the high table.  Else 0, 2^bits, 2^(bits - sa).
    unsigned cell_base, ncells, nh;
};

static CellGeom cell_geom_of(const CellIndex &c, int k)
{
    CellGeom g;
    memset(&g, 0, sizeof g);
    g.k = k;
    g.bits = c.bits;
    g.sa = c.sa;
    memcpy(g.nb, c.nb, 16);
    memcpy(g.shift, c.shift, 16);
    g.cell_base = c.cell_base;
    g.ncells = c.ncells;
    g.nh = (c.ncells + (1u << c.sa) - 1u) >> c.sa;
    return g;
}

// Shape of a grid of 2^bits cells over k dimensions: bits per dimension (the first bits % k dimensions get one more), the
// position of each dimension's bin number in the cell code, and sa = the number of low code bits that are whole dimensions
// and at most 8 (the low pruning table has 2^sa entries).
static void cell_grid_shape(int k, int bits, unsigned char nb[16], unsigned char shift[16], int *sa_out)
{
    int pos = 0, sa = 0;
    for (int d = 0; d < 16; ++d) {
        nb[d] = 0;
        shift[d] = 0;
    }
    for (int d = 0; d < k; ++d) {
        nb[d] = (unsigned char)(bits / k + (d < bits % k ? 1 : 0));
        shift[d] = (unsigned char)pos;
        if (pos <= 8)
            sa = pos;
        pos += nb[d];
    }
    if (pos <= 8)
        sa = pos;
    *sa_out = sa;
}

// Cuts at the sample quantiles: bounds[d][j - 1] = the j-th of 2^nb[d] quantiles of dimension d (+INF beyond).
static void cell_quantile_cuts(int k, const unsigned char nb[16], const float *samp, long long samples, float *bounds)
{
    std::vector<float> col((size_t)samples);
    for (int i = 0; i < 16 * (CELL_MAX_BINS - 1); ++i)
        bounds[i] = INFINITY;
    for (int d = 0; d < std::min(k, 16); ++d) {   // (16 < k <= 32: the cells cut the first 16 dimensions only)
        if (!nb[d])
            continue;
        for (long long i = 0; i < samples; ++i)
            col[(size_t)i] = samp[(size_t)i * k + d];
        const int nbins = 1 << nb[d];
        if (nbins == 2)   // one cut: the median, without sorting the column
            std::nth_element(col.begin(), col.begin() + samples / 2, col.end());
        else
            std::sort(col.begin(), col.end());
        for (int j = 1; j < nbins; ++j)
            bounds[(size_t)d * (CELL_MAX_BINS - 1) + (j - 1)] = col[(size_t)(j * samples / nbins)];
    }
}

static int cell_bits_for_rows(long long n)
{
    int bits = 0;
    long long rows_min = 144;            // cells of 144 .. 288 rows on average: 5-9 tiles each
    if (const char *e = getenv("KNN_MI355X_CELL_ROWS"))   // experiment: other cell sizes
        rows_min = std::max(32, atoi(e));
    while ((rows_min << (bits + 1)) <= n)
        ++bits;
    return bits;
}

__device__ __forceinline__ unsigned cell_bin(const float *__restrict__ bnd, int nbins, float x)
{
    unsigned b = 0u;
    for (int j = 0; j < nbins - 1; ++j)   // ascending cuts: bin b <=> bnd[b-1] <= x < bnd[b]; NaN -> bin 0
        b += x >= bnd[j] ? 1u : 0u;
    return b;
}

// ---- the norm as two fp16 halves ------------------------------------------------------------------
// word = fp16(N) | fp16((N - fp16(N)) * 2^11) << 16.  N - fp16(N) is exact in fp32 (both are fp32 values of about
// the same exponent), the scaled remainder keeps 11 more bits: hi + mid 2^-11 = N to within 2^-22 N, or 2^-25
// absolute where the scaled remainder falls into fp16's subnormal range (< 2^-14) and the matrix core flushes it.
// knn_bound_consts carries both in rho.  +INF (padding, rows outside the box) -> (+INF, 0).
typedef unsigned u4v __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_norm22(float n)
{
    if (!(n < INFINITY))
        return 0x00007C00u;
    const _Float16 hi = (_Float16)n;
    const float rem = n - (float)hi;
    const _Float16 mid = (_Float16)(rem * 2048.0f);
    return (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, mid) << 16);
}

// A operand whose rows carry (hi, mid) in K-slots 0 and 1 (nw: the row's word on lanes 0..31, ZERO on lanes 32..63,
// which hold K-slots 8..15), and the B operand that sums them: every column = {1, 2^-11, 0, ...}.
__device__ __forceinline__ h8 norm_a_operand(unsigned nw)
{
    const u4v t = {nw, 0u, 0u, 0u};
    return __builtin_bit_cast(h8, t);
}
__device__ __forceinline__ h8 norm_b_operand()
{
    const u4v t = {0x10003C00u, 0u, 0u, 0u};   // fp16 1.0 = 0x3C00, fp16 2^-11 = 0x1000
    return __builtin_bit_cast(h8, t);
}
__device__ __forceinline__ f16v zero_acc()
{
    return (f16v){0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
}

// Before a block counts itself done on a counter another block's finaliser watches: every vector-memory operation of this
// wave — the no-return global atomics on keys[] and ctl[] among them — has been performed.  `s_waitcnt vmcnt(0)` only
// (0x0F70: expcnt and lgkmcnt left alone): gfx9 counts stores and no-return atomics in vmcnt and releases the count when the
// memory side has acknowledged them; an agent-scope release fence would add `buffer_wbl2 sc1`, a write-back of the XCD's
// whole L2 per wave (110 -> 261 us at C3, round 4), which atomics performed at the memory side do not need.
__device__ __forceinline__ void cells_wait_own_atomics()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0x0F70);
}

// LDS written by some lanes of a wave, read by others of the SAME wave: order the two without a block barrier.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the LOCAL number of a cell code; a row outside the index's range of the grid (cell-range shards: the caller's partition
// was not this geometry's) is counted and parked in cell 0 — the build then fails
__device__ __forceinline__ unsigned cell_local(unsigned code, const CellGeom &g, unsigned *__restrict__ bad)
{
    const unsigned l = code - g.cell_base;
    if (code < g.cell_base || l >= g.ncells) {
        atomicAdd(bad, 1u);
        return 0u;
    }
    return l;
}

__global__ __launch_bounds__(256) void knn_cells_code_kernel(const float *__restrict__ R, long long n, CellGeom g,
                                                             const float *__restrict__ bounds,
                                                             unsigned *__restrict__ code, unsigned *__restrict__ counts,
                                                             unsigned *__restrict__ bad)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float *__restrict__ x = R + (size_t)i * g.k;
    unsigned c = 0u;
    for (int d = 0; d < min(g.k, 16); ++d)
        if (g.nb[d])
            c |= cell_bin(bounds + d * (CELL_MAX_BINS - 1), 1 << g.nb[d], x[d]) << g.shift[d];
    c = cell_local(c, g, bad);
    code[i] = c;
    atomicAdd(&counts[c], 1u);
}

// The one-pass placement for 16 < k <= 32 (two K-steps per tile: fragments [tile][2][64 lanes][8], round 5): what
// knn_cells_scatter_frag_kernel does for k <= 16, with the row's 32 (padded) dimensions as four 8-wide halves.
__global__ __launch_bounds__(256) void knn_cells_scatter_frag2_kernel(
    const float *__restrict__ R, long long n, int k, const unsigned *__restrict__ code,
    const unsigned *__restrict__ tile_start, unsigned *__restrict__ fill, const float *__restrict__ center, float sigma,
    h8 *__restrict__ frag, float *__restrict__ norms, unsigned *__restrict__ norms2, unsigned *__restrict__ perm,
    unsigned *__restrict__ out, unsigned *__restrict__ olist, unsigned ocap)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float vmax = 0.0f, nrm = 0.0f;
    if (i < n) {
        const float *__restrict__ x = R + (size_t)i * k;
        bool real = true;
        h8 v[4];
#pragma unroll
        for (int part = 0; part < 4; ++part)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = part * 8 + j;
                const float sc = d < k ? (x[d] - center[d]) * sigma : 0.0f;  // fp32 subtract, exact power-of-two scale
                const _Float16 hval = (_Float16)sc;                          // round to nearest even
                const float back = (float)hval;
                real = real && fabsf(back) <= 1.0f;                          // outside the robust box, NaN included
                vmax = fmaxf(vmax, fabsf(back));
                nrm = nrm + back * back;                                     // exact products, fp32 sum in dimension order
                v[part][j] = hval;
            }
        if (!real) {   // out of the filter (zero fragment, +INF norm), into the exact list
            const unsigned opos = atomicAdd(&out[3], 1u);
            if (opos < ocap)
                olist[opos] = (unsigned)i;
#pragma unroll
            for (int part = 0; part < 4; ++part)
                v[part] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
            vmax = 0.0f;
            nrm = 0.0f;
        }
        // the norm's two fp16 halves in the free K-slots 30, 31 (see cell_tile_step_nif).  A row that is out scores the finite 65504:
        // above the threshold of any query near the box, but NOT of one near kAmaxLimit (N + 2|q.r| alone reaches ~61 000 at
        // k = 30).  Such a position then becomes a record: the 1-NN re-rank evaluates the row exactly (it is in the exact list as
        // well; the same key folds twice), the top-K re-rank skips it (the outlier kernel has it), and a batch whose slices flood
        // with them ends in the exact evaluation of its listed pairs — tests/test_filter_margin_gpu.py walks queries up to there.
        if (k <= KNN_NIF_MAX_K) {
            const unsigned nw = real ? pack_norm22(nrm) : 0x00007BFFu;   // (65504, 0)
            v[3][6] = __builtin_bit_cast(_Float16, (unsigned short)(nw & 0xFFFFu));
            v[3][7] = __builtin_bit_cast(_Float16, (unsigned short)(nw >> 16));
        }
        const unsigned c = code[i];
        const size_t pos = (size_t)tile_start[c] * 32 + atomicAdd(&fill[c], 1u);
        h8 *__restrict__ tile = frag + (pos >> 5) * 128;   // two K-steps of 64 lanes
#pragma unroll
        for (int part = 0; part < 4; ++part)
            tile[(part >> 1) * 64 + (part & 1) * 32 + (pos & 31)] = v[part];
        norms[pos] = real ? nrm : INFINITY;
        norms2[pos] = pack_norm22(real ? nrm : INFINITY);
        perm[pos] = (unsigned)i;
    }
    vmax = wave_max_f(vmax);
    nrm = wave_max_f(nrm);
    __shared__ float s_v[4], s_n[4];
    if ((threadIdx.x & 63) == 0) {
        s_v[threadIdx.x >> 6] = vmax;
        s_n[threadIdx.x >> 6] = nrm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        guarded_atomic_max(&out[0], __float_as_uint(fmaxf(fmaxf(s_v[0], s_v[1]), fmaxf(s_v[2], s_v[3]))));
        guarded_atomic_max(&out[1], __float_as_uint(fmaxf(fmaxf(s_n[0], s_n[1]), fmaxf(s_n[2], s_n[3]))));
    }
}

// Scatter + layout in one pass (k <= 16): row i, read in row order, goes to the next free position of its
// cell as an fp16 fragment + norm — what knn_frag_kernel would write there (same arithmetic, same outlier
// rule), without a second pass that gathers 64-byte rows in cell order (8.8 ms for 2^24 rows, against 1.1).
// (the padding positions of every cell are written afterwards by knn_cells_pad_kernel); out[] as in
// knn_frag_kernel.
__global__ __launch_bounds__(256) void knn_cells_scatter_frag_kernel(
    const float *__restrict__ R, long long n, int k, const unsigned *__restrict__ code,
    const unsigned *__restrict__ tile_start, unsigned *__restrict__ fill, const float *__restrict__ center, float sigma,
    h8 *__restrict__ frag, float *__restrict__ norms, unsigned *__restrict__ norms2, unsigned *__restrict__ perm,
    unsigned *__restrict__ out, unsigned *__restrict__ olist, unsigned ocap)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float vmax = 0.0f, nrm = 0.0f;
    if (i < n) {
        const float *__restrict__ x = R + (size_t)i * k;
        bool real = true;
        h8 v[2];
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = half * 8 + j;
                const float sc = d < k ? (x[d] - center[d]) * sigma : 0.0f;  // fp32 subtract, exact power-of-two scale
                const _Float16 hval = (_Float16)sc;                          // round to nearest even
                const float back = (float)hval;
                real = real && fabsf(back) <= 1.0f;                          // outside the robust box, NaN included
                vmax = fmaxf(vmax, fabsf(back));
                nrm = nrm + back * back;                                     // exact products, fp32 sum
                v[half][j] = hval;
            }
        if (!real) {   // out of the filter (zero fragment, +INF norm), into the exact list
            const unsigned opos = atomicAdd(&out[3], 1u);
            if (opos < ocap)
                olist[opos] = (unsigned)i;
            v[0] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
            v[1] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
            vmax = 0.0f;
            nrm = 0.0f;
        }
        const unsigned c = code[i];
        const size_t pos = (size_t)tile_start[c] * 32 + atomicAdd(&fill[c], 1u);
        frag[(pos >> 5) * 64 + (pos & 31)] = v[0];
        frag[(pos >> 5) * 64 + 32 + (pos & 31)] = v[1];
        norms[pos] = real ? nrm : INFINITY;
        norms2[pos] = pack_norm22(real ? nrm : INFINITY);
        perm[pos] = (unsigned)i;
    }
    vmax = wave_max_f(vmax);
    nrm = wave_max_f(nrm);
    __shared__ float s_v[4], s_n[4];
    if ((threadIdx.x & 63) == 0) {
        s_v[threadIdx.x >> 6] = vmax;
        s_n[threadIdx.x >> 6] = nrm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        guarded_atomic_max(&out[0], __float_as_uint(fmaxf(fmaxf(s_v[0], s_v[1]), fmaxf(s_v[2], s_v[3]))));
        guarded_atomic_max(&out[1], __float_as_uint(fmaxf(fmaxf(s_n[0], s_n[1]), fmaxf(s_n[2], s_n[3]))));
    }
    // (out[2], knn_frag_kernel's count of values beyond fp16's range, stays 0 here: such rows fail the |x| <= 1
    // test above and are on the exact list)
}

// ---- the two-pass build (round 3) ---------------------------------------------------------------------------
// The one-pass placement above reads the rows once and writes every row's 44 bytes as five pieces to a random place of a
// 0.6 GB layout: 3.2 GB of HBM writes for 0.73 GB of output at n = 2^24 (partial lines), and 16 M atomics on 2^16
// counters in front of it.  Two-pass: the rows are first grouped by the TOP 8 BITS of their cell code — 256 buckets of
// consecutive cells, 256 write streams of whole 64-byte lines — and every bucket is then placed by blocks that share
// one XCD's L2: its 2-3 MB of layout are written piecewise but leave the cache as whole lines.  Cell counts come from
// per-block LDS histograms of a bucket's records instead of one global atomic per row.
#define CELL_BUCKETS 256
#define CELL_PLACE_PARTS 16   // blocks per bucket in the placement pass

#define CELL_BUILD_ROWS 4096   // rows (records) a block of the build's passes handles: 16 per thread

// the cell code of a row held in registers
__device__ __forceinline__ unsigned cell_code_of(const float (&x)[16], const CellGeom &g, const float *__restrict__ bounds)
{
    unsigned c = 0u;
#pragma unroll
    for (int d = 0; d < 16; ++d)
        if (d < g.k && g.nb[d])
            c |= cell_bin(bounds + d * (CELL_MAX_BINS - 1), 1 << g.nb[d], x[d]) << g.shift[d];
    return c;
}

// A: code of every row + how many rows each bucket gets.  (A lane reads its 64-byte row as four 16-byte loads when k = 16:
// sixteen 4-byte loads at a 64-byte stride kept the texture path busy for 0.9 ms of a pass that moves 1 GB.)
__global__ __launch_bounds__(256) void knn_cells_bucket_count_kernel(const float *__restrict__ R, long long n, CellGeom g,
                                                                     const float *__restrict__ bounds, int bshift,
                                                                     unsigned *__restrict__ code,
                                                                     unsigned *__restrict__ bucket_counts,
                                                                     unsigned *__restrict__ bad)
{
    __shared__ unsigned s_h[CELL_BUCKETS];
    __shared__ float s_bnd[16 * (CELL_MAX_BINS - 1)];
    s_h[threadIdx.x] = 0u;
    if (threadIdx.x < 16 * (CELL_MAX_BINS - 1))
        s_bnd[threadIdx.x] = bounds[threadIdx.x];
    __syncthreads();
    const bool vec = g.k == 16 && ((uintptr_t)R & 15u) == 0;
    const long long i0 = (long long)blockIdx.x * CELL_BUILD_ROWS;
    for (int it = 0; it < CELL_BUILD_ROWS / 256; ++it) {
        const long long i = i0 + it * 256 + threadIdx.x;
        if (i < n) {
            float x[16];
            if (vec) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f4v v = __builtin_nontemporal_load(&((const f4v *)(R + (size_t)i * 16))[j]);
                    x[4 * j] = v[0];
                    x[4 * j + 1] = v[1];
                    x[4 * j + 2] = v[2];
                    x[4 * j + 3] = v[3];
                }
            } else {
#pragma unroll
                for (int d = 0; d < 16; ++d)
                    x[d] = d < g.k ? R[(size_t)i * g.k + d] : 0.0f;
            }
            const unsigned c = cell_local(cell_code_of(x, g, s_bnd), g, bad);
            code[i] = c;
            atomicAdd(&s_h[c >> bshift], 1u);
        }
    }
    __syncthreads();
    if (s_h[threadIdx.x] != 0u)
        atomicAdd(&bucket_counts[threadIdx.x], s_h[threadIdx.x]);
}

// Block-wide helper of the build's passes: s_h[256] holds a histogram of the block's 4096 items over 256 bins; on return
// s_start[bin] = first slot of the bin in the block's sorted order (exclusive prefix), s_h unchanged.  256 threads.
__device__ __forceinline__ void block_prefix_256(const unsigned *__restrict__ s_h, unsigned *__restrict__ s_start,
                                                 unsigned *__restrict__ s_wsum)
{
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const unsigned v = s_h[threadIdx.x];
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(inc, off, KNN_WAVE);
        if (lane >= (unsigned)off)
            inc += o;
    }
    if (lane == 63u)
        s_wsum[w] = inc;
    __syncthreads();
    unsigned base = 0u;
    for (unsigned j = 0; j < w; ++j)
        base += s_wsum[j];
    s_start[threadIdx.x] = base + inc - v;
    __syncthreads();
}

// B: every row to the next free record of its bucket: 64 bytes of coordinates (k of them used) + (code << 32 | row).  A block
// counts its 4096 rows per bucket first and reserves its room in every bucket with ONE atomic (one per row's block of 256
// was 16 M returning atomics on 256 words: 1.6 ms), then writes in BUCKET order — a counting sort of the rows' numbers in
// LDS — so that the ~16 records it adds to a bucket leave as one 1 KiB run (in row order they were 64-byte pieces spread
// over time: 0.94 ms against 0.6).
__global__ __launch_bounds__(256) void knn_cells_bucket_scatter_kernel(const float *__restrict__ R, long long n, int k, int bshift,
                                                                       const unsigned *__restrict__ code,
                                                                       const unsigned *__restrict__ bucket_start,
                                                                       unsigned *__restrict__ bucket_fill,
                                                                       float *__restrict__ trows, u64 *__restrict__ tmeta)
{
    __shared__ unsigned s_h[CELL_BUCKETS], s_start[CELL_BUCKETS], s_cur[CELL_BUCKETS], s_base[CELL_BUCKETS], s_wsum[4];
    __shared__ unsigned short s_order[CELL_BUILD_ROWS];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const long long i0 = (long long)blockIdx.x * CELL_BUILD_ROWS;
    unsigned cs[CELL_BUILD_ROWS / 256];
#pragma unroll
    for (int it = 0; it < CELL_BUILD_ROWS / 256; ++it) {
        const long long i = i0 + it * 256 + threadIdx.x;
        cs[it] = i < n ? code[i] : 0u;
        if (i < n)
            atomicAdd(&s_h[cs[it] >> bshift], 1u);
    }
    __syncthreads();
    block_prefix_256(s_h, s_start, s_wsum);
    {
        const unsigned cnt = s_h[threadIdx.x];   // thread t reserves the block's room in bucket t
        s_base[threadIdx.x] = cnt != 0u ? bucket_start[threadIdx.x] + atomicAdd(&bucket_fill[threadIdx.x], cnt) : 0u;
        s_cur[threadIdx.x] = s_start[threadIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < CELL_BUILD_ROWS / 256; ++it)
        if (i0 + it * 256 + threadIdx.x < n)
            s_order[atomicAdd(&s_cur[cs[it] >> bshift], 1u)] = (unsigned short)(it * 256 + threadIdx.x);
    __syncthreads();
    const unsigned nrows = (unsigned)min((long long)CELL_BUILD_ROWS, n - i0);
    const bool vec = k == 16 && ((uintptr_t)R & 15u) == 0;
    for (unsigned slot = threadIdx.x; slot < nrows; slot += 256u) {
        const unsigned src = s_order[slot];
        const long long i = i0 + src;
        const unsigned c = code[i];
        const unsigned bk = c >> bshift;
        const size_t pos = (size_t)s_base[bk] + (slot - s_start[bk]);
        const float *__restrict__ x = R + (size_t)i * k;
        float *__restrict__ t = trows + pos * 16;
        if (vec) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                ((f4v *)t)[j] = ((const f4v *)x)[j];
        } else {
            for (int d = 0; d < k; ++d)
                t[d] = x[d];
        }
        tmeta[pos] = ((u64)c << 32) | (u64)(unsigned)i;
    }
}

// ---- the fast build (round 5): no pass over the rows for counts, no host round trip between the passes ---------------
// B': A and B in one kernel, for buckets of FIXED room (`cap` records each: the caller sizes it for rows that spread evenly
// over the buckets + 1/8, which is what the quantile cuts give on data they fit; a bucket that outgrows its room raises
// `overflow` and the caller builds again with the counted passes above).  The block reads its 4096 rows ONCE from memory —
// codes worked out from the rows on the fly and parked in LDS, no `code` array — and copies them in bucket order four lanes
// to a row: every load and store of the copy is a whole 64-byte line (one lane per row was four instructions touching 64
// different lines each).  The second read of a row comes out of the L2 (the block's rows are 256 KiB).
// R / n: the rows [row0, row0 + n) of the shard (a chunk of an ingest, or all of it): tmeta carries row0 + the row's number in R.
__global__ __launch_bounds__(256) void knn_cells_bucket_scatter_fixed_kernel(const float *__restrict__ R, long long n, long long row0, CellGeom g,
                                                                             const float *__restrict__ bounds, int bshift, unsigned cap,
                                                                             unsigned *__restrict__ bucket_fill,
                                                                             float *__restrict__ trows, u64 *__restrict__ tmeta,
                                                                             unsigned *__restrict__ overflow)
{
    __shared__ unsigned s_h[CELL_BUCKETS], s_start[CELL_BUCKETS], s_cur[CELL_BUCKETS], s_base[CELL_BUCKETS], s_wsum[4];
    __shared__ unsigned short s_order[CELL_BUILD_ROWS], s_code[CELL_BUILD_ROWS];
    __shared__ float s_bnd[16 * (CELL_MAX_BINS - 1)];
    s_h[threadIdx.x] = 0u;
    if (threadIdx.x < 16 * (CELL_MAX_BINS - 1))
        s_bnd[threadIdx.x] = bounds[threadIdx.x];
    __syncthreads();
    const long long i0 = (long long)blockIdx.x * CELL_BUILD_ROWS;
    const bool vec = g.k == 16 && ((uintptr_t)R & 15u) == 0;
    if (vec) {
        // four lanes to a row, 16 bytes each: the block reads its 256 KiB as one linear stream (a lane per row was four
        // instructions, each touching 64 different lines).  A lane bins its four dimensions, the quad ORs the pieces.
        const unsigned q = threadIdx.x & 3u;
        unsigned nbq[4], shq[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            nbq[e] = g.nb[4 * q + e];      // (a dependent load from the kernel arguments per lane: once, outside the loop)
            shq[e] = g.shift[4 * q + e];
        }
#pragma unroll 4
        for (int it = 0; it < CELL_BUILD_ROWS / 64; ++it) {
            const unsigned row = (unsigned)it * 64u + (threadIdx.x >> 2);
            const long long i = i0 + row;
            unsigned c = 0u;
            if (i < n) {
                const f4v v = ((const f4v *)(R + (size_t)i * 16))[q];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (nbq[e])
                        c |= cell_bin(s_bnd + (4 * q + e) * (CELL_MAX_BINS - 1), 1 << nbq[e], v[e]) << shq[e];
            }
            c |= (unsigned)__shfl_xor((int)c, 1, KNN_WAVE);
            c |= (unsigned)__shfl_xor((int)c, 2, KNN_WAVE);
            if (q == 0u && i < n) {
                s_code[row] = (unsigned short)c;
                atomicAdd(&s_h[c >> bshift], 1u);
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < CELL_BUILD_ROWS / 256; ++it) {
            const long long i = i0 + it * 256 + threadIdx.x;
            if (i < n) {
                float x[16];
#pragma unroll
                for (int d = 0; d < 16; ++d)
                    x[d] = d < g.k ? R[(size_t)i * g.k + d] : 0.0f;
                const unsigned c = cell_code_of(x, g, s_bnd);   // (no shard geometry on this path: local = global code, < 2^16)
                s_code[it * 256 + threadIdx.x] = (unsigned short)c;
                atomicAdd(&s_h[c >> bshift], 1u);
            }
        }
    }
    __syncthreads();
    block_prefix_256(s_h, s_start, s_wsum);
    {
        const unsigned cnt = s_h[threadIdx.x];   // thread t reserves the block's room in bucket t
        unsigned at = 0u;
        if (cnt != 0u) {
            at = atomicAdd(&bucket_fill[threadIdx.x], cnt);
            if (at + cnt > cap)
                atomicOr(overflow, 1u);
        }
        s_base[threadIdx.x] = at;   // position INSIDE the bucket; records beyond `cap` are not written
        s_cur[threadIdx.x] = s_start[threadIdx.x];
    }
    __syncthreads();
    const unsigned nrows = (unsigned)min((long long)CELL_BUILD_ROWS, n - i0);
    for (unsigned j = threadIdx.x; j < nrows; j += 256u)
        s_order[atomicAdd(&s_cur[(unsigned)s_code[j] >> bshift], 1u)] = (unsigned short)j;
    __syncthreads();
    if (vec) {
        const unsigned q = threadIdx.x & 3u;
        for (unsigned slot = threadIdx.x >> 2; slot < nrows; slot += 64u) {
            const unsigned src = s_order[slot];
            const unsigned c = s_code[src];
            const unsigned bk = c >> bshift;
            const unsigned inb = s_base[bk] + (slot - s_start[bk]);
            if (inb < cap) {
                const size_t pos = (size_t)bk * cap + inb;
                // (streaming stores: the records are read next by another kernel; the block's own rows should stay cached for
                // this second read of them)
                __builtin_nontemporal_store(((const f4v *)(R + (size_t)(i0 + src) * 16))[q], &((f4v *)(trows + pos * 16))[q]);
                if (q == 0u)
                    __builtin_nontemporal_store(((u64)c << 32) | (u64)(unsigned)(row0 + i0 + src), &tmeta[pos]);
            }
        }
    } else {
        for (unsigned slot = threadIdx.x; slot < nrows; slot += 256u) {
            const unsigned src = s_order[slot];
            const unsigned c = s_code[src];
            const unsigned bk = c >> bshift;
            const unsigned inb = s_base[bk] + (slot - s_start[bk]);
            if (inb < cap) {
                const size_t pos = (size_t)bk * cap + inb;
                const float *__restrict__ x = R + (size_t)(i0 + src) * g.k;
                float *__restrict__ t = trows + pos * 16;
                for (int d = 0; d < g.k; ++d)
                    t[d] = x[d];
                tmeta[pos] = ((u64)c << 32) | (u64)(unsigned)(row0 + i0 + src);
            }
        }
    }
}

// C1': the cells' tile ranges and the scan's items from the cell counts, on the device (rounds 2-4: counts to the host, prefix
// there, tile ranges and items back).  One cell per thread, 1024 cells per block: block b first adds up what the cells in
// front of its own need (every block reads the counts before its range again — 8 MB out of the L2 in all at 2^16 cells — instead
// of waiting for its neighbours), then scans its own 1024.  Everything is read and written with consecutive lanes on
// consecutive words (a first form — one block, 64 consecutive cells per thread — took 97-176 us: 64 lines per instruction
// from ONE compute unit).  res = {tiles, items, rows of the largest cell}; the caller zeroes counts[] afterwards (it
// becomes the placement's fill counters).
__global__ __launch_bounds__(1024) void knn_cells_prefix_kernel(const unsigned *__restrict__ counts, unsigned ncells,
                                                                unsigned *__restrict__ tile_start, u64 *__restrict__ items,
                                                                unsigned *__restrict__ res)
{
    __shared__ unsigned s_t[1024], s_i[1024], s_red[3][16];
    const unsigned first = blockIdx.x * 1024u, c = first + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned bt = 0u, bi = 0u;   // what the cells in front of this block need
    for (unsigned j = threadIdx.x; j < first; j += 1024u) {
        const unsigned t = (counts[j] + 31u) / 32u;
        bt += t;
        bi += (t + KNN_CELL_ITEM_TILES - 1u) / KNN_CELL_ITEM_TILES;
    }
    const unsigned rows = c < ncells ? counts[c] : 0u;
    const unsigned tiles = (rows + 31u) / 32u, nit = (tiles + KNN_CELL_ITEM_TILES - 1u) / KNN_CELL_ITEM_TILES;
    unsigned big = rows;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bt += (unsigned)__shfl_xor((int)bt, off, KNN_WAVE);
        bi += (unsigned)__shfl_xor((int)bi, off, KNN_WAVE);
        big = max(big, (unsigned)__shfl_xor((int)big, off, KNN_WAVE));
    }
    if (lane == 0u) {
        s_red[0][w] = bt;
        s_red[1][w] = bi;
        s_red[2][w] = big;
    }
    s_t[threadIdx.x] = tiles;
    s_i[threadIdx.x] = nit;
    __syncthreads();
    bt = bi = big = 0u;
    for (int j = 0; j < 16; ++j) {
        bt += s_red[0][j];
        bi += s_red[1][j];
        big = max(big, s_red[2][j]);
    }
    for (unsigned off = 1u; off < 1024u; off <<= 1) {   // inclusive scans of the block's own cells (Hillis-Steele, 10 steps)
        const unsigned a = threadIdx.x >= off ? s_t[threadIdx.x - off] : 0u, b = threadIdx.x >= off ? s_i[threadIdx.x - off] : 0u;
        __syncthreads();
        s_t[threadIdx.x] += a;
        s_i[threadIdx.x] += b;
        __syncthreads();
    }
    if (c < ncells) {
        const unsigned tb = bt + s_t[threadIdx.x] - tiles;
        unsigned ib = bi + s_i[threadIdx.x] - nit;
        tile_start[c] = tb;
        for (unsigned t0 = 0u; t0 < tiles; t0 += KNN_CELL_ITEM_TILES)   // (one item per cell on data the cuts fit)
            items[ib++] = ((u64)c << 48) | ((u64)min((unsigned)KNN_CELL_ITEM_TILES, tiles - t0) << 40) | (u64)(tb + t0);
    }
    if (threadIdx.x == 0u)
        atomicMax(&res[2], big);
    if (c == ncells - 1u) {   // the last cell's thread has the totals
        tile_start[ncells] = bt + s_t[threadIdx.x];
        res[0] = bt + s_t[threadIdx.x];
        res[1] = bi + s_i[threadIdx.x];
    }
}

// C1: rows per cell from the buckets' records (a bucket's cells are consecutive: an LDS histogram per block).
// (bucket_fill, nullable: the fast build's buckets have fixed room — bucket b holds records [bucket_start[b], + bucket_fill[b]))
__device__ __forceinline__ unsigned bucket_end(const unsigned *__restrict__ bucket_start, const unsigned *__restrict__ bucket_fill, unsigned b)
{
    const unsigned r0 = bucket_start[b], room = bucket_start[b + 1] - r0;
    return bucket_fill ? r0 + min(bucket_fill[b], room) : r0 + room;
}

__global__ __launch_bounds__(256) void knn_cells_bucket_cellcount_kernel(const u64 *__restrict__ tmeta,
                                                                         const unsigned *__restrict__ bucket_start, int bshift,
                                                                         unsigned *__restrict__ counts,
                                                                         const unsigned *__restrict__ bucket_fill)
{
    __shared__ unsigned s_h[256];   // cells of one bucket (2^bshift <= 256: bits <= 16)
    const unsigned b = blockIdx.x / CELL_PLACE_PARTS, part = blockIdx.x % CELL_PLACE_PARTS;
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned r0 = bucket_start[b], r1 = bucket_end(bucket_start, bucket_fill, b);
    const unsigned len = (r1 - r0 + CELL_PLACE_PARTS - 1u) / CELL_PLACE_PARTS;
    const unsigned a = min(r0 + part * len, r1), e = min(a + len, r1);
    for (unsigned i = a + threadIdx.x; i < e; i += 256u)
        atomicAdd(&s_h[(unsigned)(tmeta[i] >> 32) & ((1u << bshift) - 1u)], 1u);
    __syncthreads();
    if (threadIdx.x < (1u << bshift) && s_h[threadIdx.x] != 0u)
        atomicAdd(&counts[((size_t)b << bshift) + threadIdx.x], s_h[threadIdx.x]);
}

// C2: a bucket's records to their places in the layout: what knn_cells_scatter_frag_kernel writes for a row (same
// arithmetic, same outlier rule).  All CELL_PLACE_PARTS blocks of a bucket run on ONE XCD (blocks go to the XCDs round robin),
// 32 buckets per XCD one after the other.  A block walks its records in runs of 4096: cells counted in LDS, the run's room
// in every cell reserved with one atomic per cell, ranks from LDS.
__global__ __launch_bounds__(256) void knn_cells_place_kernel(
    const float *__restrict__ trows, const u64 *__restrict__ tmeta, const unsigned *__restrict__ bucket_start, int k, int bshift,
    const unsigned *__restrict__ tile_start, unsigned *__restrict__ fill, const float *__restrict__ center, float sigma,
    h8 *__restrict__ frag, float *__restrict__ norms, unsigned *__restrict__ norms2, unsigned *__restrict__ perm,
    unsigned *__restrict__ out, unsigned *__restrict__ olist, unsigned ocap, const unsigned *__restrict__ bucket_fill)
{
    __shared__ unsigned s_h[256], s_start[256], s_cur[256], s_pos[256], s_wsum[4];
    __shared__ unsigned short s_order[CELL_BUILD_ROWS];
    __shared__ float s_c[16];
    const unsigned xcd = blockIdx.x & 7u, jb = blockIdx.x >> 3;
    const unsigned b = (jb / CELL_PLACE_PARTS) * 8u + xcd, part = jb % CELL_PLACE_PARTS;
    const unsigned r0 = bucket_start[b], r1 = bucket_end(bucket_start, bucket_fill, b);
    const unsigned len = (r1 - r0 + CELL_PLACE_PARTS - 1u) / CELL_PLACE_PARTS;
    const unsigned a = min(r0 + part * len, r1), e = min(a + len, r1);
    const unsigned cmask = (1u << bshift) - 1u;
    if (threadIdx.x < 16)
        s_c[threadIdx.x] = threadIdx.x < (unsigned)k ? center[threadIdx.x] : 0.0f;
    float vmax = 0.0f, nmaxv = 0.0f;
    for (unsigned run = a; run < e; run += CELL_BUILD_ROWS) {   // (block-uniform)
        __syncthreads();   // the previous run's tables are done with
        s_h[threadIdx.x] = 0u;
        __syncthreads();
        unsigned cl[CELL_BUILD_ROWS / 256];
#pragma unroll
        for (int it = 0; it < CELL_BUILD_ROWS / 256; ++it) {
            const unsigned i = run + it * 256 + threadIdx.x;
            cl[it] = i < e ? (unsigned)(tmeta[i] >> 32) & cmask : 0u;
            if (i < e)
                atomicAdd(&s_h[cl[it]], 1u);
        }
        __syncthreads();
        block_prefix_256(s_h, s_start, s_wsum);
        {
            const unsigned cnt = s_h[threadIdx.x];   // thread t: cell t of the bucket
            const unsigned c = (b << bshift) + threadIdx.x;
            s_pos[threadIdx.x] = cnt != 0u ? tile_start[c] * 32u + atomicAdd(&fill[c], cnt) : 0u;
            s_cur[threadIdx.x] = s_start[threadIdx.x];
        }
        __syncthreads();
        // the run's records in CELL order (counting sort of their numbers): the ~16 a cell gets go to consecutive places
#pragma unroll
        for (int it = 0; it < CELL_BUILD_ROWS / 256; ++it)
            if (run + it * 256 + threadIdx.x < e)
                s_order[atomicAdd(&s_cur[cl[it]], 1u)] = (unsigned short)(it * 256 + threadIdx.x);
        __syncthreads();
        const unsigned nrec = min((unsigned)CELL_BUILD_ROWS, e - run);
        for (unsigned slot = threadIdx.x; slot < nrec; slot += 256u) {
            const unsigned i = run + s_order[slot];
            const u64 meta = tmeta[i];
            const unsigned c = (unsigned)(meta >> 32), row = (unsigned)meta;
            const f4v *__restrict__ x4 = (const f4v *)(trows + (size_t)i * 16);
            bool real = true;
            float nrm = 0.0f, vm = 0.0f;
            h8 v[2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const f4v xa = x4[2 * half], xb = x4[2 * half + 1];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const int d = half * 8 + jj;
                    const float xv = jj < 4 ? xa[jj] : xb[jj - 4];
                    const float sc = d < k ? (xv - s_c[d]) * sigma : 0.0f;   // fp32 subtract, exact power-of-two scale
                    const _Float16 hval = (_Float16)sc;                      // round to nearest even
                    const float back = (float)hval;
                    real = real && fabsf(back) <= 1.0f;                      // outside the robust box, NaN included
                    vm = fmaxf(vm, fabsf(back));
                    nrm = nrm + back * back;                                 // exact products, fp32 sum
                    v[half][jj] = hval;
                }
            }
            if (!real) {   // out of the filter (zero fragment, +INF norm), into the exact list
                const unsigned opos = atomicAdd(&out[3], 1u);
                if (opos < ocap)
                    olist[opos] = row;
                v[0] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
                v[1] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
                vm = 0.0f;
                nrm = 0.0f;
            }
            const size_t pos = (size_t)s_pos[c & cmask] + (slot - s_start[c & cmask]);
            frag[(pos >> 5) * 64 + (pos & 31)] = v[0];
            frag[(pos >> 5) * 64 + 32 + (pos & 31)] = v[1];
            norms[pos] = real ? nrm : INFINITY;
            norms2[pos] = pack_norm22(real ? nrm : INFINITY);
            perm[pos] = row;
            vmax = fmaxf(vmax, vm);
            nmaxv = fmaxf(nmaxv, nrm);
        }
    }
    vmax = wave_max_f(vmax);
    nmaxv = wave_max_f(nmaxv);
    __shared__ float s_v[4], s_n[4];
    if ((threadIdx.x & 63) == 0) {
        s_v[threadIdx.x >> 6] = vmax;
        s_n[threadIdx.x >> 6] = nmaxv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        guarded_atomic_max(&out[0], __float_as_uint(fmaxf(fmaxf(s_v[0], s_v[1]), fmaxf(s_v[2], s_v[3]))));
        guarded_atomic_max(&out[1], __float_as_uint(fmaxf(fmaxf(s_n[0], s_n[1]), fmaxf(s_n[2], s_n[3]))));
    }
}

// The padding of every cell's last tile: positions [rows of the cell, its tiles x 32) get what the scan must see there — zero
// fragment, +INF norm (never a score under a threshold), no row.  32 threads per cell, after the placement (fill[c] = rows
// placed).  Rounds 2-3 memset the whole layout first: 0.76 GB of writes for 46 MB of padding at C3.
__global__ __launch_bounds__(256) void knn_cells_pad_kernel(const unsigned *__restrict__ tile_start, const unsigned *__restrict__ fill,
                                                            unsigned ncells, h8 *__restrict__ frag, float *__restrict__ norms,
                                                            unsigned *__restrict__ norms2, unsigned *__restrict__ perm, int kt, int nif)
{
    const unsigned c = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, j = threadIdx.x & 31u;   // 32 threads per cell: at most 31 pads
    if (c >= ncells)
        return;
    const size_t pos = (size_t)tile_start[c] * 32 + fill[c] + j, end = (size_t)tile_start[c + 1u] * 32;
    if (pos < end) {
        for (int t = 0; t < 2 * kt; ++t) {   // (kt K-steps x two halves of 32 lanes)
            h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            // (kt = 2, k <= 30: K-slot 30 carries the norm — a padding row's: the finite 65504.  A query near kAmaxLimit can have a
            // threshold above it; the position is then a record that the re-rank ignores, perm = ~0: see knn_cells_scatter_frag2_kernel's note)
            if (nif && t == 3)
                z[6] = __builtin_bit_cast(_Float16, (unsigned short)0x7BFFu);
            frag[(pos >> 5) * 64 * kt + t * 32 + (pos & 31)] = z;
        }
        norms[pos] = INFINITY;
        norms2[pos] = 0x00007C00u;
        perm[pos] = 0xFFFFFFFFu;
    }
}

__device__ __forceinline__ float min_tree16(const f16v &x, float seed)
{
    const float m0 = min3f(x[0], x[1], x[2]);
    const float m1 = min3f(x[3], x[4], x[5]);
    const float m2 = min3f(x[6], x[7], x[8]);
    const float m3 = min3f(x[9], x[10], x[11]);
    const float m4 = min3f(x[12], x[13], x[14]);
    const float m5 = min3f(m0, m1, m2);
    const float m6 = min3f(m3, m4, x[15]);
    return min3f(m5, m6, seed);
}

// Cell-major matching: a block of 8 waves owns cells 64b .. 64b+63 (one high-table entry, 64 consecutive
// low-table entries).  Pass 1 (queries on the lanes, an eighth of the batch per wave): which queries at least ONE of the
// block's 64 cells will list — the list test (knn_cell_listed) on the smallest of the block's 64 low entries, which the prep
// kernel left in lo_min[group][query]; fp32 addition does not decrease when an operand grows, so this queue is exactly the
// union of the 64 lists (knn_cell_queued, tests/test_match_prefilter_logic.py) — compacted into an LDS queue: 153 of 1024
// queries at C3 on uniform data, against 258 that get past the high table alone (what this pass queued before; a final list
// holds 27).  Pass 2 (cells on the lanes, the queue cut into one run per wave): the low-table entry of each queued query, 24 loads
// in flight per wave; survivors go to the cell's list at offsets prefix-summed over the waves.  cell_counts[c] = queries
// that could not rule cell c out, lists[c][0..) = their numbers.  No global atomics: per-cell
// appends with returning atomics ran at 22 per ns, 0.13 ms for this batch (tools/atomic_probe).
#define CELL_MATCH_STAGED_CAP 640u
template <int CELL_MATCH_WAVES>   // 8, or 16 for shards of few cells (one block per 64 cells: 128 blocks at 2^13 cells)
__global__ __launch_bounds__(64 * CELL_MATCH_WAVES) void knn_cells_match_kernel(
    const float *__restrict__ lo_tab, const float *__restrict__ hi_tab, const float *__restrict__ lo_min, const float *__restrict__ dup, int m,
    int m_padded, CellGeom g, unsigned ncells, unsigned cap, unsigned short *__restrict__ lists,
    unsigned *__restrict__ cell_counts, unsigned *__restrict__ ctl,
    unsigned stage)   // entries of a list assembled in LDS (<= cap; 0: none): the launch's dynamic LDS holds 64 x (stage + 2) of them
{
    __shared__ unsigned short s_q[1024];
    __shared__ float s_hv[1024], s_dq[1024];
    __shared__ unsigned s_npass, s_flag, s_wcnt[CELL_MATCH_WAVES][64];
    // the first `stage` entries of every list are put together in LDS (dynamic: 64 rows of stage + 2 entries — a row stride of an
    // odd number of dwords, 65 at 128: lanes appending at the same depth hit different banks) and written out as whole rows;
    // what lies beyond goes straight to memory (k <= 16: stage = 128, lists are 25-125 entries long on uniform data).  (16 < k <= 32, lists of 384 / 640: written straight to memory —
    // ten million two-byte stores 768 bytes apart at k = 20 — the launch took 75 us at C3's shape; staged in LDS 0.326 -> 0.304 ms per step at k = 20, 0.810 -> 0.709 at k = 24)
    extern __shared__ __attribute__((aligned(16))) unsigned short s_list[];
    const unsigned lstride = stage + 2u;
    // (the flag is read ONCE per block: other blocks of this launch may raise it, and threads of one block must not
    // disagree about leaving before the barriers below)
    if (threadIdx.x == 0)
        s_flag = ctl[KNN_CTL_FALLBACK];
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned c0 = blockIdx.x * 64u;
    const unsigned cell = c0 + (unsigned)lane;
    const int nl = 1 << g.sa;
    const unsigned h = c0 >> g.sa;                      // block-uniform: nl >= 64
    const unsigned l = cell & (unsigned)(nl - 1);
    const float *__restrict__ hrow = hi_tab + (size_t)h * m_padded;
    const float *__restrict__ mrow = lo_min + (size_t)((c0 & (unsigned)(nl - 1)) >> 6) * m_padded;   // block-uniform: the block's 64 low entries are one group
    if (threadIdx.x == 0)
        s_npass = 0u;
    __syncthreads();
    if (s_flag != 0u)
        return;
    {   // pass 1: this wave's share of the batch (m <= 1024: 16 chunks of 64 queries over the waves)
        constexpr int U = 16 / CELL_MATCH_WAVES;
        float hv[U], dq[U], lm[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = (u * CELL_MATCH_WAVES + wib) * 64 + lane;
            hv[u] = q < m ? hrow[q] : INFINITY;
            dq[u] = q < m ? dup[q] : -INFINITY;
            lm[u] = q < m ? mrow[q] : INFINITY;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = (u * CELL_MATCH_WAVES + wib) * 64 + lane;
            const bool pass = q < m && knn_cell_queued(lm[u], hv[u], dq[u]);
            const u64 mask = __ballot(pass);
            if (mask != 0ull) {   // wave-uniform
                unsigned base = 0u;
                if (lane == 0)
                    base = atomicAdd(&s_npass, (unsigned)__popcll(mask));
                base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
                if (pass) {
                    const unsigned pos = base + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                          __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                    s_q[pos] = (unsigned short)q;
                    s_hv[pos] = hv[u];
                    s_dq[pos] = dq[u];
                }
            }
        }
    }
    __syncthreads();
    const unsigned npass = s_npass;
    unsigned short *__restrict__ my_lds = s_list + (size_t)lane * lstride, *__restrict__ my_mem = lists + (size_t)cell * cap;
    // pass 2: the queue in contiguous runs, one per wave (<= 1024 / WAVES entries); a lane keeps "my cell could not
    // rule entry j out" as bit j of a mask, the waves' counts are prefix-summed through LDS, and the second sweep
    // writes every survivor to its final place — no LDS atomics (16 waves adding to the same 64 counters cost
    // more than the table loads at 2^13 cells, where a list holds ~125 of 1024 queries), lists in the queue's order (the
    // waves' chunks of the batch in the order they reached s_npass, ascending inside a chunk).
    // (64 loads outstanding — a wave's whole run of the queue in one round trip instead of three — measured in round 4: 76-80
    // registers instead of 55-58, C3 one batch at a time 0.150 -> 0.155 ms, pipelined 0.1195 -> 0.1235.  With the queue on the
    // group minima a wave's run at C3 is 19.5 entries on average, 26 at most: 24 outstanding take it in one round trip where
    // 16 need two, at the same 64 registers — C3 pipelined 0.1011-0.1022 ms with 16, 0.0995-0.1003 with 24, 0.0994-0.1002 with
    // 28; 32 are 70 registers, three blocks per CU instead of four, 0.1017-0.1020.  profiles/r17_match_prefilter.txt)
    constexpr int EPW = 1024 / CELL_MATCH_WAVES, INFLIGHT = 24;   // entries per wave; low-table loads outstanding
    const unsigned per = (npass + CELL_MATCH_WAVES - 1u) / CELL_MATCH_WAVES;
    const unsigned e_begin = min((unsigned)wib * per, npass), e_end = min(e_begin + per, npass);
    u64 keep[EPW / 64];
#pragma unroll
    for (int w64 = 0; w64 < EPW / 64; ++w64)
        keep[w64] = 0ull;
    for (unsigned e0 = e_begin; e0 < e_end; e0 += INFLIGHT) {
        float lo[INFLIGHT];
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) {
            const unsigned e = min(e0 + (unsigned)u, e_end - 1u);
            lo[u] = lo_tab[(size_t)s_q[e] * nl + l];
        }
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) {
            const unsigned e = e0 + (unsigned)u;
            if (e < e_end) {
                const unsigned j = e - e_begin;
                if (knn_cell_listed(lo[u], s_hv[e], s_dq[e])) {
#pragma unroll
                    for (int w64 = 0; w64 < EPW / 64; ++w64)
                        if ((int)(j >> 6) == w64)
                            keep[w64] |= 1ull << (j & 63u);
                }
            }
        }
    }
    unsigned mine = 0u;
#pragma unroll
    for (int w64 = 0; w64 < EPW / 64; ++w64)
        mine += (unsigned)__popcll(keep[w64]);
    s_wcnt[wib][lane] = mine;
    __syncthreads();
    unsigned pos = 0u, total = 0u;
    for (int w = 0; w < CELL_MATCH_WAVES; ++w) {
        const unsigned v = s_wcnt[w][lane];
        pos += w < wib ? v : 0u;
        total += v;
    }
#pragma unroll
    for (int w64 = 0; w64 < EPW / 64; ++w64)
        for (u64 bits = keep[w64]; bits != 0ull; bits &= bits - 1ull) {
            const unsigned e = e_begin + (unsigned)w64 * 64u + (unsigned)__builtin_ctzll(bits);
            if (pos < stage)
                my_lds[pos] = s_q[e];
            else if (pos < cap)
                my_mem[pos] = s_q[e];   // (beyond the staged part: rare where the lists are short, the rule where nothing is staged)
            ++pos;
        }
    if (wib == 0) {
        cell_counts[cell] = total;   // (> cap: the list is cut short and the scan scores the cell against the whole batch)
    }
    __syncthreads();
    if (stage != 0u) {
        for (int j = wib; j < 64; j += CELL_MATCH_WAVES) {
            unsigned cj = 0u;
            for (int w = 0; w < CELL_MATCH_WAVES; ++w)
                cj += s_wcnt[w][j];
            cj = min(cj, stage);
            for (unsigned d = (unsigned)lane; d * 2u < cj; d += 64u)
                ((unsigned *)(lists + (size_t)(c0 + (unsigned)j) * cap))[d] = ((const unsigned *)(s_list + (size_t)j * lstride))[d];
        }
    }
}

// The scan.  A block's waves share the batch's B operands and thresholds in LDS.  Per item a wave issues every load it
// needs at once (tiles, norms, list: one round trip), and the kernel is written lean (~80 VGPRs, 12 waves per block) so
// that 5-6 waves per SIMD each have an item in flight.  The C tile (norms) goes through a per-wave LDS window, four
// broadcast ds_read_b128 per tile and block of queries.  (Round 3 measured the C tile out of one extra MFMA on split norms
// instead: 115-138 VGPRs, slower at every size — tools/arms/README.md.)
#define CELL_SCAN_WAVES 12
#define CELL_SCAN_WAVES_KT2 16   // 16 < k <= 32: one block per CU (74 KiB of operands), 4 waves per SIMD, 128 registers each
#define CELL_SCAN_CHUNK 256   // slots of a block's share whose tile ranges and list lengths sit in LDS at a time (DYN)
#define CELL_INLINE_RERANK_MAX 64u   // records a scan wave re-ranks itself; a longer list is left to the tail kernel
#define CELL_PUBLISH_STEP 64u             // records between two publications of a wave's count to the batch's counter
#define CELL_BATCH_RECORD_LIMIT (1u << 19)   // records of a batch beyond which it goes to the exact evaluation of its listed pairs
#define CELL_TOPK_RECORD_LIMIT (1u << 21)    // the same for a top-K batch (then: FALLBACK, the exact top-K): 2048 records per query of a
                                             // full pass.  Chosen, not measured: four times the 1-NN limit, and half the record buffer, so
                                             // that the waves' slices (the other half, evenly dealt) still hold a pass at the limit
#define CELL_SCAN_RUN 16      // DYN: consecutive items a block takes at a time; its next run lies gridDim.x runs further on

// An 8-bit row tile's lane (8 codes, byte j = K-slot j) as the fp16 A operand (code - 128) / 128: v_perm_b32 puts each code under
// the high byte 0x48 — the fp16 number 8 + code / 128, exact (8 <= x < 16: steps of 2^-7) — and one packed add of -9 per pair
// leaves (code - 128) / 128, exact.  (perm selector byte i: 0-3 = bytes of the second source, 4-7 = bytes of the first.)
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h8 cell_widen_u8(u2v w)
{
    const h2v nine = {(_Float16)9.0f, (_Float16)9.0f};
    h8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned x = __builtin_amdgcn_perm(0x48484848u, w[i >> 1], (i & 1) ? 0x04030402u : 0x04010400u);
        const h2v p = __builtin_bit_cast(h2v, x) - nine;
        r[2 * i] = p[0];
        r[2 * i + 1] = p[1];
    }
    return r;
}

// One (tile, block of 32 listed queries) step: scores + min tree + threshold test -> hit mask.
template <int KT>
__device__ __forceinline__ u64 cell_tile_step(const h8 (&a)[KT], const f4v *__restrict__ my_nrm, int p, int half, const h8 (&b)[KT], float th)
{
    f16v d;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const f4v v = my_nrm[p * 8 + 2 * gq + half];
        d[4 * gq + 0] = v[0];
        d[4 * gq + 1] = v[1];
        d[4 * gq + 2] = v[2];
        d[4 * gq + 3] = v[3];
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk)
        d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk], b[kk], d, 0, 0, 0);
    const float mn = min_tree16(d, th);
    return __ballot(mn < th);
}

// 16 < k <= 30 (round 5): the norm rides in the fragment — K-slots 30 and 31 of a row hold its norm's two fp16 halves
// (pack_norm22: hi + mid 2^-11 = N to 2^-22 N, in rho since round 3), the scan's B operands 1 and 2^-11 there — so the two
// MFMAs of a step give N - 2 a.b out of a ZERO C tile: no norm window, no LDS reads for it.  Every (tile, block of 32 queries)
// step read 4 KiB of LDS for its C tile; at the 5-10 blocks per tile of these dimensions that was the scan's bound (k 20:
// 2.9 M steps x 4.2 KiB = 176 us of the LDS pipe's time under a 165 us HBM floor).
template <int KT>
__device__ __forceinline__ u64 cell_tile_step_nif(const h8 (&a)[KT], const h8 (&b)[KT], float th)
{
    f16v d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], b[0], zero_acc(), 0, 0, 0);
#pragma unroll
    for (int kk = 1; kk < KT; ++kk)
        d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[kk], b[kk], d, 0, 0, 0);
    const float mn = min_tree16(d, th);
    return __ballot(mn < th);
}

// |coordinate| a query may have in a cell's frame: twice that must stay an fp16 number (the B operand is -2 x the query); the
// bounds do not mind the size — every error term is relative to the pair's own amax (64 box half-widths at the largest scale).
#define CELL_FRAME_AMAX 16384.0f
static_assert(CELL_FRAME_AMAX == KNN_FRAME_AMAX, "knn_frame_dup.h restates the frame's limit");

// The centred scan's B operand and threshold for one (query, cell) pair (per-cell frames, knn_cells_recentre): lane = (query
// of the block, half of the dimensions).  The query is rounded in the CELL's frame exactly as knn_cells_prep_kernel rounds it
// in the shard's — fp32 subtract, exact power-of-two scale, fp16 to nearest even, times -2 —; amax and the computed norm mq
// are the pair's own.  The threshold is knn_threshold's last line with the constants of knn_bound_consts(k, 1, scale_c, amax,
// bmax_c, nmax_c), evaluated in fp32 with everything rounded towards "pass":
//     thr = Dup + 2 eta sqrt(Dup) + eta^2 + rho - mq (1 - gamma)          (Dup in the cell's units: Dup_q x ratio^2)
// P = the positive terms: eight fp32 operations on positive numbers, constants rounded up — within 2^-20 of exact, taken
// 10^-5 larger; mq x 0.999996 <= mq (1 - gamma)(1 - 10^-6)(1 - 2^-22) (gamma = 18 x 2^-24 = 1.07 x 10^-6; the 10^-6 is the slack
// knn_threshold gives its own double arithmetic: the fp32 value is never below the double one — tests/test_cells_logic.py checks
// 200 000 random pairs); the last subtraction rounds by at most 2^-24 (P + mq), 2.4 x 10^-7 (P + mq) is added.  A pair whose query does not fit the cell's frame: see the end.
// U8 (8-bit rows): the constants of knn_bound_consts_u8(k, 1, scale_c, amax, er_c, nmax8_c) instead — emax = thp amax + er_c + 2 nu0,
// er_c = the cell's cell_u8 word 0 taken 10^-6 larger (`er`), nmaxc = the cell's largest norm of the dequantised rows.
template <bool U8 = false>
__device__ __forceinline__ void cell_centred_operand(const float *__restrict__ s_q32, int k, unsigned qid, int half, bool valid,
                                                     const float (&cc)[8], float scale, float ratio, float bmaxc, float nmaxc, float er,
                                                     float dupq, float sqdq, h8 &b, float &th)
{
#pragma clang fp contract(off)
    // the query's fp32 row, padded to 16 dimensions with zeros, from LDS (the centre is zero there too: no masks)
    const f4v x0 = *(const f4v *)(s_q32 + (size_t)qid * 16 + 8 * half), x1 = *(const f4v *)(s_q32 + (size_t)qid * 16 + 8 * half + 4);
    const float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    float sc[8], a = 0.0f, mq = 0.0f;
    h8 hv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sc[j] = (x[j] - cc[j]) * scale;
        hv[j] = (_Float16)sc[j];
        const float back = (float)hv[j];
        a = fmaxf(a, fabsf(back));   // (+INF where a coordinate left the fp16 range; a NaN — a query that is not finite: the prep kernel has sent its batch to the exact scan — is skipped)
        mq = mq + back * back;
    }
    a = fmaxf(a, __shfl_xor(a, 32, KNN_WAVE));
    mq = mq + __shfl_xor(mq, 32, KNN_WAVE);
    b = hv * (_Float16)-2.0f;   // exact: |coordinate| <= CELL_FRAME_AMAX = 2^14 below
    const float kf = (float)k;
    const float emax = U8 ? 4.8865e-4f * a + er * 1.000001f + 1.2220e-4f   // theta' amax + er + 2 nu0
                          : 4.8865e-4f * (a + bmaxc) + 1.2220e-4f;           // theta' (amax + bmax) + 2 nu0
    const float sqk = k <= 1 ? 1.0f : k <= 4 ? 2.0f : k <= 9 ? 3.0f : 4.0f;   // >= sqrt(k), k <= 16 (no square root here: the exact kernels' ISA is checked for FMAs)
    const float eta = sqk * emax, eta2 = kf * emax * emax;
    const float rho = 1.1921e-5f * (nmaxc + 16.0f * a * a) + 1.79e-7f + 4.77e-7f * nmaxc;
    const float dupc = dupq * ratio * ratio, sqdc = sqdq * ratio;
    const float P = dupc + 2.0f * eta * sqdc + eta2 + rho;
    th = (P * 1.00001f + (P + mq) * 2.4e-7f + 1e-30f) - mq * 0.999996f;
    if (!(a <= CELL_FRAME_AMAX)) {   // (both lanes of a query take this together: `a` is the pair's)
        // The query does not fit the cell's frame (a coordinate beyond CELL_FRAME_AMAX cell units): along that coordinate it is
        // at least a32 (1 - 2^-22) - bmax_c (1 + 2^-10) - nu0 away from every row of the cell, in exact arithmetic.  Further than
        // sqrt(Dup): no row of this cell can be its answer (a `dense` cell is scored against the whole batch, queries that never
        // listed it included).  Else every real row passes — a ZERO operand leaves the rows' norms as scores (finite; an operand
        // of fp16 infinities would make them NaN, which no threshold passes) — and is re-ranked exactly, as any candidate is.
        float a32 = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            a32 = fmaxf(a32, fabsf(sc[j]));
        a32 = fmaxf(a32, __shfl_xor(a32, 32, KNN_WAVE));
        const float lb = a32 * 0.999f - bmaxc * 1.001f - 0.001f;
        const bool beyond = lb > 0.0f && lb * lb > dupc * 1.001f;   // (a32 = +INF: beyond any finite Dup)
        b = (h8){0, 0, 0, 0, 0, 0, 0, 0};
        th = dupq > -INFINITY && !beyond ? INFINITY : -INFINITY;
    }
    if (!valid)
        th = -INFINITY;
}

// ------------------------------------------------------------------------------------------
// Round 3: everything a batch needs before its cells can be matched, in ONE kernel — one block of 4 waves per query.
// Replaces knn_frag_kernel (queries) + knn_cells_seed_kernel + the keys-fill launch of round 2 (three launches, 26 us
// back to back at 1024 queries; this one 13).  Every wave rounds the query to its fp16 B operand (cheap, and each needs
// it), the block tabulates the squared gaps and the two pruning tables with all 256 threads, wave w scores seed cell w
// (own cell + the cells across the two nearest cuts) with all its tiles in flight at once, and thread 0 turns the best
// score into thr_q and Dup_q.  (One WAVE per query, the first form of this kernel, took 24 us: 34 seed tiles and 288
// table entries in one serial stream per query.)
// ------------------------------------------------------------------------------------------
#define CELL_PREP_WAVES 4
#define CELL_PREP_TILES 9     // seed tiles a wave requests at once (a cell of 144 .. 288 rows: one round trip)
#define CELL_SEED_MAX_TILES 36u   // tiles of one seed cell a query looks at (a larger cell: every stride-th tile)
#define CELL_SEED_MAX_TILES_CTR 144u   // the same with per-cell frames (clustered data: cells of thousands of tiles)
#define CELL_OUTER_SEED_TILES 2   // cell-range shards: tiles an outer seed cell of this rank contributes (the layer's depth by default)

// Where the seed tiles of cells OUTSIDE this index's range come from (cell-range shards; all zero otherwise): every rank's
// part of the replicated seed layer, `tiles` tiles per cell (ShardGeom::part_bytes).
#define KNN_MAX_RANKS 64
struct SeedLayer {
    const unsigned char *base;
    unsigned cpr, tiles;             // cells a part has room for (the largest rank's), tiles per cell
    unsigned nranks;
    unsigned long long part_bytes;
    unsigned first[KNN_MAX_RANKS + 1];   // first cell code of every rank's range (first[nranks] = the grid's cells)
};

// PW: waves per query, 4 or 2 (half the registers held while batches are in flight side by side, see knn_cells_query).
// SD: seed dimensions — the seeds are the query's own cell and every combination of moves across its SD nearest cuts:
//     2 = 4 cells (what ships; a cell of this index WHOLE, a cell of another rank through the seed layer's few tiles).  The
//     kernel is generic in SD: 4 = 16 cells leaves fewer survivors (profiles/r04_shard_sim.txt: 236 cells per query and
//     rank at N = 8 against 399, 199 with the bound one GPU would have) but measured slower end to end (knn_cells_query).
// KT: K-steps of a tile, 1 (k <= 16) or 2 (16 < k <= 32, round 5: the cuts, the gaps and the tables cover the first 16
//     dimensions; the fragments and the seed scores all of them)
// CTR: per-cell frames (knn_cells_recentre; KT = 1, no seed layer): every seed cell is scored with the query rounded in THAT
//     cell's frame, each gives its own bound Dup (frame-free: a squared distance) and the smallest stands; thr[q] = an upper
//     bound of sqrt(Dup_q) — what the centred scan's per-pair thresholds start from — instead of a score threshold
// TK: a top-K batch (knn_cells_query_topk): u = the K-th smallest (K arrives in lo_by_entry) finite score among the scored
//     rows instead of the smallest — knn_seed_kth.h has the rule, the argument and the mechanism; thr_q and Dup_q come from it
//     through the same lines below.  keys_init is null there (the select kernel starts or folds the m x K keys).  On a cell-range
//     shard (KNN_QUERY_TOPK_PARTIAL) the scored rows include other ranks' rows from the seed layer: u is then a bound over the GLOBAL
//     set, under bmax / nmax taken over all ranks' parts (knn_index_seed_attach) exactly as the 1-NN form's — DESIGN §6.1.
//     With CTR (KNN_QUERY_TOPK_FRAMES): the K-th smallest of the frame-free bounds Dup_c(u) instead — the `CTR && TK` branch below.
//     WR (with TK, never with CTR: knn_index_query_topk_within, knn_cells_prep_within_kernel): Dup_q is capped by the radius, min(Dup(u), dup_r) — knn_threshold_within —,
//     and a query with fewer than K finite scores is bounded by the radius alone instead of sending the pass to the exact top-K.
//     (The body is a file of its own, knn_cells_prep_body.inc, so that the radius form can be a kernel of its own with one argument
//     more: the other forms keep their argument lists, their names and their code as they are.)
template <int PW, int SD, int KT = 1, bool CTR = false, bool TK = false>
__global__ __launch_bounds__(64 * PW, KT == 1 && !CTR ? 4 : 3) void knn_cells_prep_kernel(   // (4 waves per SIMD: a batch of 1024 queries is resident at once)
    const float *__restrict__ Q, int m, int m_padded, CellGeom g, const float *__restrict__ bounds, double sigma2,
    const float *__restrict__ center, float sigma, const unsigned *__restrict__ tile_start, long long ntiles,
    const h8 *__restrict__ rf, const unsigned *__restrict__ rn2, SeedLayer layer, h8 *__restrict__ qfg, float *__restrict__ lo_tab,
    float *__restrict__ hi_tab, float *__restrict__ lo_min, float bmax, float nmax, float amax_limit, float *__restrict__ thr,
    float *__restrict__ dup_out, unsigned *__restrict__ ctl, unsigned *__restrict__ ctl_next,
    unsigned *__restrict__ counts, unsigned nlists, u64 *__restrict__ keys_init,
    int lo_by_entry,   // != 0: the low table as [entry][query] (what the self-listing scan reads: a cell's row is contiguous)
                       // TK: K instead — the table is [query][entry] there (match-made lists only), and one more argument
                       // would move the hidden arguments of every 1-NN instantiation (their ISA stays as it is)
    const float *__restrict__ frame, const unsigned *__restrict__ tile_cell)   // CTR only
{
#pragma clang fp contract(off)
    constexpr bool WR = false, CNT = false, EACH = false;
    constexpr float max_dist2 = 0.0f;
#include "knn_cells_prep_body.inc"
}

// The radius form of the top-K prep kernel on one-frame layouts (knn_index_query_topk_within): the TK form's body with WR, K and
// the radius arguments of their own.
template <int PW, int SD, int KT>
__global__ __launch_bounds__(64 * PW, KT == 1 ? 4 : 3) void knn_cells_prep_within_kernel(
    const float *__restrict__ Q, int m, int m_padded, CellGeom g, const float *__restrict__ bounds, double sigma2,
    const float *__restrict__ center, float sigma, const unsigned *__restrict__ tile_start, long long ntiles,
    const h8 *__restrict__ rf, const unsigned *__restrict__ rn2, SeedLayer layer, h8 *__restrict__ qfg, float *__restrict__ lo_tab,
    float *__restrict__ hi_tab, float *__restrict__ lo_min, float bmax, float nmax, float amax_limit, float *__restrict__ thr,
    float *__restrict__ dup_out, unsigned *__restrict__ ctl, unsigned *__restrict__ ctl_next,
    unsigned *__restrict__ counts, unsigned nlists, int lo_by_entry /* K */, float max_dist2)
{
#pragma clang fp contract(off)
    constexpr bool CTR = false, TK = true, WR = true, CNT = false, EACH = false;
    u64 *const keys_init = nullptr;
    const float *const frame = nullptr;
    const unsigned *const tile_cell = nullptr;
#include "knn_cells_prep_body.inc"
}

// The count form (knn_index_count_within on the cell-pruned way, knn_cells_query_count): the radius form's body with CNT — query
// fragments, gap tables, control-word and counter clearing as every form, and thr[q] / dup_out[q] = knn_threshold_within at
// u = +INF, the radius cap alone: no seed tile is read, no selection network, no seed layer.  A kernel of its own, so that the
// other forms' instantiations compile as they did.
template <int PW, int SD, int KT>
__global__ __launch_bounds__(64 * PW, KT == 1 ? 4 : 3) void knn_cells_prep_count_kernel(
    const float *__restrict__ Q, int m, int m_padded, CellGeom g, const float *__restrict__ bounds, double sigma2,
    const float *__restrict__ center, float sigma, const unsigned *__restrict__ tile_start, h8 *__restrict__ qfg,
    float *__restrict__ lo_tab, float *__restrict__ hi_tab, float *__restrict__ lo_min, float bmax, float nmax, float amax_limit, float *__restrict__ thr,
    float *__restrict__ dup_out, unsigned *__restrict__ ctl, unsigned *__restrict__ ctl_next, unsigned *__restrict__ counts,
    unsigned nlists, float max_dist2)
{
#pragma clang fp contract(off)
    constexpr bool CTR = false, TK = true, WR = true, CNT = true, EACH = false;
    constexpr int lo_by_entry = 1;   // (TK: the low table is [query][entry]; K has no meaning here)
    constexpr long long ntiles = 0;
    u64 *const keys_init = nullptr;
    const h8 *const rf = nullptr;
    const unsigned *const rn2 = nullptr;
    const SeedLayer layer = {nullptr, 0u, 0u, 0u, 0ull, {0u}};   // the empty seed layer: a count needs no seed
    const float *const frame = nullptr;
    const unsigned *const tile_cell = nullptr;
#include "knn_cells_prep_body.inc"
}

// The count form with a radius per query (knn_index_count_within_each, knn_index_list_within_each on the cell-pruned way): one
// block per query, so the block turns its OWN query's radius into the body's max_dist2 — the query's bound min(radii[qi], cap)
// (knn_each_radius.h; cap finite), or -1 when the query has no candidates (a NaN or negative radius), which the body's last lines
// answer with the threshold of a padding query.  A padding block qi >= m reads no radius.  The scan behind it never sees a radius.
template <int PW, int SD, int KT>
__global__ __launch_bounds__(64 * PW, KT == 1 ? 4 : 3) void knn_cells_prep_each_kernel(
    const float *__restrict__ Q, int m, int m_padded, CellGeom g, const float *__restrict__ bounds, double sigma2,
    const float *__restrict__ center, float sigma, const unsigned *__restrict__ tile_start, h8 *__restrict__ qfg,
    float *__restrict__ lo_tab, float *__restrict__ hi_tab, float *__restrict__ lo_min, float bmax, float nmax, float amax_limit, float *__restrict__ thr,
    float *__restrict__ dup_out, unsigned *__restrict__ ctl, unsigned *__restrict__ ctl_next, unsigned *__restrict__ counts,
    unsigned nlists, const float *__restrict__ radii, float cap)
{
#pragma clang fp contract(off)
    constexpr bool CTR = false, TK = true, WR = true, CNT = true, EACH = true;
    constexpr int lo_by_entry = 1;
    constexpr long long ntiles = 0;
    u64 *const keys_init = nullptr;
    const h8 *const rf = nullptr;
    const unsigned *const rn2 = nullptr;
    const SeedLayer layer = {nullptr, 0u, 0u, 0u, 0ull, {0u}};
    const float *const frame = nullptr;
    const unsigned *const tile_cell = nullptr;
    float max_dist2 = -1.0f;
    if ((int)blockIdx.x < m) {   // block-uniform
        const float rad = radii[blockIdx.x];
        if (knn_each_has(rad))
            max_dist2 = knn_each_bound(rad, cap) + 0.0f;   // (-0 -> +0: the threshold's arithmetic sees the scalar call's 0)
    }
#include "knn_cells_prep_body.inc"
}

// (<= 80 VGPRs: registers are handed out in eights and 6 waves x 88 do not fit a SIMD's 512)
// (HIP's second launch bound is waves per SIMD: 6 = at most 80 registers.  Left at 2 the allocator settled at 96-98 once the
// dense-cell and overflow paths were in — 4 waves per SIMD, and the kernel alone went from 0.035 to 0.042 ms at 2^21 rows)
// What ends a batch (the last block of the scan on a clean batch, else of the tail kernel): local row -> global id of the
// keys' index half when the shard's rows carry their own global numbers (cell-range shards, knn_index_create_sharded),
// and the int32 indices when the caller asked for them (knn_index_query: no separate unpack launch).
struct CellFinal {
    const unsigned *gids;   // nullable: keys hold base + row already
    int *out_idx;           // nullable
    int defer;              // != 0: more launches fold into the keys behind the scan (rows outside the robust box): the tail finalises
};

__device__ __forceinline__ void cells_finalize(u64 *__restrict__ keys, int m, const CellFinal &fin, unsigned tid, unsigned nthreads)
{
    if (!fin.gids && !fin.out_idx)
        return;
    for (unsigned i = tid; i < (unsigned)m; i += nthreads) {
        // (agent scope: the keys were folded by atomics of blocks on other XCDs; a plain load may see this XCD's stale L2 line)
        u64 key = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fin.gids && (unsigned)(key >> 32) != 0x7F800000u) {   // (+INF, 0) = nothing found: v0's index 0 stays
            key = (key & 0xFFFFFFFF00000000ull) | (u64)fin.gids[(unsigned)key];
            keys[i] = key;
        }
        if (fin.out_idx)
            fin.out_idx[i] = (int)(unsigned)key;
    }
}

#ifdef KNN_SCAN_TIMELINE
// development only (tools/build_timeline_lib.sh builds a private copy of the library with this macro, tools/scan_timeline.py
// reads it): five stamps per wave of the last scan launch — entry, LDS filled, items done, own records re-ranked, exit — of
// the 100 MHz wall clock.  The product build compiles none of it.
__device__ unsigned long long g_scan_stamps[8192 * 5];
#define SCAN_STAMP(i)                                                                                  \
    do {                                                                                               \
        if ((threadIdx.x & 63) == 0 && blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6) < 8192u)      \
            g_scan_stamps[(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 5 + (i)] = wall_clock64(); \
    } while (0)
extern "C" int knn_debug_scan_stamps(unsigned long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_scan_stamps), sizeof(unsigned long long) * 8192 * 5);
}
#else
#define SCAN_STAMP(i) do { } while (0)
#endif
// K: 16 = compile-time dimension of the inline re-rank, 0 = run-time k <= 16
// SELF: the waves make the lists of their own items (cell_self_list, knn_exact_dev.h) — no match launch in front of the scan;
//       cell_counts / lists are unused and `cap` is CELL_SELF_CAP
// KT:   K-steps of a tile: 1 (k <= 16), 2 (16 < k <= 32, round 5: tiles of 2 KiB, two MFMAs per step, 64-byte B operands — 74 KiB
//       of LDS for a batch, so a CU holds ONE block: it has 16 waves of up to 128 registers, windows of nine tiles like KT = 1;
//       K = 0 there: the inline re-rank walks k in chunks of 16 dimensions)
// CTR:  per-cell frames (knn_cells_recentre; KT = 1, lists from the match launch): the B operand and the threshold of a (query,
//       cell) pair are made here, from the fp32 query, the cell's frame and Dup_q (cell_centred_operand) — s_thr holds the
//       batch's sqrt(Dup) bounds, s_dup the Dup values, the B operands' room in LDS stays unused
// NIF:  16 < k <= 30: the norms ride in the fragments' K-slots 30, 31 (cell_tile_step_nif): no norm window
// U8:   with CTR: `rf` / `rn` are the 8-bit rows and their norms (knn_cells_recentre_kernel) — 512-byte tiles, widened to fp16 in
//       registers (cell_widen_u8) at every step; the pair's threshold from knn_bound_consts_u8's constants
//       without CTR (bin frames, knn_cells_bin_rows_kernel): the same tiles, rn = N''; the 12-wave one-frame scan with the B operands
//       of `qfg` times 2^e, s_thr = knn_u8_bin_threshold of every query (made in the fill), and per (cell, block of 32 queries)
//       the pair term B.w_c — eight exact fp32 products, fp32 sums, one swap of halves — taken off the threshold (knn_filter_dev.h)
// TOPK (the body, knn_cells_scan_body.inc, is shared with knn_cells_records_kernel below, where it is true): the record-only
//       form of a top-K pass
template <bool DYN, int K, bool SELF, int KT = 1, bool CTR = false, bool NIF = false, bool U8 = false>
__global__ __launch_bounds__(64 * (KT == 1 && !CTR ? CELL_SCAN_WAVES : CELL_SCAN_WAVES_KT2), CTR ? 4 : KT == 1 ? 6 : 4) void knn_cells_scan_kernel(
    const h8 *__restrict__ rf, const float *__restrict__ rn, const u64 *__restrict__ items, unsigned nitems,
    const h8 *__restrict__ qfg, const float *__restrict__ thrg, int m, int m_padded,
    const unsigned *__restrict__ cell_counts, const unsigned short *__restrict__ lists, unsigned cap,
    u64 *__restrict__ rec, unsigned *__restrict__ counts, unsigned *__restrict__ ctl, unsigned slice,
    unsigned ovf_base, unsigned ovf_cap,
    // the exact re-rank of this wave's own records (v0 arithmetic on the fp32 rows, through perm) and the end of the batch
    const float *__restrict__ Q, const float *__restrict__ R, int krt, const unsigned *__restrict__ perm, long long npos,
    long long base, u64 *__restrict__ keys, CellFinal fin, CellSelf self)
{
#pragma clang fp contract(off)
    constexpr bool TOPK = false;
#include "knn_cells_scan_body.inc"
}

// The record-only scan of a top-K pass (knn_cells_query_topk): the same body with TOPK = true — scoring, thresholds, lists, item
// deal and record append as they are; no inline re-rank, no atomic-min on the keys, no finalisation: the records go to the
// launches behind the scan.  An over-full pass ends in KNN_CTL_FALLBACK there (the overflow area's re-rank sees the count), not
// in the tail kernel's listed-pairs evaluation, which is a 1-NN fold.  Match-made lists only, one instantiation per shape (the
// inline re-rank's K has no meaning here): fp16 rows KT 1, KT 2 with and without NIF, each with both item deals, and the
// bin-frame 8-bit rows with the counter deal.  krt: the run-time k the bin-frame fill needs.  Block shapes and register caps
// are the 1-NN twins'.  (A kernel of its own name, not one more flag of knn_cells_scan_kernel: what tests/test_host_logic.py
// asserts of every scan kernel — v0 arithmetic inside, the counted end of the batch — is not true of this form by design.)
template <bool DYN, int KT = 1, bool NIF = false, bool U8 = false>
__global__ __launch_bounds__(64 * (KT == 1 ? CELL_SCAN_WAVES : CELL_SCAN_WAVES_KT2), KT == 1 ? 6 : 4) void knn_cells_records_kernel(
    const h8 *__restrict__ rf, const float *__restrict__ rn, const u64 *__restrict__ items, unsigned nitems,
    const h8 *__restrict__ qfg, const float *__restrict__ thrg, int m, int m_padded,
    const unsigned *__restrict__ cell_counts, const unsigned short *__restrict__ lists, unsigned cap,
    u64 *__restrict__ rec, unsigned *__restrict__ counts, unsigned *__restrict__ ctl, unsigned slice,
    unsigned ovf_base, unsigned ovf_cap, int krt, CellSelf self)
{
#pragma clang fp contract(off)
    constexpr bool TOPK = true, SELF = false, CTR = false;
    constexpr int K = 0;
    const float *const Q = nullptr;   // (read by the per-cell-frame fill only: a form this kernel does not have)
#define KNN_CELLS_SCAN_RECORD_ONLY   // the body without the 1-NN epilogue (inline re-rank, finalisation) and what only that reads
#include "knn_cells_scan_body.inc"
#undef KNN_CELLS_SCAN_RECORD_ONLY
}

// The record-only scan of a top-K pass on per-cell frames (KNN_QUERY_TOPK_FRAMES): the body with TOPK = true and CTR = true — the B
// operand and the threshold of a (query, cell) pair made from the fp32 query rows, the cell's frame and the prep kernel's
// Dup_(K) / sqrt(Dup_(K)), exactly as the 1-NN per-cell-frame scan makes them from its Dup.  fp16 rows with both item deals, the
// 8-bit per-cell rows with the counter deal; block shape and register cap of knn_cells_scan_kernel<DYN, 0, false, 1, true, false, U8>.
template <bool DYN, bool U8>
__global__ __launch_bounds__(64 * CELL_SCAN_WAVES_KT2, 4) void knn_cells_frame_records_kernel(
    const h8 *__restrict__ rf, const float *__restrict__ rn, const u64 *__restrict__ items, unsigned nitems,
    const h8 *__restrict__ qfg, const float *__restrict__ thrg, int m, int m_padded,
    const unsigned *__restrict__ cell_counts, const unsigned short *__restrict__ lists, unsigned cap,
    u64 *__restrict__ rec, unsigned *__restrict__ counts, unsigned *__restrict__ ctl, unsigned slice,
    unsigned ovf_base, unsigned ovf_cap, const float *__restrict__ Q, int krt, CellSelf self)
{
#pragma clang fp contract(off)
    constexpr bool TOPK = true, SELF = false, CTR = true, NIF = false;
    constexpr int K = 0, KT = 1;
#define KNN_CELLS_SCAN_RECORD_ONLY
#include "knn_cells_scan_body.inc"
#undef KNN_CELLS_SCAN_RECORD_ONLY
}

// What is left of a batch behind the scan, in ONE gated launch (rounds 2-3: a re-rank launch and two gated ones):
//   nothing (the usual case: the scan's last block has finalised the batch)     -> every block returns at once
//   records in the shared overflow area                                        -> re-ranked here, all blocks striding
//   the area over-full (a cluster tighter than the fp16 step: the fp16 scores do not separate the batch's rows)
//                                                                              -> the batch's listed (item, query) pairs
//                                                                                 with the exact arithmetic (cells_exact_items)
//   FALLBACK (a query nothing bounds)                                          -> K = 16: the exact scan of the whole shard,
//                                                                                 here (exact_qreg_body); other k: the gated
//                                                                                 exact launch in front of this one has run
//   fin.defer                                                                  -> only the finalisation
// KT (with K = 0): run-time k <= 16 KT
template <int K, int KT = 1>
__global__ __launch_bounds__(KNN_BLOCK) void knn_cells_tail_kernel(
    const float *__restrict__ Q, const float *__restrict__ R, int krt, int m, long long nrows, long long npos, long long base,
    const u64 *__restrict__ items, unsigned nitems, const unsigned *__restrict__ cell_counts,
    const unsigned short *__restrict__ lists, unsigned cap, const unsigned *__restrict__ perm,
    const u64 *__restrict__ rec, unsigned ovf_base, unsigned ovf_cap, unsigned *__restrict__ ctl, u64 *__restrict__ keys,
    CellFinal fin,
    // the scan's record lists (counts[nlists], `slice` records each): lists longer than CELL_INLINE_RERANK_MAX are re-ranked here
    const unsigned *__restrict__ counts, unsigned nlists, unsigned slice,
    CellSelf self)   // lo_t != null: the scan made its own lists; the exact evaluation of the listed pairs makes them again
{
#pragma clang fp contract(off)
    __shared__ unsigned short s_tail_list[KNN_WAVES][CELL_SELF_CAP];
    const unsigned fb = ctl[KNN_CTL_FALLBACK], have = ctl[KNN_CTL_RECORDS];   // final: prep and the scan are complete
    const unsigned deferred = ctl[KNN_CTL_DEFERRED];
    if (!fin.defer && fb == 0u && have == 0u && deferred == 0u)
        return;
    if (fb != 0u) {
        if constexpr (K == 16) {
            // a query nothing bounds (not finite, far outside the box): v0's arithmetic over the whole shard, 512 queries per
            // block (two per lane), slices of 1024 rows strided over the blocks
            const unsigned qgroups = ((unsigned)m + 511u) / 512u, gx = gridDim.x / qgroups;
            if (gx != 0u && blockIdx.x < gx * qgroups)
                exact_qreg_body<16, 1>(Q, R, m, nrows, base, keys, 1024ll, blockIdx.x / qgroups, gx, blockIdx.x % qgroups);
        }
    } else {
        if (have > ovf_cap) {
            if (blockIdx.x == 0 && threadIdx.x == 0)
                ctl[KNN_CTL_EXACT_CELLS] = 1u;   // (statistics: knn_index_last_stats[2] = 2)
            cells_exact_items<K, KT>(Q, R, krt, m, base, items, nitems, cell_counts, lists, cap, perm, keys,
                                 blockIdx.x * (unsigned)KNN_WAVES + (threadIdx.x >> 6), gridDim.x * (unsigned)KNN_WAVES, self,
                                 &s_tail_list[threadIdx.x >> 6][0]);
        } else {
          const int k = K > 0 ? K : krt;
          if (deferred != 0u) {   // the long lists the scan's waves left alone: a block per list, 16 lanes per record
            for (unsigned l = blockIdx.x; l < nlists; l += gridDim.x) {
                const unsigned n = min(counts[l], slice);   // block-uniform
                if (n <= CELL_INLINE_RERANK_MAX)
                    continue;
                const u64 *__restrict__ lr = rec + (size_t)l * slice;
                const unsigned pairs = n * 16u;
                const unsigned padded = (pairs + KNN_BLOCK - 1) / KNN_BLOCK * KNN_BLOCK;
                for (unsigned c = threadIdx.x; c < padded; c += KNN_BLOCK) {
                    u64 key = ~0ull;
                    unsigned qi = 0u;
                    if (c < pairs)
                        key = rerank_pair<K>(Q, R, k, npos, base, lr[c >> 4], c & 15u, 0xFFFFu, 0u, perm, qi);
#pragma unroll
                    for (int off = 8; off > 0; off >>= 1) {
                        const u64 o = __shfl_xor(key, off, KNN_WAVE);
                        key = o < key ? o : key;
                    }
                    if ((threadIdx.x & 15u) == 0u && key != ~0ull && key < keys[qi])
                        key_atomic_min(&keys[qi], key);
                }
            }
          }
          if (have != 0u) {
            const u64 *__restrict__ ovf = rec + ovf_base;
            const unsigned pairs = have * 16u;
            const unsigned padded = (pairs + KNN_BLOCK - 1) / KNN_BLOCK * KNN_BLOCK;
            for (unsigned c = blockIdx.x * KNN_BLOCK + threadIdx.x; c < padded; c += gridDim.x * KNN_BLOCK) {
                u64 key = ~0ull;
                unsigned qi = 0u;
                if (c < pairs)
                    key = rerank_pair<K>(Q, R, k, npos, base, ovf[c >> 4], c & 15u, 0xFFFFu, 0u, perm, qi);
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) {
                    const u64 o = __shfl_xor(key, off, KNN_WAVE);
                    key = o < key ? o : key;
                }
                if ((threadIdx.x & 15u) == 0u && key != ~0ull && key < keys[qi])
                    key_atomic_min(&keys[qi], key);
            }
          }
        }
    }
    if (!fin.gids && !fin.out_idx)
        return;
    __shared__ unsigned s_last;
    cells_wait_own_atomics();   // (as in the scan: this wave's atomics have been performed)
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(&ctl[KNN_CTL_TAIL_DONE], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (s_last != 0u)
        cells_finalize(keys, m, fin, threadIdx.x, KNN_BLOCK);
}

// ------------------------------------------------------------------------------------------
// Cell-range shards (round 4): the caller's partition pass, the replicated seed layer, the check of the rows' global numbers.
// ------------------------------------------------------------------------------------------
// owner[i] = the rank whose range of the global grid holds row i's cell
__global__ __launch_bounds__(256) void knn_geom_assign_kernel(const float *__restrict__ R, long long n, CellGeom g,
                                                              const float *__restrict__ bounds_arg, unsigned nranks,
                                                              int *__restrict__ owner)
{
    __shared__ float s_bnd[16 * (CELL_MAX_BINS - 1)];
    if (threadIdx.x < 16 * (CELL_MAX_BINS - 1))
        s_bnd[threadIdx.x] = bounds_arg[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    unsigned c = 0u;
    for (int d = 0; d < g.k; ++d)
        if (g.nb[d])
            c |= cell_bin(s_bnd + d * (CELL_MAX_BINS - 1), 1 << g.nb[d], R[(size_t)i * g.k + d]) << g.shift[d];
    owner[i] = (int)knn_shard_owner(c, g.ncells, nranks, 1u << g.sa);   // (one 64-bit division per row: a build-time pass)
}

// This rank's part of the seed layer: for every cell of its range the first T tiles of the cell-sorted layout (fragments
// and split norms; a cell of fewer tiles is padded with zero fragments and +INF norms, which never give a score).
// One block per cell.
__global__ __launch_bounds__(256) void knn_cells_seed_export_kernel(const unsigned *__restrict__ tile_start, unsigned ncells,
                                                                    unsigned cpr, unsigned T, const h8 *__restrict__ rf,
                                                                    const unsigned *__restrict__ rn2,
                                                                    unsigned char *__restrict__ part, float bmax, float nmax)
{
    const unsigned cell = blockIdx.x;   // < cpr
    h8 *__restrict__ of = (h8 *)(part + KNN_SEED_HEADER_BYTES + (size_t)cell * T * 1024u);
    unsigned *__restrict__ on = (unsigned *)(part + KNN_SEED_HEADER_BYTES + (size_t)cpr * T * 1024u + (size_t)cell * T * 128u);
    unsigned tb = 0u, nt = 0u;
    if (cell < ncells) {
        tb = tile_start[cell];
        nt = min(T, tile_start[cell + 1u] - tb);
    }
    for (unsigned i = threadIdx.x; i < T * 64u; i += 256u)
        of[i] = i < nt * 64u ? rf[(size_t)tb * 64 + i] : (h8){0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned i = threadIdx.x; i < T * 32u; i += 256u)
        on[i] = i < nt * 32u ? rn2[(size_t)tb * 32 + i] : 0x00007C00u;
    if (cell == 0u && threadIdx.x == 0) {   // header: what the bound constants of every rank must cover
        ((float *)part)[0] = bmax;
        ((float *)part)[1] = nmax;
    }
}

__global__ __launch_bounds__(256) void knn_gids_check_kernel(const unsigned *__restrict__ gids, long long n, unsigned *__restrict__ bad)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += stride)
        if (!(gids[i] < gids[i + 1]))
            atomicAdd(bad, 1u);
}

hipError_t knn_geom_assign_launch(const ShardGeom &sg, const float *rows_dev, long long n, int *owner_dev, hipStream_t s)
{
    if (n <= 0)
        return hipSuccess;
    CellGeom g;
    memset(&g, 0, sizeof g);
    g.k = sg.k;
    g.bits = sg.bits;
    g.sa = sg.sa;
    memcpy(g.nb, sg.nb, 16);
    memcpy(g.shift, sg.shift, 16);
    g.ncells = sg.ncells;
    float *bnd = nullptr;
    FTRY(KNN_DEV_ALLOC((void **)&bnd, sizeof sg.bounds));
    hipError_t e = hipMemcpyAsync(bnd, sg.bounds, sizeof sg.bounds, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(knn_geom_assign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows_dev, n, g, bnd,
                           (unsigned)sg.nranks, owner_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);   // (the cuts' staging buffer goes back to the pool)
    (void)KNN_DEV_FREE(bnd);
    return e;
}

hipError_t knn_cells_seed_export(const FilterState &st, int rank, unsigned char *layer_dev, hipStream_t s)
{
    if (!st.cells || !st.cells->geom || !layer_dev)
        return hipErrorInvalidValue;
    const ShardGeom &sg = *st.cells->geom;
    hipLaunchKernelGGL(knn_cells_seed_export_kernel, dim3(sg.cells_per_rank), dim3(256), 0, s, st.cells->tile_start, st.cells->ncells,
                       sg.cells_per_rank, (unsigned)sg.seed_tiles, (const h8 *)st.ref_frags, st.ref_norms2,
                       layer_dev + (size_t)rank * sg.part_bytes(), st.bmax, st.nmax);
    return hipGetLastError();
}

hipError_t knn_gids_check(const unsigned *gids_dev, long long n, unsigned *bad_out, hipStream_t s)
{
    *bad_out = 0u;
    if (n < 2)
        return hipSuccess;
    unsigned *bad = nullptr;
    FTRY(KNN_DEV_ALLOC((void **)&bad, sizeof(unsigned)));
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(unsigned), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(knn_gids_check_kernel, dim3(1024), dim3(256), 0, s, gids_dev, n, bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(bad_out, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void)KNN_DEV_FREE(bad);
    return e;
}

// The global grid of a cell-range sharded set.  bits: as many as the rows allow (>= 144 rows per cell on average, the
// rule of a single index), at most 4 per dimension, and no more than lets every rank hold <= 2^16 cells; every rank's range
// starts at a multiple of 2^sa codes (whole entries of the high pruning table; 2^sa >= 64: whole blocks of the match pass).
bool knn_geom_cells(ShardGeom &g, int k, long long n_global, int nranks, const float *sample, long long samples, int seed_tiles)
{
    if (k < 1 || k > 16 || nranks < 1 || nranks > 64 || samples < 64 || seed_tiles < 1 || seed_tiles > 8 || n_global < 1)
        return false;
    int bits = std::min(cell_bits_for_rows(n_global), 4 * k);
    while (bits > 0 && ((1ull << bits) + (unsigned long long)nranks - 1ull) / (unsigned long long)nranks > 65536ull)
        --bits;
    if (bits < 9)
        return false;
    g.k = k;
    g.bits = bits;
    g.nranks = nranks;
    g.seed_tiles = seed_tiles;
    g.n_global = n_global;
    g.ncells = 1u << bits;
    cell_grid_shape(k, bits, g.nb, g.shift, &g.sa);
    if (g.sa < 6)
        return false;
    g.cells_per_rank = 0u;
    for (int r = 0; r < nranks; ++r) {   // every rank needs a layout of its own, of at most 2^16 cells
        const unsigned cr = g.cells_of(r);
        if (cr < 512u || cr > 65536u || cr % 64u != 0u)
            return false;
        g.cells_per_rank = std::max(g.cells_per_rank, cr);
    }
    cell_quantile_cuts(k, g.nb, sample, samples, g.bounds);
    return true;
}


// ------------------------------------------------------------------------------------------
// Per-cell frames (round 5; VERDICT r03 / r04: "centre fragments on their cell's box").  The shard's ONE frame rounds a
// coordinate to fp16 with an error of 2^-12 of the box; where the rows of a cell sit in a thousandth of the box (clustered
// data: 64 clusters of width 10^-3 — tools/distribution_check.py) that error is a quarter of the cluster's width, the
// thresholds admit most of the cluster (2 200 candidates per query) and the batch ends in the exact evaluation of its listed
// pairs.  In a frame of the CELL — fragment = fp16((row - centre_c) x scale_c), scale_c = sigma 2^e <= 2^8 sigma so that the
// cell's rows fill [-1, 1] — the same rounding is 2^-12 of the cell, and everything knn_filter_dev.h derives for (centre,
// sigma) holds for (centre_c, scale_c) word for word: the B operand of a (query, cell) pair is the query in THAT frame
// (built by the scan's lanes from the fp32 query, which the block keeps in LDS: knn_cells_scan_kernel<CTR>), its threshold comes from Dup_q — a squared
// DISTANCE, frame-free up to the power-of-two ratio — and the pair's own amax, the cell's bmax and nmax.
// Built as a pass over the finished cell-sorted layout (rows gathered through perm: ~3 ms per 2^24 rows — taken only when the
// build's sample says the data is clustered, or on request: knn_cells_recentre).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_cells_tile_cell_kernel(const unsigned *__restrict__ tile_start, unsigned ncells,
                                                                  unsigned *__restrict__ tile_cell)
{
    // 32 threads per cell (a cell of a clustered set can hold thousands of tiles)
    const unsigned c = (blockIdx.x * blockDim.x + threadIdx.x) >> 5, j = threadIdx.x & 31u;
    if (c >= ncells)
        return;
    for (unsigned t = tile_start[c] + j; t < tile_start[c + 1u]; t += 32u)
        tile_cell[t] = c;
}

// box[c][0..15] = min, box[c][16..31] = max of the cell's rows (ordered-uint images; rows outside the robust box — +INF norm —
// and padding positions do not count).  One wave per run of CELL_BOX_RUN consecutive tiles, lane = (row, half of the
// dimensions): the lanes keep their own minima while the run stays in one cell (tiles are in cell order) and fold them — 5
// shuffle steps, 16 guarded atomics per half — when the cell changes or the run ends.  (One wave per tile, folding every tile:
// 4.0 ms for the 131 072 tiles of 64 clusters — 32 atomics per tile on 64 cells' words; this form 0.2 ms.)
#define CELL_BOX_RUN 32u
__global__ __launch_bounds__(256) void knn_cells_box_kernel(const float *__restrict__ R, int k, const unsigned *__restrict__ perm,
                                                            const float *__restrict__ norms, unsigned ntiles,
                                                            const unsigned *__restrict__ tile_cell, unsigned *__restrict__ box)
{
    const unsigned t0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * CELL_BOX_RUN;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    if (t0 >= ntiles)
        return;
    const unsigned t1 = min(t0 + CELL_BOX_RUN, ntiles);
    float lo[8], hi[8];
    auto reset = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            lo[j] = INFINITY;
            hi[j] = -INFINITY;
        }
    };
    auto fold = [&](unsigned cell) {
#pragma unroll
        for (int off = 16; off > 0; off >>= 1)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lo[j] = fminf(lo[j], __shfl_xor(lo[j], off, KNN_WAVE));
                hi[j] = fmaxf(hi[j], __shfl_xor(hi[j], off, KNN_WAVE));
            }
        if ((lane & 31) == 0) {
            unsigned *__restrict__ b = box + (size_t)cell * 32;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (lo[j] < INFINITY)
                    guarded_atomic_min(&b[8 * half + j], f2ord(lo[j]));
                if (hi[j] > -INFINITY)
                    guarded_atomic_max(&b[16 + 8 * half + j], f2ord(hi[j]));
            }
        }
    };
    reset();
    unsigned cur = tile_cell[t0];
    for (unsigned t = t0; t < t1; ++t) {
        const unsigned cell = tile_cell[t];   // wave-uniform
        if (cell != cur) {
            fold(cur);
            reset();
            cur = cell;
        }
        const size_t pos = (size_t)t * 32 + (lane & 31);
        const unsigned row = perm[pos];
        if (row != 0xFFFFFFFFu && norms[pos] < INFINITY) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (8 * half + j < k) {
                    const float x = R[(size_t)row * k + 8 * half + j];
                    lo[j] = fminf(lo[j], x);
                    hi[j] = fmaxf(hi[j], x);
                }
        }
    }
    fold(cur);
}

// frame[c] = { centre[16], scale, 2^e, 0 (bmax), 0 (nmax) }: the centre is the middle of the cell's box, e the largest
// exponent <= 8 for which the box, scaled, stays inside [-1, 1]
__global__ __launch_bounds__(256) void knn_cells_frame_kernel(const unsigned *__restrict__ box, unsigned ncells, int k, float sigma,
                                                              float *__restrict__ frame)
{
    const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells)
        return;
    float *__restrict__ f = frame + (size_t)c * KNN_CELL_FRAME_WORDS;
    float hw = 0.0f;
    for (int d = 0; d < 16; ++d) {
        float ctr = 0.0f;
        if (d < k && box[(size_t)c * 32 + d] <= box[(size_t)c * 32 + 16 + d]) {   // (min <= max: the cell has a row)
            const float lo = ord2f(box[(size_t)c * 32 + d]), hi = ord2f(box[(size_t)c * 32 + 16 + d]);
            ctr = 0.5f * lo + 0.5f * hi;
            hw = fmaxf(hw, fmaxf(hi - ctr, ctr - lo));
        }
        f[d] = ctr;
    }
    float ratio = 1.0f;
    for (int e = 0; e < 8 && hw * sigma * (2.0f * ratio) <= 0.999f; ++e)
        ratio *= 2.0f;
    f[16] = sigma * ratio;
    f[17] = ratio;
    f[18] = 0.0f;
    f[19] = 0.0f;
}

// With rows8 (option `cells_rows`): every row also as one byte per coordinate in its cell's frame, for the scan alone (the prep
// kernel's seeds keep reading the fp16 fragments).  v = (row - centre_c) x scale_c is the fp32 value the fragment rounds to fp16 (fp32 subtract, exact power-of-two scale: |v - v_exact| <= 2^-24 |v_exact|), and it
// is rounded ONCE: code = 128 + clamp(rint(128 v), -128, 127), so the row the scan scores is r^ = (code - 128) / 128 — a
// multiple of 2^-7 in [-1, 127/128], exact in fp16.  Per coordinate |v_exact - r^| <= |v - r^| + 2^-23 |v|, at most 2^-8 + 2^-23
// inside the cell's box (|v| <= 1), 2^-7 where the clamp bites; cell_u8[c][0] holds the cell's largest err of knn_u8_code
// (|v - r^| + 2^-22 |v| + 2^-100, rounded: the scan takes it 10^-6 larger), the row error knn_bound_consts_u8 starts from.  norms8 =
// |r^|^2, exact in fp32 (16 multiples of 2^-14 below 1); cell_u8[c][1] its largest value in the cell.  Padding rows and rows
// outside the shard's robust box: code 128 (r^ = 0) and norm +INF, as in the fp16 layout.  Lane order: the fragments'.
// The fragments, norms and norm halves of every tile again, in its cell's frame; frame[c][18] / [19] = the cell's largest
// |coordinate| and norm.  Same arithmetic as the placement (fp32 subtract, exact power-of-two scale, round to nearest even,
// exact products summed in fp32), same rule for rows outside the shard's robust box (they stay out: zero fragment, +INF norm).
__global__ __launch_bounds__(256) void knn_cells_recentre_kernel(const float *__restrict__ R, int k, const unsigned *__restrict__ perm,
                                                                 unsigned ntiles, const unsigned *__restrict__ tile_cell,
                                                                 float *__restrict__ frame, h8 *__restrict__ frag,
                                                                 float *__restrict__ norms, unsigned *__restrict__ norms2,
                                                                 u2v *__restrict__ rows8, float *__restrict__ norms8, float *__restrict__ cell_u8)
{
    const unsigned t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    if (t >= ntiles)
        return;
    const size_t pos = (size_t)t * 32 + (lane & 31);
    const unsigned row = perm[pos];
    const bool real = row != 0xFFFFFFFFu && norms[pos] < INFINITY;
    float *__restrict__ f = frame + (size_t)tile_cell[t] * KNN_CELL_FRAME_WORDS;
    const float scale = f[16];
    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    float vmax = 0.0f, part = 0.0f;
    u2v code = {0x80808080u, 0x80808080u};   // 8-bit rows (rows8 != null): see above — the same v, rounded once more
    float err8 = 0.0f, part8 = 0.0f;
    if (real) {
        code = (u2v){0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = 8 * half + j;
            const float sc = d < k ? (R[(size_t)row * k + d] - f[d]) * scale : 0.0f;
            const _Float16 hval = (_Float16)sc;
            const float back = (float)hval;
            vmax = fmaxf(vmax, fabsf(back));
            part = part + back * back;
            v[j] = hval;
            float rh, e;
            const unsigned b = knn_u8_code(sc, rh, e);
            err8 = fmaxf(err8, e);
            part8 = part8 + rh * rh;   // exact
            code[j >> 2] |= b << (8 * (j & 3));
        }
    }
    if (rows8) {   // (kernel-uniform) the 8-bit rows from the same gather of the rows
        const float other8 = __shfl_xor(part8, 32, KNN_WAVE);
        const float nrm8 = half == 0 ? part8 + other8 : other8 + part8;
        rows8[(size_t)t * 64 + lane] = code;
        if (half == 0)
            norms8[pos] = real ? nrm8 : INFINITY;
        err8 = wave_max_f(err8);
        const float nmax8 = wave_max_f(real ? nrm8 : 0.0f);
        if (lane == 0) {
            guarded_atomic_max((unsigned *)&cell_u8[(size_t)tile_cell[t] * 2], __float_as_uint(err8));
            guarded_atomic_max((unsigned *)&cell_u8[(size_t)tile_cell[t] * 2 + 1], __float_as_uint(nmax8));
        }
    }
    const float other = __shfl_xor(part, 32, KNN_WAVE);
    const float nrm = half == 0 ? part + other : other + part;   // (dimensions 0..7) + (dimensions 8..15) on both lanes of a row
    frag[(size_t)t * 64 + lane] = v;
    if (half == 0) {
        norms[pos] = real ? nrm : INFINITY;
        norms2[pos] = pack_norm22(real ? nrm : INFINITY);
    }
    vmax = wave_max_f(vmax);
    const float nmaxv = wave_max_f(real ? nrm : 0.0f);
    if (lane == 0) {
        guarded_atomic_max((unsigned *)&f[18], __float_as_uint(vmax));
        guarded_atomic_max((unsigned *)&f[19], __float_as_uint(nmaxv));
    }
}

// With bin frames (option `cells_u8_frame`): every row as one byte per coordinate, the offset from its cell's w_c at the shard's
// scale sigma 2^e (knn_u8_bin_code; the derivation is beside it in knn_filter_dev.h).  The fp16 fragments, norms and norm halves
// are not touched: they stay in the shard's one frame for the prep kernel's seeds.  norms8 = N'' = |w_c + r^|^2, summed in
// double (every term exact) and rounded once; cell_u8[0] / [1] = the shard's largest err / N''.  Padding rows and rows outside
// the shard's robust box: code 128 and norm +INF, as in the fp16 layout.  Lane order: the fragments'.
__global__ __launch_bounds__(256) void knn_cells_bin_rows_kernel(const float *__restrict__ R, int k, const unsigned *__restrict__ perm,
                                                                 const float *__restrict__ norms, unsigned ntiles,
                                                                 const unsigned *__restrict__ tile_cell, const float *__restrict__ center,
                                                                 float scale, const h8 *__restrict__ binw, u2v *__restrict__ rows8,
                                                                 float *__restrict__ norms8, float *__restrict__ cell_u8)
{
    const unsigned t = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63, half = lane >> 5;
    if (t >= ntiles)
        return;
    const size_t pos = (size_t)t * 32 + (lane & 31);
    const unsigned row = perm[pos];
    const bool real = row != 0xFFFFFFFFu && norms[pos] < INFINITY;
    const h8 w = binw[(size_t)tile_cell[t] * 2 + half];
    u2v code = {0x80808080u, 0x80808080u};
    float err8 = 0.0f;
    double part = 0.0;
    if (real) {
        code = (u2v){0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = 8 * half + j;
            float rh = 0.0f, e = 0.0f;
            unsigned b = 128u;
            if (d < k)
                b = knn_u8_bin_code(R[(size_t)row * k + d], center[d], scale, (float)w[j], rh, e);
            err8 = fmaxf(err8, e);
            const double f = (double)w[j] + (double)rh;   // (0 beyond k: w and r^ are)
            part = part + f * f;
            code[j >> 2] |= b << (8 * (j & 3));
        }
    }
    const double other = __shfl_xor(part, 32, KNN_WAVE);
    const float nrm = (float)(part + other);   // (the same sum on both lanes of a row)
    rows8[(size_t)t * 64 + lane] = code;
    if (half == 0)
        norms8[pos] = real ? nrm : INFINITY;
    err8 = wave_max_f(err8);
    const float nmax8 = wave_max_f(real ? nrm : 0.0f);
    if (lane == 0) {
        guarded_atomic_max((unsigned *)&cell_u8[0], __float_as_uint(err8));
        guarded_atomic_max((unsigned *)&cell_u8[1], __float_as_uint(nmax8));
    }
}

// ------------------------------------------------------------------------------------------
// Host side.
// ------------------------------------------------------------------------------------------
void knn_cells_free(CellIndex *&c)
{
    if (!c)
        return;
    (void)KNN_DEV_FREE(c->bounds);
    (void)KNN_DEV_FREE(c->tile_start);
    (void)KNN_DEV_FREE(c->perm);
    (void)KNN_DEV_FREE(c->items);
    knn_cells_release_build_scratch(*c);
    (void)KNN_DEV_FREE(c->cell_frame);
    (void)KNN_DEV_FREE(c->tile_cell);
    (void)KNN_DEV_FREE(c->rows8);
    (void)KNN_DEV_FREE(c->norms8);
    (void)KNN_DEV_FREE(c->cell_u8);
    (void)KNN_DEV_FREE(c->binw);
    delete c;
    c = nullptr;
}

std::atomic<int> g_knn_cells_centre{0};                 // option `cells_centre`
std::atomic<long long> g_knn_cells_centred_builds{0};   // read-only option `cells_centred_builds`
std::atomic<int> g_knn_cells_rows{0};                   // option `cells_rows`
std::atomic<long long> g_knn_cells_u8_builds{0};        // read-only option `cells_u8_builds`
std::atomic<int> g_knn_cells_u8_frame{0};               // option `cells_u8_frame`
std::atomic<long long> g_knn_cells_u8_bin_builds{0};    // read-only option `cells_u8_bin_builds`

// The 8-bit rows in per-dimension bin frames (knn_filter_dev.h, knn_u8_bin_code), from the finished cells' boxes (`box`, host
// copy `hb`).  Auto (forced = false) takes them where the bins fit the cells: for >= 95 % of the (non-empty cell, cut dimension)
// pairs the bin's extent is at most twice the cell's own — uniform-like rows (a cell fills its orthant); clustered rows, whose
// cells hold a sliver of their bins, keep per-cell frames.  -> *done: the layout has them.  Enqueues on `s` and synchronises.
static hipError_t knn_cells_bin_frame(FilterState &st, const float *r, const std::vector<unsigned> &hb, hipStream_t s, bool forced, bool *done)
{
    *done = false;
    CellIndex &c = *st.cells;
    const int k = st.k;
    float ctr[16] = {0};
    FTRY(hipMemcpyAsync(ctr, st.center, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, s));
    FTRY(hipStreamSynchronize(s));
    auto bin_of = [&](unsigned cell, int d) { return c.nb[d] ? (cell >> c.shift[d]) & ((1u << c.nb[d]) - 1u) : 0u; };
    auto filled = [&](unsigned cell, int d) { return hb[(size_t)cell * 32 + d] <= hb[(size_t)cell * 32 + 16 + d]; };
    double blo[16][CELL_MAX_BINS], bhi[16][CELL_MAX_BINS];
    for (int d = 0; d < 16; ++d)
        for (int b = 0; b < CELL_MAX_BINS; ++b) {
            blo[d][b] = INFINITY;
            bhi[d][b] = -INFINITY;
        }
    for (unsigned cell = 0; cell < c.ncells; ++cell)
        for (int d = 0; d < k; ++d)
            if (filled(cell, d)) {
                const unsigned b = bin_of(cell, d);
                blo[d][b] = std::min(blo[d][b], (double)ord2f_host(hb[(size_t)cell * 32 + d]));
                bhi[d][b] = std::max(bhi[d][b], (double)ord2f_host(hb[(size_t)cell * 32 + 16 + d]));
            }
    if (!forced) {
        size_t pairs = 0, fit = 0;
        for (unsigned cell = 0; cell < c.ncells; ++cell)
            for (int d = 0; d < k; ++d)
                if (c.nb[d] && filled(cell, d)) {
                    const unsigned b = bin_of(cell, d);
                    const double cw = (double)ord2f_host(hb[(size_t)cell * 32 + 16 + d]) - (double)ord2f_host(hb[(size_t)cell * 32 + d]);
                    ++pairs;
                    fit += bhi[d][b] - blo[d][b] <= 2.0 * cw ? 1u : 0u;
                }
        if (pairs == 0 || (double)fit < 0.95 * (double)pairs)
            return hipSuccess;
    }
    // the scale: the widest bin's half-extent, in sigma units, fills [-1, 1] up to the 2^-7 the offsets' rounding moves a centre
    double hw = 0.0;
    for (int d = 0; d < k; ++d)
        for (int b = 0; b < CELL_MAX_BINS; ++b)
            if (blo[d][b] <= bhi[d][b])
                hw = std::max(hw, 0.5 * (bhi[d][b] - blo[d][b]) * (double)st.sigma);
    int e = 0;
    while (e < 4 && hw * std::ldexp(1.0, e + 1) + 0x1p-7 <= 1.0)
        ++e;
    const float ratio = std::ldexp(1.0f, e), scale = st.sigma * ratio;
    float wt[16][CELL_MAX_BINS];
    for (int d = 0; d < 16; ++d)
        for (int b = 0; b < CELL_MAX_BINS; ++b) {
            wt[d][b] = 0.0f;
            if (d < k && blo[d][b] <= bhi[d][b]) {
                const double o = 0.5 * (blo[d][b] + bhi[d][b]);
                const double w = std::rint((o - (double)ctr[d]) * (double)scale * 64.0) / 64.0;
                if (!(std::fabs(w) < 32.0))
                    return hipSuccess;   // (not an fp16 number of <= 11 bits: keep per-cell frames)
                wt[d][b] = (float)w;
            }
        }
    std::vector<_Float16> hw16((size_t)c.ncells * 16);
    double w1 = 0.0;
    for (unsigned cell = 0; cell < c.ncells; ++cell) {
        double sum = 0.0;
        for (int d = 0; d < 16; ++d) {
            const float w = d < k ? wt[d][bin_of(cell, d)] : 0.0f;
            hw16[(size_t)cell * 16 + d] = (_Float16)w;   // exact
            sum += std::fabs((double)w);
        }
        w1 = std::max(w1, sum);
    }
    FTRY(KNN_DEV_ALLOC(&c.binw, hw16.size() * sizeof(_Float16)));
    FTRY(hipMemcpyAsync(c.binw, hw16.data(), hw16.size() * sizeof(_Float16), hipMemcpyHostToDevice, s));
    FTRY(hipMemsetAsync(c.cell_u8, 0, 2 * sizeof(float), s));
    const unsigned ntiles = (unsigned)st.ntiles;
    hipLaunchKernelGGL(knn_cells_bin_rows_kernel, dim3((ntiles + 3u) / 4u), dim3(256), 0, s, r, k, c.perm, st.ref_norms, ntiles, c.tile_cell,
                       st.center, scale, (const h8 *)c.binw, (u2v *)c.rows8, c.norms8, c.cell_u8);
    FTRY(hipGetLastError());
    float mx[2];
    FTRY(hipMemcpyAsync(mx, c.cell_u8, sizeof mx, hipMemcpyDeviceToHost, s));
    FTRY(hipStreamSynchronize(s));   // (hw16 and mx are on this stack)
    c.bin_ratio = ratio;
    c.bin_er = mx[0];
    c.bin_nmax = mx[1];
    c.bin_w1 = (float)(w1 * (1.0 + 1e-6));
    c.bins = true;
    *done = true;
    return hipSuccess;
}

// Moves a finished cell-sorted layout (k <= 16, no shard geometry) into per-cell frames — see the kernels — or, for 8-bit rows
// in bin frames, leaves it in the shard's frame and adds the rows (knn_cells_bin_frame).  Enqueues on `s`; the caller's next
// synchronisation covers it.
hipError_t knn_cells_recentre(FilterState &st, const float *r, hipStream_t s, bool rows_u8, bool frames_wanted)
{
    if (!st.cells || st.kt != 1 || st.cells->geom || st.cells->centred || st.cells->rows_u8)
        return hipSuccess;
    CellIndex &c = *st.cells;
    const unsigned ntiles = (unsigned)st.ntiles;
    unsigned *box = nullptr;
    if (rows_u8 && ntiles != 0u) {   // 8-bit rows for the scan (the fp16 fragments stay: the prep kernel's seeds)
        hipError_t e8 = KNN_DEV_ALLOC((void **)&c.rows8, (size_t)ntiles * 64 * 8);
        if (e8 == hipSuccess)
            e8 = KNN_DEV_ALLOC((void **)&c.norms8, (size_t)ntiles * 32 * sizeof(float));
        if (e8 == hipSuccess)
            e8 = KNN_DEV_ALLOC((void **)&c.cell_u8, (size_t)c.ncells * 2 * sizeof(float));
        if (e8 == hipSuccess)
            e8 = hipMemsetAsync(c.cell_u8, 0, (size_t)c.ncells * 2 * sizeof(float), s);
        if (e8 != hipSuccess) {   // no room: per-cell frames only if they were asked for on their own, else the shard's one frame
            (void)KNN_DEV_FREE(c.rows8);
            (void)KNN_DEV_FREE(c.norms8);
            (void)KNN_DEV_FREE(c.cell_u8);
            c.rows8 = nullptr;
            c.norms8 = c.cell_u8 = nullptr;
            (void)hipGetLastError();
            if (!frames_wanted)
                return hipSuccess;
        }
    }
    FTRY(KNN_DEV_ALLOC((void **)&c.tile_cell, (size_t)std::max(1u, ntiles) * sizeof(unsigned)));
    FTRY(KNN_DEV_ALLOC((void **)&box, (size_t)c.ncells * 32 * sizeof(unsigned)));
    hipError_t e = hipMemsetAsync(box, 0xFF, (size_t)c.ncells * 32 * sizeof(unsigned), s);   // min = ~0; max: cleared below
    if (e == hipSuccess)
        e = hipMemset2DAsync(box + 16, 32 * sizeof(unsigned), 0, 16 * sizeof(unsigned), c.ncells, s);
    if (e == hipSuccess && ntiles != 0u) {
        hipLaunchKernelGGL(knn_cells_tile_cell_kernel, dim3((c.ncells * 32u + 255u) / 256u), dim3(256), 0, s, c.tile_start, c.ncells, c.tile_cell);
        hipLaunchKernelGGL(knn_cells_box_kernel, dim3(((ntiles + CELL_BOX_RUN - 1u) / CELL_BOX_RUN + 3u) / 4u), dim3(256), 0, s, r, st.k, c.perm, st.ref_norms,
                           ntiles, c.tile_cell, box);
        e = hipGetLastError();
    }
    // Which frame the 8-bit rows get (option `cells_u8_frame`: 0 auto, 1 per-cell, 2 per-bin): per-bin where asked for, or — auto,
    // unless per-cell frames are wanted on their own (clustered data) — where the bins fit the cells (knn_cells_bin_frame)
    const int fopt = g_knn_cells_u8_frame;
    if (e == hipSuccess && c.rows8 && ntiles != 0u && (fopt == 2 || (fopt == 0 && !frames_wanted))) {
        std::vector<unsigned> hb((size_t)c.ncells * 32);
        e = hipMemcpyAsync(hb.data(), box, hb.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        bool done = false;
        if (e == hipSuccess)
            e = knn_cells_bin_frame(st, r, hb, s, fopt == 2, &done);
        if (e == hipSuccess && done) {
            (void)KNN_DEV_FREE(box);
            c.rows_u8 = true;
            ++g_knn_cells_u8_builds;
            ++g_knn_cells_u8_bin_builds;
            return hipSuccess;
        }
    }
    if (e == hipSuccess)
        e = KNN_DEV_ALLOC((void **)&c.cell_frame, (size_t)c.ncells * KNN_CELL_FRAME_WORDS * sizeof(float));
    if (e == hipSuccess && ntiles != 0u) {
        hipLaunchKernelGGL(knn_cells_frame_kernel, dim3((c.ncells + 255u) / 256u), dim3(256), 0, s, box, c.ncells, st.k, st.sigma, c.cell_frame);
        hipLaunchKernelGGL(knn_cells_recentre_kernel, dim3((ntiles + 3u) / 4u), dim3(256), 0, s, r, st.k, c.perm, ntiles, c.tile_cell,
                           c.cell_frame, (h8 *)st.ref_frags, st.ref_norms, st.ref_norms2, (u2v *)c.rows8, c.norms8, c.cell_u8);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);   // (box is scratch)
    (void)KNN_DEV_FREE(box);
    FTRY(e);
    c.centred = true;
    ++g_knn_cells_centred_builds;
    if (c.rows8) {
        c.rows_u8 = true;
        ++g_knn_cells_u8_builds;
    }
    return hipSuccess;
}

// What the builds call once a cell-sorted layout stands: per-cell frames when option `cells_centre` asks for them (1), or
// (0) when the build's host sample looks clustered.  samp may be null (no sample at hand: only on request).
hipError_t knn_cells_maybe_recentre(FilterState &st, const float *r, const float *samp, long long samples, hipStream_t s)
{
    if (!st.usable || !st.cells || st.kt != 1 || st.cells->geom)
        return hipSuccess;
    const int opt = g_knn_cells_centre, rows = g_knn_cells_rows;
    const bool clustered = samp && knn_cells_sample_is_clustered(samp, samples, st.k, st.sigma);
    // 8-bit rows (they need per-cell frames): on request, or — library policy — for shards of >= 2^24 rows whose sample is
    // uniform-like (profiles/r06_u8_rows.txt, one batch at a time, fp16 -> u8 ms: uniform 2^24 0.153 -> 0.149 (C3 pipelined -6 %,
    // C4 -25 %); uniform 2^22 0.080 -> 0.094, gaussian 2^24 0.187 -> 0.219, unit sphere 0.166 -> 0.199, heavy tails 0.365 ->
    // 0.368: where the lists are long the per-pair operand work of the per-cell-frame scan costs more than the bytes save)
    const bool rows_u8 = rows == 2 || (rows == 0 && opt != 2 && !clustered && st.n >= (1ll << 24) && samp &&
                                       knn_cells_sample_is_uniform_like(samp, samples, st.k));
    const bool frames = opt == 1 || (opt == 0 && clustered);
    if (!rows_u8 && !frames)
        return hipSuccess;
    return knn_cells_recentre(st, r, s, rows_u8, frames);
}

// Is the build's host sample uniform-like?  Per dimension, the inter-quartile range against the 1st..99th percentile range:
// 0.5 for uniform rows (and for uniform integer codes), 0.29 for gaussian, less for heavy tails; the mean over the dimensions
// must reach 0.4.  Where the rows are spread evenly the cells' lists are short and the 8-bit rows' bytes are what counts.
bool knn_cells_sample_is_uniform_like(const float *samp, long long samples, int k)
{
    if (samples < 256 || k < 1)
        return false;
    std::vector<float> col((size_t)samples);
    double sum = 0.0;
    for (int d = 0; d < k; ++d) {
        for (long long i = 0; i < samples; ++i)
            col[(size_t)i] = samp[(size_t)i * k + d];
        auto at = [&](double f) {
            const size_t j = (size_t)(f * (double)(samples - 1));
            std::nth_element(col.begin(), col.begin() + j, col.end());
            return (double)col[j];
        };
        const double p01 = at(0.01), p25 = at(0.25), p75 = at(0.75), p99 = at(0.99);
        if (!(p99 > p01))
            return false;
        sum += (p75 - p25) / (p99 - p01);
    }
    return sum / k >= 0.4;
}

// Does the build's host sample look clustered?  Median, over 64 sample rows, of the distance (largest coordinate difference)
// to the nearest of up to 256 other sample rows, in units of the frame's box (scaled: the box is [-1, 1]): uniform or gaussian
// data in 16 dimensions ~0.5-1, 1000 blobs of 0.05 of the box likewise (the sample's neighbours are in other blobs), 64
// clusters of 10^-3 of the box 0.007.  Below 1/16 the per-cell frames pay for their pass over the rows.  (0.05 ms of host
// arithmetic in every build of a cell-sorted layout.)
bool knn_cells_sample_is_clustered(const float *samp, long long samples, int k, float sigma)
{
    const long long cand = std::min<long long>(samples, 256), step = cand > 0 ? samples / cand : 1, probes = std::min<long long>(cand, 64);
    if (cand < 32)
        return false;
    std::vector<float> nn((size_t)probes, INFINITY);
    for (long long i = 0; i < probes; ++i) {
        const float *a = samp + (size_t)(i * (cand / probes) * step) * k;
        for (long long j = 0; j < cand; ++j) {
            const float *b = samp + (size_t)(j * step) * k;
            if (a == b)
                continue;
            float dmax = 0.0f;
            for (int d = 0; d < k; ++d)
                dmax = std::max(dmax, fabsf(a[d] - b[d]));
            if (!(dmax == dmax))
                return false;
            nn[(size_t)i] = std::min(nn[(size_t)i], dmax);
        }
    }
    std::nth_element(nn.begin(), nn.begin() + probes / 2, nn.end());
    return nn[(size_t)(probes / 2)] * sigma < 1.0f / 16.0f;
}

// ---- the build --------------------------------------------------------------------------------
// A cell-sorted layout is built in four steps: the grid (knn_cells_plan: host arithmetic), the strategy
// (knn_cells_first_build, then knn_cells_next_build), the staging of the rows into cells (knn_cells_stage: codes, counts or
// buckets, tile ranges, items) and the finish (knn_filter.hip: layouts, placement, ONE synchronisation, accept or reject).

// The grid of the shard's cell-sorted layout (see the head of this file): shape, cuts (h_bounds), list capacity and lbits.
// geom != null: the cell-range shard `rank` of that global grid (no cuts of its own).  samp: the strided host sample of the
// build (samples x k).  False when the shard is too small, the dimension does not suit, or the grid would be too coarse.
bool knn_cells_plan(CellIndex &c, int k, long long n, const float *samp, long long samples, const ShardGeom *geom, int rank)
{
    c = CellIndex();
    // (16 < k <= 32, round 5: the cells cut the first 16 dimensions — a lower bound over some dimensions is one over all —
    // and the layout has two K-steps per tile; one-pass placement, no shard geometry)
    if (k > 32 || (k > 16 && geom) || n > 0x7FFFFFFFll || (!geom && (n < (1ll << 17) || samples < 64)))
        return false;
    static_assert(sizeof c.h_bounds == 16 * (CELL_MAX_BINS - 1) * sizeof(float) && sizeof c.h_bounds == sizeof geom->bounds, "cuts");
    if (geom) {
        // cell-range shard: the global grid's shape and cuts, this rank's range of its codes
        c.bits = geom->bits;
        c.sa = geom->sa;
        memcpy(c.nb, geom->nb, 16);
        memcpy(c.shift, geom->shift, 16);
        c.cell_base = geom->first_cell(rank);
        c.ncells = geom->cells_of(rank);
        c.geom = geom;
        memcpy(c.h_bounds, geom->bounds, sizeof c.h_bounds);
        if (c.ncells < 512u || c.ncells % 64u != 0u || c.ncells > 65536u)   // (knn_geom_from_sample sizes the ranges so)
            return false;
    } else {
        const int kc = std::min(k, 16);   // dimensions the cells may cut
        const int bits = std::min(cell_bits_for_rows(n), std::min(16, 4 * kc));
        if (bits < 9)
            return false;
        c.bits = bits;
        c.ncells = 1u << bits;
        cell_grid_shape(kc, bits, c.nb, c.shift, &c.sa);
        if (c.sa < 6)   // a wave of the match pass covers 64 consecutive low-table entries
            return false;
        cell_quantile_cuts(k, c.nb, samp, samples, c.h_bounds);
    }
    // list capacity per cell and batch: 384 queries per cell at >= 2^15 cells (48 MiB of lists per slot at 2^16 cells; uniform
    // data in 16 dimensions keeps 25 of 1024 on average, 53 at most), every query of a batch at <= 2^13 cells
    // (round 5: 384 entries at >= 2^15 cells, was 128 — heavy-tailed rows with gaussian queries, n 2^24: lists of 121 .. 213
    // queries, nearly every cell `dense` (scored against all 1024), 1.16 ms per step; 0.36 with room for the lists.  The match
    // kernel assembles the first 128 entries of a list in LDS as before and writes the rest straight to memory)
    c.cap = std::min(1024u, std::max(384u, (1u << 23) / c.ncells));
    if (k > 16)   // (more dimensions, fewer cells ruled out: lists of ~100-200 of 1024 queries at k = 20 — 128 entries made most cells dense)
        c.cap = std::min(1024u, std::max(k > 20 ? 640u : 384u, (1u << 24) / c.ncells));
    // (k = 24, n 2^24: lists of 384 left most cells dense, 1.19 ms per step; 640 or 1024 entries 0.75 — the full scan takes 0.97)
    while ((1u << c.lbits) < c.ncells)   // bits of a LOCAL cell number (= bits without a shard geometry)
        ++c.lbits;
    return true;
}

// The first strategy to try.  The fast build (round 5) is taken for whole indexes (no shard geometry: their rows' codes are
// local = global and fit 16 bits) of >= 512 cells whose scratch (n x 96 bytes) fits; the counted two-pass build needs n x 64
// bytes of scratch (shards of up to 2^25 rows: beyond, the scratch is gigabytes that the buffer pool does not keep between
// builds, and one hipMalloc / hipFree pair of that size in eight took 2.2 SECONDS on a 2^27-row shard — tools/build_repeat.py:
// 30 20 19 19 19 19 2208 21 ms — where the one-pass placement's 33 ms are steady); the one-pass placement serves k > 16 and
// everything else.  cells_build: option `cells_build` (0 auto, 1 one-pass, 2 counted: A/B timing and tests).  An ingest
// (CellRows::Host) has no rows on the device to count: the fast build under the copy, or nothing.
CellBuild knn_cells_first_build(const CellIndex &plan, int k, long long n, int cells_build, CellRows rows)
{
    const bool fast_fits = !plan.geom && (size_t)n * 96 <= ((size_t)2 << 30) && plan.ncells >= 512u;
    if (rows == CellRows::Host)
        return k <= 16 && fast_fits ? CellBuild::Fast : CellBuild::None;
    if (k > 16 || cells_build == 1 || (size_t)n * 64 > ((size_t)2 << 30))
        return CellBuild::OnePass;
    return cells_build == 0 && rows == CellRows::Sample && fast_fits ? CellBuild::Fast : CellBuild::Counted;
}

// What follows a strategy that could not finish: Fast -> Counted (a bucket outgrew its fixed room — data the quantile cuts do
// not spread evenly over the 256 buckets — or no room for its scratch), Counted -> OnePass (no room for its scratch).  An
// ingest gives up instead: its rows are not on the device yet, the caller copies them, then builds.
CellBuild knn_cells_next_build(CellBuild how, CellRows rows)
{
    if (how == CellBuild::Fast && rows != CellRows::Host)
        return CellBuild::Counted;
    return how == CellBuild::Counted ? CellBuild::OnePass : CellBuild::None;
}

// The build's scratch (buckets, codes, fill counters): the layout keeps the rest.  The only place that frees it.
void knn_cells_release_build_scratch(CellIndex &c)
{
    (void)KNN_DEV_FREE(c.tmp_rows);
    (void)KNN_DEV_FREE(c.tmp_meta);
    (void)KNN_DEV_FREE(c.bucket_start);
    c.tmp_rows = nullptr;
    c.tmp_meta = nullptr;
    c.bucket_start = c.bucket_fill = c.build_res = nullptr;
}

void CellStaging::release()
{
    (void)KNN_DEV_FREE(code);
    (void)KNN_DEV_FREE(fill);
    code = fill = nullptr;
    if (c)
        knn_cells_release_build_scratch(*c);
}

// The fast build in stages (an ingest runs the scatter chunk by chunk under the copy): rows [row0, row1) of the shard, at `r`
// = the shard's first row on the device.
hipError_t knn_cells_fast_scatter(CellIndex &c, int k, const float *r, long long row0, long long row1, hipStream_t s)
{
    if (row1 <= row0)
        return hipSuccess;
    const CellGeom g = cell_geom_of(c, k);
    const long long rows = row1 - row0;
    hipLaunchKernelGGL(knn_cells_bucket_scatter_fixed_kernel, dim3((unsigned)((rows + CELL_BUILD_ROWS - 1) / CELL_BUILD_ROWS)), dim3(256), 0,
                       s, r + (size_t)row0 * k, rows, row0, g, c.bounds, c.lbits - 8, c.bucket_cap, c.bucket_fill, c.tmp_rows, c.tmp_meta,
                       c.build_res + 3);
    return hipGetLastError();
}

// rows per cell, tile ranges + items (device prefix), fill counters zeroed for the placement
hipError_t knn_cells_fast_finish(CellIndex &c, unsigned *counts, hipStream_t s)
{
    hipLaunchKernelGGL(knn_cells_bucket_cellcount_kernel, dim3(CELL_BUCKETS * CELL_PLACE_PARTS), dim3(256), 0, s, c.tmp_meta, c.bucket_start,
                       c.lbits - 8, counts, c.bucket_fill);
    hipLaunchKernelGGL(knn_cells_prefix_kernel, dim3((c.ncells + 1023u) / 1024u), dim3(1024), 0, s, counts, c.ncells, c.tile_start, c.items,
                       c.build_res);
    FTRY(hipGetLastError());
    return hipMemsetAsync(counts, 0, (size_t)c.ncells * sizeof(unsigned), s);   // the counts become the placement's fill counters
}

// The fast build (round 5): no counting pass over the rows, no host round trip (see the kernels).  Everything it launches is
// asynchronous — the finish reads c->build_res behind the placement and, if a bucket outgrew its fixed room, the build starts
// over with the counted one.  scatter = false (an ingest): everything allocated and uploaded, nothing scattered yet.
// False: no room (or a launch failed).
static bool cells_stage_fast(CellStaging &stg, const CellIndex &plan, int k, long long n, const float *r, hipStream_t s, bool scatter)
{
    CellIndex *c = new CellIndex(plan);
    // room per bucket: an even spread + 1/2.  The cuts are medians of a 1024-row sample: each is off by ~1.6 % of the rows
    // (1 sigma), a bucket is the product of 8 such halves — 1 sigma 9 %, the fullest of 256 buckets ~27 % over the mean on
    // uniform data (measured: + 1/8 overflowed at C3)
    const unsigned cap_rows = (unsigned)((n / CELL_BUCKETS) + (n / CELL_BUCKETS) / 2 + CELL_BUILD_ROWS);
    const size_t recs = (size_t)cap_rows * CELL_BUCKETS;
    const long long tiles_ub = n / 32 + (long long)c->ncells;                         // every cell wastes less than a tile
    const size_t items_ub = (size_t)c->ncells + (size_t)(tiles_ub / KNN_CELL_ITEM_TILES) + 1u;
    unsigned *counts = nullptr;
    hipError_t a = KNN_DEV_ALLOC((void **)&c->bounds, sizeof c->h_bounds + sizeof(float));
    if (a == hipSuccess)
        a = KNN_DEV_ALLOC((void **)&c->tile_start, ((size_t)c->ncells + 1) * sizeof(unsigned));
    if (a == hipSuccess)
        a = KNN_DEV_ALLOC((void **)&counts, (size_t)c->ncells * sizeof(unsigned));
    if (a == hipSuccess)
        a = KNN_DEV_ALLOC((void **)&c->tmp_rows, recs * 16 * sizeof(float));
    if (a == hipSuccess)
        a = KNN_DEV_ALLOC((void **)&c->tmp_meta, recs * sizeof(u64));
    if (a == hipSuccess)   // [257] bucket starts | [256] fills | [4] results
        a = KNN_DEV_ALLOC((void **)&c->bucket_start, (CELL_BUCKETS + 1 + CELL_BUCKETS + 4) * sizeof(unsigned));
    if (a == hipSuccess)
        a = KNN_DEV_ALLOC((void **)&c->items, items_ub * sizeof(u64));
    if (a == hipSuccess)
        a = KNN_DEV_ALLOC((void **)&c->perm, (size_t)tiles_ub * 32 * sizeof(unsigned));
    if (a == hipSuccess) {
        c->bucket_fill = c->bucket_start + CELL_BUCKETS + 1;
        c->build_res = c->bucket_fill + CELL_BUCKETS;
        for (int b = 0; b <= CELL_BUCKETS; ++b)
            c->h_bucket_start[b] = (unsigned)b * cap_rows;
        a = hipMemcpyAsync(c->bounds, c->h_bounds, sizeof c->h_bounds, hipMemcpyHostToDevice, s);
        if (a == hipSuccess)
            a = hipMemcpyAsync(c->bucket_start, c->h_bucket_start, sizeof c->h_bucket_start, hipMemcpyHostToDevice, s);
        if (a == hipSuccess)
            a = hipMemsetAsync(c->bucket_fill, 0, (CELL_BUCKETS + 4) * sizeof(unsigned), s);
        if (a == hipSuccess)
            a = hipMemsetAsync(counts, 0, (size_t)c->ncells * sizeof(unsigned), s);
        c->bucket_cap = cap_rows;
        if (a == hipSuccess && scatter) {
            a = knn_cells_fast_scatter(*c, k, r, 0, n, s);
            if (a == hipSuccess)
                a = knn_cells_fast_finish(*c, counts, s);
        }
    }
    if (a != hipSuccess) {
        (void)hipGetLastError();
        (void)KNN_DEV_FREE(counts);
        knn_cells_free(c);
        return false;
    }
    c->nitems = 0u;   // (the finish fills nitems / max_cell_rows in from build_res)
    stg.c = c;
    stg.fill = counts;
    stg.ntiles = tiles_ub;
    return true;
}

// The counted build (how = Counted: rows to buckets, bucket counts to the host, rows to cells in buckets; see the kernels) or
// the one-pass placement (how = OnePass: cell codes and counts in one pass, the rows placed straight from the shard).  Both
// end in the host prefix of the cells' counts and hand the codes and zeroed fill counters to the placement.  stg.c stays null
// when the layout is declined: no room for it, no items, or (geom) rows outside this rank's cell range — *bad_rows_out says
// how many.  Synchronous.
static hipError_t cells_stage_counted(CellStaging &stg, const CellIndex &plan, CellBuild how, int k, long long n, const float *r, hipStream_t s,
                                      unsigned *bad_rows_out)
{
    CellIndex *c = new CellIndex(plan);
    const CellGeom g = cell_geom_of(*c, k);
    unsigned *code = nullptr, *counts = nullptr;
    std::vector<unsigned> hcounts((size_t)c->ncells), hstart((size_t)c->ncells + 1);
    std::vector<u64> hitems;
    // (one word behind the cuts counts rows outside the index's cell range)
    hipError_t e = KNN_DEV_ALLOC((void **)&c->bounds, sizeof c->h_bounds + sizeof(float));
    unsigned *bad_dev = (unsigned *)(c->bounds + sizeof c->h_bounds / sizeof(float));
    if (e == hipSuccess)
        e = hipMemsetAsync(bad_dev, 0, sizeof(unsigned), s);
    if (e == hipSuccess)
        e = KNN_DEV_ALLOC((void **)&c->tile_start, hstart.size() * sizeof(unsigned));
    if (e == hipSuccess)
        e = KNN_DEV_ALLOC((void **)&code, (size_t)n * sizeof(unsigned));
    if (e == hipSuccess)
        e = KNN_DEV_ALLOC((void **)&counts, hcounts.size() * sizeof(unsigned));
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->bounds, c->h_bounds, sizeof c->h_bounds, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemsetAsync(counts, 0, hcounts.size() * sizeof(unsigned), s);
    const int bshift = c->lbits - 8;   // >= 512 cells: a bucket = 2^bshift consecutive (local) cells
    const unsigned bblocks = (unsigned)((n + CELL_BUILD_ROWS - 1) / CELL_BUILD_ROWS);
    unsigned *bucket_counts = nullptr, hb[CELL_BUCKETS], hbs[CELL_BUCKETS + 1];   // (hbs: the source of a copy the sync below waits for)
    if (e == hipSuccess && how == CellBuild::Counted) {   // the scratch: n x 72 bytes
        hipError_t a = KNN_DEV_ALLOC((void **)&c->tmp_rows, (size_t)n * 16 * sizeof(float));
        if (a == hipSuccess)
            a = KNN_DEV_ALLOC((void **)&c->tmp_meta, (size_t)n * sizeof(u64));
        if (a == hipSuccess)
            a = KNN_DEV_ALLOC((void **)&c->bucket_start, (CELL_BUCKETS + 1) * sizeof(unsigned));
        if (a == hipSuccess)
            a = KNN_DEV_ALLOC((void **)&bucket_counts, 2 * CELL_BUCKETS * sizeof(unsigned));
        if (a != hipSuccess) {
            (void)hipGetLastError();
            knn_cells_release_build_scratch(*c);
            (void)KNN_DEV_FREE(bucket_counts);
            bucket_counts = nullptr;
            how = knn_cells_next_build(how, CellRows::Sample);
        }
    }
    if (e == hipSuccess && how == CellBuild::Counted) {
        unsigned *bucket_fill = bucket_counts + CELL_BUCKETS;
        e = hipMemsetAsync(bucket_counts, 0, 2 * CELL_BUCKETS * sizeof(unsigned), s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(knn_cells_bucket_count_kernel, dim3(bblocks), dim3(256), 0, s, r, n, g, c->bounds, bshift, code,
                               bucket_counts, bad_dev);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(hb, bucket_counts, sizeof hb, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (e == hipSuccess) {
            unsigned acc = 0u;
            for (int b = 0; b < CELL_BUCKETS; ++b) {
                hbs[b] = acc;
                acc += hb[b];
            }
            hbs[CELL_BUCKETS] = acc;
            e = hipMemcpyAsync(c->bucket_start, hbs, sizeof hbs, hipMemcpyHostToDevice, s);
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(knn_cells_bucket_scatter_kernel, dim3(bblocks), dim3(256), 0, s, r, n, k, bshift, code, c->bucket_start,
                               bucket_fill, c->tmp_rows, c->tmp_meta);
            hipLaunchKernelGGL(knn_cells_bucket_cellcount_kernel, dim3(CELL_BUCKETS * CELL_PLACE_PARTS), dim3(256), 0, s, c->tmp_meta,
                               c->bucket_start, bshift, counts, (const unsigned *)nullptr);
            e = hipGetLastError();
        }
    } else if (e == hipSuccess) {
        hipLaunchKernelGGL(knn_cells_code_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, r, n, g, c->bounds, code, counts, bad_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(hcounts.data(), counts, hcounts.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    (void)KNN_DEV_FREE(bucket_counts);
    bool keep = e == hipSuccess;
    if (keep && c->geom) {   // rows outside this rank's cell range: the caller partitioned with another geometry
        unsigned hbad = 0u;
        e = hipMemcpy(&hbad, bad_dev, sizeof hbad, hipMemcpyDeviceToHost);
        if (e == hipSuccess && hbad != 0u) {
            if (bad_rows_out)
                *bad_rows_out = hbad;
            keep = false;
        }
        keep = keep && e == hipSuccess;
    }
    long long tiles = 0;
    if (keep) {
        unsigned biggest = 0u;
        for (unsigned i = 0; i < c->ncells; ++i) {
            hstart[i] = (unsigned)tiles;
            tiles += (hcounts[i] + 31u) / 32u;
            biggest = std::max(biggest, hcounts[i]);
        }
        hstart[c->ncells] = (unsigned)tiles;
        c->max_cell_rows = biggest;
        // (round 2 gave up here when the largest cell held more than 16x the average — clustered or low-rank data the
        // per-dimension quantiles do not spread.  The scan now takes ITEMS, runs of at most KNN_CELL_ITEM_TILES tiles of one
        // cell, so a fat cell is many waves' work instead of one's, and cells without rows cost nothing)
        for (unsigned i = 0; i < c->ncells; ++i)
            for (unsigned t = hstart[i]; t < hstart[i + 1]; t += KNN_CELL_ITEM_TILES)
                hitems.push_back(((u64)i << 48) | ((u64)std::min((unsigned)KNN_CELL_ITEM_TILES, hstart[i + 1] - t) << 40) | (u64)t);
        c->nitems = (unsigned)hitems.size();
        keep = c->nitems != 0u;
    }
    if (keep) {
        // the rows are placed (and turned into fragments) by knn_cells_scatter_frag_kernel once the layout buffers
        // exist: `code` and the zeroed fill counters go to the finish
        e = hipMemcpyAsync(c->tile_start, hstart.data(), hstart.size() * sizeof(unsigned), hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = hipMemsetAsync(counts, 0, hcounts.size() * sizeof(unsigned), s);
        if (e == hipSuccess)
            e = KNN_DEV_ALLOC((void **)&c->items, hitems.size() * sizeof(u64));
        if (e == hipSuccess)
            e = hipMemcpyAsync(c->items, hitems.data(), hitems.size() * sizeof(u64), hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            e = KNN_DEV_ALLOC((void **)&c->perm, (size_t)tiles * 32 * sizeof(unsigned));   // (filled by the placement + padding kernels)
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);   // hstart / hitems are about to go out of scope
    }
    if (e == hipErrorOutOfMemory) {   // no room for the sort: the plain layout still works
        (void)hipGetLastError();
        e = hipSuccess;
        keep = false;
    }
    if (e != hipSuccess || !keep) {
        (void)KNN_DEV_FREE(code);
        (void)KNN_DEV_FREE(counts);
        knn_cells_free(c);
        return e;
    }
    stg.c = c;
    stg.code = code;
    stg.fill = counts;
    stg.ntiles = tiles;
    return hipSuccess;
}

// Stages `how` (Fast, Counted or OnePass): the rows' cells counted, the cells' tile ranges and items made (the fast build:
// enqueued), the layout's perm allocated.  A fast build without room for its scratch falls back (knn_cells_next_build) here.
// stg.c stays null when the shard does not suit the cells.
hipError_t knn_cells_stage(CellStaging &stg, const CellIndex &plan, CellBuild how, CellRows rows, int k, long long n, const float *r,
                           hipStream_t s, unsigned *bad_rows_out)
{
    stg = CellStaging();
    if (how == CellBuild::Fast) {
        if (cells_stage_fast(stg, plan, k, n, r, s, rows != CellRows::Host))
            return hipSuccess;
        how = knn_cells_next_build(how, rows);
    }
    if (how == CellBuild::None)
        return hipSuccess;
    return cells_stage_counted(stg, plan, how, k, n, r, s, bad_rows_out);
}

// Every row to its cell (knn_cells_place_kernel / knn_cells_scatter_frag_kernel), then the padding of the cells' last tiles.
// code / fill: what knn_cells_stage handed back; out: the 4 words of knn_frag_kernel's statistics.
hipError_t knn_cells_place_rows(FilterState &st, const float *r, const unsigned *code, unsigned *fill, unsigned *out,
                                unsigned ocap, hipStream_t s)
{
    if (st.cells->tmp_rows)
        hipLaunchKernelGGL(knn_cells_place_kernel, dim3(CELL_BUCKETS * CELL_PLACE_PARTS), dim3(256), 0, s, st.cells->tmp_rows,
                           st.cells->tmp_meta, st.cells->bucket_start, st.k, st.cells->lbits - 8, st.cells->tile_start, fill, st.center, st.sigma,
                           (h8 *)st.ref_frags, st.ref_norms, st.ref_norms2, st.cells->perm, out, st.outliers, ocap,
                           (const unsigned *)st.cells->bucket_fill);
    else if (st.kt == 2)
        hipLaunchKernelGGL(knn_cells_scatter_frag2_kernel, dim3((unsigned)((st.n + 255) / 256)), dim3(256), 0, s, r, st.n, st.k, code,
                           st.cells->tile_start, fill, st.center, st.sigma, (h8 *)st.ref_frags, st.ref_norms, st.ref_norms2,
                           st.cells->perm, out, st.outliers, ocap);
    else
        hipLaunchKernelGGL(knn_cells_scatter_frag_kernel, dim3((unsigned)((st.n + 255) / 256)), dim3(256), 0, s, r, st.n, st.k, code,
                           st.cells->tile_start, fill, st.center, st.sigma, (h8 *)st.ref_frags, st.ref_norms, st.ref_norms2,
                           st.cells->perm, out, st.outliers, ocap);
    FTRY(hipGetLastError());
    hipLaunchKernelGGL(knn_cells_pad_kernel, dim3((st.cells->ncells + 7u) / 8u), dim3(256), 0, s, st.cells->tile_start, fill,
                       st.cells->ncells, (h8 *)st.ref_frags, st.ref_norms, st.ref_norms2, st.cells->perm, st.kt,
                       st.kt == 2 && st.k <= KNN_NIF_MAX_K ? 1 : 0);
    return hipGetLastError();
}

void knn_cells_workspace_free(FilterWorkspace &w)
{
    (void)KNN_DEV_FREE(w.cell_counts);
    (void)KNN_DEV_FREE(w.cell_lists);
    (void)KNN_DEV_FREE(w.dup);
    (void)KNN_DEV_FREE(w.lo_tab);
    (void)KNN_DEV_FREE(w.hi_tab);
    (void)KNN_DEV_FREE(w.lo_min);
    w.cell_counts = nullptr;
    w.cell_lists = nullptr;
    w.dup = w.lo_tab = w.hi_tab = w.lo_min = nullptr;
    w.cell_m_cap = 0;
}

// ---- per batch ---------------------------------------------------------------------------------

// The dynamic-LDS limit is an attribute of the function on the device, not of a launch: a variant that may ask for more than the
// default gets the most it can ask for (the plan's limit) once per device, before its first launch there.  (Set per launch to the
// batch's own size, another thread's set could lower it between that set and that launch.)
static hipError_t cells_lds_limit(const void *fn, size_t limit)
{
    if (!limit)
        return hipSuccess;
    int dev = 0;
    FTRY(hipGetDevice(&dev));
    static std::mutex mu;
    static std::set<std::pair<int, const void *>> done;
    std::lock_guard<std::mutex> lock(mu);
    if (!done.count({dev, fn})) {
        FTRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
        done.insert({dev, fn});
    }
    return hipSuccess;
}

// What the launches of one batch read: the index, the slot's workspace, the plan and the call's arguments.  A driver fills in
// the call's part; cells_pass_front adds the last three, which follow from the workspace.
struct CellBatch {
    const FilterState &st;
    const CellIndex &c;
    const FilterWorkspace &w;
    const CellQueryPlan &p;
    int m;
    const float *q, *r;
    long long base;
    u64 *keys, *keys_init;
    CellFinal fin;
    SeedLayer layer;
    hipStream_t s;
    int topk = 0;   // a top-K pass: K (the prep kernel's TK form)
    float max_dist2 = INFINITY;   // a top-K pass of a radius call, a count pass: the radius (finite: the prep kernel's WR form)
    int m_padded = 0;
    CellSelf self = CellSelf{};
    unsigned *ctl_next = nullptr;
    const float *radii = nullptr;   // a count pass with a radius per query: the pass's radii (max_dist2 the cap; the prep kernel's EACH form)
};

struct CellKernel {   // a kernel the plan picked: its launch for a batch, and the kernel itself (for its attributes)
    void (*launch)(const CellBatch &);
    const void *fn;
};

// (SD = 2, four seed cells; cell-range shards take the same four — those of another rank through the seed layer.  Sixteen seed
// cells (SD = 4) leave 20 % fewer candidates, as the simulation said, and cost more than they save: the prep kernel is a chain
// of dependent round trips, and at a rank's size the step is made of those — emulated rank of N = 8, ms per step / one
// batch at a time: 16 cells x 2 tiles 0.0302 / 0.0526, 8 x 2 0.0279 / 0.0493, 4 x 2 0.0275 / 0.0471, 4 x 4 0.0271 / 0.0473;
// N = 4: 0.0432 / 0.0423 / 0.0414 / 0.0408.  profiles/r04_seed_sweep.txt)
// knn_cells_prep_kernel's three forms, told apart by its last four arguments:
//   1-NN (TK false)             keys_init, the low table's order, the cells' frames (read with CTR only)
//   top-K (TK, one frame)       no keys (the select kernel starts them), K — the K-th smallest seed score (knn_seed_kth.h) —, no frames
//   top-K on per-cell frames    no keys, K — the K-th smallest frame-free bound (knn_frame_dup.h) —, the cells' frames
template <int PW, int KT, bool CTR, bool TK>
static CellKernel cells_prep_of()
{
    return {[](const CellBatch &b) {
                const FilterState &st = b.st;
                const bool frames = CTR || !TK;
                hipLaunchKernelGGL((knn_cells_prep_kernel<PW, 2, KT, CTR, TK>), dim3((unsigned)b.m_padded), dim3(64 * PW), 0, b.s, b.q, b.m,
                                   b.m_padded, cell_geom_of(b.c, st.k), b.c.bounds, (double)st.sigma * (double)st.sigma, st.center, st.sigma,
                                   b.c.tile_start, st.ntiles, (const h8 *)st.ref_frags, st.ref_norms2, b.layer, (h8 *)b.w.qry_frags, b.w.lo_tab,
                                   b.w.hi_tab, b.w.lo_min, st.bmax, st.nmax, kAmaxLimit, b.w.thr, b.w.dup, b.w.ctl_cur, b.ctl_next, b.w.counts, b.w.nlists,
                                   TK ? (u64 *)nullptr : b.keys_init, TK ? b.topk : b.p.self_lists ? 1 : 0,
                                   frames ? b.c.cell_frame : (const float *)nullptr, frames ? b.c.tile_cell : (const unsigned *)nullptr);
            },
            (const void *)knn_cells_prep_kernel<PW, 2, KT, CTR, TK>};
}
// ... of a radius call (knn_index_query_topk_within): Dup_q capped by the radius
template <int PW, int KT>
static CellKernel cells_prep_within_of()
{
    return {[](const CellBatch &b) {
                const FilterState &st = b.st;
                hipLaunchKernelGGL((knn_cells_prep_within_kernel<PW, 2, KT>), dim3((unsigned)b.m_padded), dim3(64 * PW), 0, b.s, b.q, b.m,
                                   b.m_padded, cell_geom_of(b.c, st.k), b.c.bounds, (double)st.sigma * (double)st.sigma, st.center, st.sigma,
                                   b.c.tile_start, st.ntiles, (const h8 *)st.ref_frags, st.ref_norms2, b.layer, (h8 *)b.w.qry_frags, b.w.lo_tab,
                                   b.w.hi_tab, b.w.lo_min, st.bmax, st.nmax, kAmaxLimit, b.w.thr, b.w.dup, b.w.ctl_cur, b.ctl_next, b.w.counts, b.w.nlists,
                                   b.topk, b.max_dist2);
            },
            (const void *)knn_cells_prep_within_kernel<PW, 2, KT>};
}
// ... of a count pass (knn_index_count_within): the radius cap alone
template <int PW, int KT>
static CellKernel cells_prep_count_of()
{
    return {[](const CellBatch &b) {
                const FilterState &st = b.st;
                hipLaunchKernelGGL((knn_cells_prep_count_kernel<PW, 2, KT>), dim3((unsigned)b.m_padded), dim3(64 * PW), 0, b.s, b.q, b.m,
                                   b.m_padded, cell_geom_of(b.c, st.k), b.c.bounds, (double)st.sigma * (double)st.sigma, st.center, st.sigma,
                                   b.c.tile_start, (h8 *)b.w.qry_frags, b.w.lo_tab, b.w.hi_tab, b.w.lo_min, st.bmax, st.nmax, kAmaxLimit, b.w.thr, b.w.dup,
                                   b.w.ctl_cur, b.ctl_next, b.w.counts, b.w.nlists, b.max_dist2);
            },
            (const void *)knn_cells_prep_count_kernel<PW, 2, KT>};
}
// ... of a count pass with a radius per query (knn_index_count_within_each): the block's own query's bound
template <int PW, int KT>
static CellKernel cells_prep_each_of()
{
    return {[](const CellBatch &b) {
                const FilterState &st = b.st;
                hipLaunchKernelGGL((knn_cells_prep_each_kernel<PW, 2, KT>), dim3((unsigned)b.m_padded), dim3(64 * PW), 0, b.s, b.q, b.m,
                                   b.m_padded, cell_geom_of(b.c, st.k), b.c.bounds, (double)st.sigma * (double)st.sigma, st.center, st.sigma,
                                   b.c.tile_start, (h8 *)b.w.qry_frags, b.w.lo_tab, b.w.hi_tab, b.w.lo_min, st.bmax, st.nmax, kAmaxLimit, b.w.thr, b.w.dup,
                                   b.w.ctl_cur, b.ctl_next, b.w.counts, b.w.nlists, b.radii, b.max_dist2);
            },
            (const void *)knn_cells_prep_each_kernel<PW, 2, KT>};
}
// The prep kernel's forms: what the pass is for, then the plan's prep shape (prep_pw waves per query, prep_kt, prep_ctr) — the 12
// instantiations of knn_cells_prep_kernel and the 4 each of the radius, the count and the radius-per-query kernel.
enum class CellPrepForm { Nearest, Topk, TopkWithin, Count, CountEach };
static CellKernel cells_prep_kernel(CellPrepForm form, const CellQueryPlan &p)
{
    const bool two = p.prep_pw == 2, kt2 = p.prep_kt == 2;
    if (form == CellPrepForm::CountEach)
        return kt2 ? (two ? cells_prep_each_of<2, 2>() : cells_prep_each_of<4, 2>()) : (two ? cells_prep_each_of<2, 1>() : cells_prep_each_of<4, 1>());
    if (form == CellPrepForm::Count)
        return kt2 ? (two ? cells_prep_count_of<2, 2>() : cells_prep_count_of<4, 2>()) : (two ? cells_prep_count_of<2, 1>() : cells_prep_count_of<4, 1>());
    if (form == CellPrepForm::Nearest) {
        if (p.prep_ctr)
            return two ? cells_prep_of<2, 1, true, false>() : cells_prep_of<4, 1, true, false>();
        return kt2 ? (two ? cells_prep_of<2, 2, false, false>() : cells_prep_of<4, 2, false, false>())
                   : (two ? cells_prep_of<2, 1, false, false>() : cells_prep_of<4, 1, false, false>());
    }
    if (p.prep_ctr)   // (per-cell frames are not capped: a radius call clips their lists behind)
        return two ? cells_prep_of<2, 1, true, true>() : cells_prep_of<4, 1, true, true>();
    if (form == CellPrepForm::TopkWithin)
        return kt2 ? (two ? cells_prep_within_of<2, 2>() : cells_prep_within_of<4, 2>()) : (two ? cells_prep_within_of<2, 1>() : cells_prep_within_of<4, 1>());
    return kt2 ? (two ? cells_prep_of<2, 2, false, true>() : cells_prep_of<4, 2, false, true>())
               : (two ? cells_prep_of<2, 1, false, true>() : cells_prep_of<4, 1, false, true>());
}

template <int WAVES>
static CellKernel cells_match_of()
{
    return {[](const CellBatch &b) {
                hipLaunchKernelGGL(knn_cells_match_kernel<WAVES>, dim3(b.c.ncells / 64u), dim3(64 * WAVES), b.p.match_lds, b.s, b.w.lo_tab,
                                   b.w.hi_tab, b.w.lo_min, b.w.dup, b.m, b.m_padded, cell_geom_of(b.c, b.st.k), b.c.ncells, b.c.cap, b.w.cell_lists,
                                   b.w.cell_counts, b.w.ctl_cur, b.p.stage);
            },
            (const void *)knn_cells_match_kernel<WAVES>};
}
static CellKernel cells_match_kernel(int waves)
{
    return waves == 16 ? cells_match_of<16>() : cells_match_of<8>();
}

template <bool DYN, int K, bool SELF, int KT = 1, bool CTR = false, bool NIF = false, bool U8 = false>
static CellKernel cells_scan_of()
{
    return {[](const CellBatch &b) {
                const CellIndex &c = b.c;
                const FilterWorkspace &w = b.w;
                hipLaunchKernelGGL((knn_cells_scan_kernel<DYN, K, SELF, KT, CTR, NIF, U8>), dim3(b.p.grid.blocks), dim3(64 * b.p.grid.waves),
                                   b.p.grid.lds_bytes, b.s, U8 ? (const h8 *)c.rows8 : (const h8 *)b.st.ref_frags, U8 ? c.norms8 : b.st.ref_norms,
                                   c.items, c.nitems, (const h8 *)w.qry_frags, w.thr, b.m, b.m_padded, w.cell_counts, w.cell_lists,
                                   b.p.list_cap, w.records, w.counts, w.ctl_cur, w.slice, w.ovf_base, w.ovf_cap, b.q, b.r, b.st.k, c.perm,
                                   b.st.ntiles * 32, b.base, b.keys, b.fin, b.self);
            },
            (const void *)knn_cells_scan_kernel<DYN, K, SELF, KT, CTR, NIF, U8>};
}
// The scan's forms (knn_cells_query_plan picks one): the 20 instantiations of knn_cells_scan_kernel.
static CellKernel cells_scan_kernel(const CellScanForm &f)
{
    const bool k16 = f.k == 16;
    if (f.u8)
        return f.ctr ? (k16 ? cells_scan_of<true, 16, false, 1, true, false, true>() : cells_scan_of<true, 0, false, 1, true, false, true>())
                     : (k16 ? cells_scan_of<true, 16, false, 1, false, false, true>() : cells_scan_of<true, 0, false, 1, false, false, true>());
    if (f.ctr)
        return f.dyn ? (k16 ? cells_scan_of<true, 16, false, 1, true>() : cells_scan_of<true, 0, false, 1, true>())
                     : (k16 ? cells_scan_of<false, 16, false, 1, true>() : cells_scan_of<false, 0, false, 1, true>());
    if (f.kt == 2)
        return f.nif ? (f.dyn ? cells_scan_of<true, 0, false, 2, false, true>() : cells_scan_of<false, 0, false, 2, false, true>())
                     : (f.dyn ? cells_scan_of<true, 0, false, 2>() : cells_scan_of<false, 0, false, 2>());
    if (f.self)
        return f.dyn ? (k16 ? cells_scan_of<true, 16, true>() : cells_scan_of<true, 0, true>())
                     : (k16 ? cells_scan_of<false, 16, true>() : cells_scan_of<false, 0, true>());
    return f.dyn ? (k16 ? cells_scan_of<true, 16, false>() : cells_scan_of<true, 0, false>())
                 : (k16 ? cells_scan_of<false, 16, false>() : cells_scan_of<false, 0, false>());
}

template <bool DYN, int KT = 1, bool NIF = false, bool U8 = false>
static CellKernel cells_records_of()
{
    return {[](const CellBatch &b) {
                const CellIndex &c = b.c;
                const FilterWorkspace &w = b.w;
                hipLaunchKernelGGL((knn_cells_records_kernel<DYN, KT, NIF, U8>), dim3(b.p.grid.blocks), dim3(64 * b.p.grid.waves),
                                   b.p.grid.lds_bytes, b.s, U8 ? (const h8 *)c.rows8 : (const h8 *)b.st.ref_frags, U8 ? c.norms8 : b.st.ref_norms,
                                   c.items, c.nitems, (const h8 *)w.qry_frags, w.thr, b.m, b.m_padded, w.cell_counts, w.cell_lists,
                                   b.p.list_cap, w.records, w.counts, w.ctl_cur, w.slice, w.ovf_base, w.ovf_cap, b.st.k, b.self);
            },
            (const void *)knn_cells_records_kernel<DYN, KT, NIF, U8>};
}
template <bool DYN, bool U8>
static CellKernel cells_frame_records_of()
{
    return {[](const CellBatch &b) {
                const CellIndex &c = b.c;
                const FilterWorkspace &w = b.w;
                hipLaunchKernelGGL((knn_cells_frame_records_kernel<DYN, U8>), dim3(b.p.grid.blocks), dim3(64 * b.p.grid.waves),
                                   b.p.grid.lds_bytes, b.s, U8 ? (const h8 *)c.rows8 : (const h8 *)b.st.ref_frags, U8 ? c.norms8 : b.st.ref_norms,
                                   c.items, c.nitems, (const h8 *)w.qry_frags, w.thr, b.m, b.m_padded, w.cell_counts, w.cell_lists,
                                   b.p.list_cap, w.records, w.counts, w.ctl_cur, w.slice, w.ovf_base, w.ovf_cap, b.q, b.st.k, b.self);
            },
            (const void *)knn_cells_frame_records_kernel<DYN, U8>};
}
// The record-only scan's forms (knn_cells_topk_plan picks one): the 7 instantiations of knn_cells_records_kernel and, for per-cell
// frames, the 3 of knn_cells_frame_records_kernel.
static CellKernel cells_records_kernel(const CellScanForm &f)
{
    if (f.ctr)
        return f.u8 ? cells_frame_records_of<true, true>() : f.dyn ? cells_frame_records_of<true, false>() : cells_frame_records_of<false, false>();
    if (f.u8)
        return cells_records_of<true, 1, false, true>();
    if (f.kt == 2)
        return f.nif ? (f.dyn ? cells_records_of<true, 2, true>() : cells_records_of<false, 2, true>())
                     : (f.dyn ? cells_records_of<true, 2>() : cells_records_of<false, 2>());
    return f.dyn ? cells_records_of<true>() : cells_records_of<false>();
}

template <int K, int KT = 1>
static void cells_tail_as(const CellBatch &b)
{
    const FilterWorkspace &w = b.w;
    hipLaunchKernelGGL((knn_cells_tail_kernel<K, KT>), dim3(b.p.tail_blocks), dim3(KNN_BLOCK), 0, b.s, b.q, b.r, b.st.k, b.m, b.st.n,
                       b.st.ntiles * 32, b.base, b.c.items, b.c.nitems, w.cell_counts, w.cell_lists, b.p.list_cap, b.c.perm, w.records, w.ovf_base, w.ovf_cap,
                       w.ctl_cur, b.keys, b.fin, w.counts, w.nlists, w.slice, b.self);
}
static void cells_tail_launch(const CellBatch &b)
{
    (b.p.tail_kt == 2 ? cells_tail_as<0, 2> : b.p.tail_k == 16 ? cells_tail_as<16> : b.p.tail_k == 8 ? cells_tail_as<8> : cells_tail_as<0>)(b);
}

static hipError_t ensure_cells_workspace(const FilterState &st,FilterWorkspace &w, int m, const CellQueryPlan &p, const CellKernel &scan)
{
    const CellIndex &c = *st.cells;
    if (!w.cell_counts)
        FTRY(KNN_DEV_ALLOC((void **)&w.cell_counts, (size_t)c.ncells * sizeof(unsigned)));
    if (!w.cell_lists)
        FTRY(KNN_DEV_ALLOC((void **)&w.cell_lists, (size_t)c.ncells * c.cap * sizeof(unsigned short)));
    const int m_padded = (m + 31) / 32 * 32;
    if (m_padded > w.cell_m_cap) {
        (void)KNN_DEV_FREE(w.dup);
        (void)KNN_DEV_FREE(w.lo_tab);
        (void)KNN_DEV_FREE(w.hi_tab);
        (void)KNN_DEV_FREE(w.lo_min);
        w.dup = w.lo_tab = w.hi_tab = w.lo_min = nullptr;
        w.cell_m_cap = 0;
        FTRY(KNN_DEV_ALLOC((void **)&w.dup, (size_t)m_padded * sizeof(float)));
        FTRY(KNN_DEV_ALLOC((void **)&w.lo_tab, (size_t)m_padded * ((size_t)1 << c.sa) * sizeof(float)));
        FTRY(KNN_DEV_ALLOC((void **)&w.hi_tab, (size_t)m_padded * (size_t)((c.ncells + (1u << c.sa) - 1u) >> c.sa) * sizeof(float)));
        FTRY(KNN_DEV_ALLOC((void **)&w.lo_min, (size_t)m_padded * (((size_t)1 << c.sa) / 64u) * sizeof(float)));   // (2^sa >= 64)
        w.cell_m_cap = m_padded;
    }
    FTRY(cells_lds_limit(scan.fn, p.scan_lds_limit));
    if (p.match_waves)
        FTRY(cells_lds_limit(cells_match_kernel(p.match_waves).fn, p.match_lds_limit));
    return hipSuccess;
}

// Every size the scan launch and the re-rank behind it index with, in one place (tests/test_cells_logic.py checks the
// arithmetic on the CPU through knn_debug_scan_plan):
//   blocks   scan grid: blocks_per_cu per CU, fewer when the index has fewer items than that many waves
//   nlists   = blocks x CELL_SCAN_WAVES record lists, one per wave: counts[nlists] (the workspace holds kMaxLists = 2^16)
//   slice    records [w x slice, (w + 1) x slice) belong to wave w
//   ovf      records [ovf_base, ovf_base + ovf_cap) are the area all waves share; nlists x slice <= ovf_base
//   lds      dynamic LDS of the scan: m_padded x (32 B operand + 4 B threshold) + one norm window per wave
CellScanPlan knn_cells_scan_plan(int num_cu, int blocks_per_cu, unsigned nitems, unsigned rec_cap, int m_padded, bool self_lists, int kt,
                                 bool centred)
{
    CellScanPlan p;
    const unsigned sw = kt == 1 && !centred ? CELL_SCAN_WAVES : CELL_SCAN_WAVES_KT2;
    p.waves = sw;
    p.blocks = (unsigned)num_cu * (unsigned)(kt == 1 && !centred ? blocks_per_cu : 1);
    if (p.blocks * sw > nitems)
        p.blocks = std::max(1u, nitems / sw);
    p.nlists = p.blocks * sw;
    // the tail of the record buffer is shared by all waves: what a wave's own slice cannot hold goes there.  2^16 records:
    // room for a batch whose queries crowd into a few cells (1024 copies of one query leave ~2000 records there), and small
    // enough that a batch the fp16 scores cannot separate at all (a cluster tighter than the fp16 step: millions of
    // candidates, one atomic on ONE word per overflowing step) over-fills it — and stops scanning — within microseconds
    p.ovf_cap = std::min(rec_cap / 4u, 1u << 16);
    p.ovf_base = rec_cap - p.ovf_cap;
    p.slice = p.ovf_base / p.nlists;
    // (16 < k <= 32: 64-byte B operands, 74 KiB for 1024 queries: with windows of nine 2-KiB tiles in registers (126 VGPRs) a CU
    // holds ONE block, so that block has sixteen waves — four per SIMD; the kernel's dynamic-LDS limit is raised above the
    // default 64 KiB (cells_lds_limit).  Round 5, one box, ms per step at k 17 / 18 / 20, n 2^24: four tiles per pass, 12 waves, 96
    // registers 0.282 / 0.315 / 0.428; five 0.269 / 0.303 / 0.399; nine, 12 waves (3 per SIMD) 0.237 / 0.242 / 0.352)
    p.lds_bytes = (size_t)m_padded * ((centred ? 64 : 32 * kt) + 4) + (size_t)sw * CELL_TILES_PER_PASS * 8 * sizeof(f4v);   // (per-cell frames: the queries' fp32 rows)
    if (self_lists)   // the self-listing scan: the batch's Dup values + one list room per wave
        p.lds_bytes += (size_t)m_padded * sizeof(float) + (size_t)sw * CELL_SELF_CAP * sizeof(unsigned short);
    else if (centred)   // per-cell frames: the batch's Dup values
        p.lds_bytes += (size_t)m_padded * sizeof(float);
    return p;
}

// Who lists the queries of a cell (option `cells_lists` 0 = this policy, 1 = the match launch, 2 = the scan's own waves).
// Measured (round 5, one MI355X, k 16, m 1024, uniform; profiles/r05_self_lists.txt): the self-listing scan saves the match
// launch and a dependent round trip per item, and pays with 16 steps of table arithmetic per item inside the hot kernel.  One
// batch at a time on a rank of 8 of C3 (2^13 cells): 0.0469 -> 0.0439 ms; with four batches in flight the match launch hides
// behind the other batches and the longer scan does not: 0.0252 -> 0.0288 per step.  2^14 cells: 0.0599 -> 0.0616 / 0.0397 ->
// 0.0433; C3: 0.1430 -> 0.1448 / 0.1176 -> 0.1280.
bool knn_cells_lists_policy(unsigned ncells, bool several_slots)
{
    return !several_slots && ncells <= 8192u;
}

// What one batch launches and with which sizes, decided in one place (host arithmetic: nothing allocated or launched;
// tests/test_cells_logic.py checks it on the CPU through knn_debug_cells_query_plan).
CellQueryPlan knn_cells_query_plan(const CellQueryInputs &in)
{
    CellQueryPlan p;
    const int m_padded = (in.m + 31) / 32 * 32;
    // prep: batches in flight side by side: two waves per query (two seed cells each) — half the registers the launch holds,
    // 0.0421 -> 0.0408 ms per step at n_local 2^21 for 2 us more when a batch runs alone; else four waves per query
    p.prep_pw = in.several_slots ? 2 : 4;
    p.prep_kt = in.centred ? 1 : in.kt;
    p.prep_ctr = in.centred;
    // scan grid: two blocks of CELL_SCAN_WAVES waves per CU fill every SIMD's registers (6 waves x 80) and give the shortest
    // launch — and leave nothing for the kernels of the next batch, so with batches in flight side by side the step was the
    // SUM of the kernels' durations.  One block per CU: the scan alone takes 10-20 % longer, the step of a shard of up to 2^14
    // cells 5-7 % less (0.0465 -> 0.0444 ms at 2^21 rows; at C3 the two are within 1 %: it keeps two).
    // (2^15 cells, n = 2^23: step 0.0795 -> 0.0777 with one, three runs each on one box; 2^16 cells, C3: 0.1237 -> 0.1223, not
    // worth the 8 % the launch itself gets longer)
    const bool one_block = in.scan_blocks == 1 || (in.scan_blocks == 0 && in.several_slots && in.ncells <= 32768u);
    // Who makes the cells' lists of queries: knn_cells_match_kernel in a launch of its own (rounds 2-4), or the scan's waves
    // for the items they take (round 5, cell_self_list).  Policy in knn_cells_lists_policy.  Per-cell frames and 8-bit rows:
    // lists from the match launch.
    p.self_lists = in.kt == 1 && !in.centred && !in.rows_u8 &&
                   (in.cells_lists == 2 || (in.cells_lists == 0 && knn_cells_lists_policy(in.ncells, in.several_slots)));
    p.grid = knn_cells_scan_plan(in.num_cu, one_block ? 1 : 2, in.nitems, in.rec_cap, m_padded, p.self_lists, in.kt, in.centred);
    p.list_cap = p.self_lists ? CELL_SELF_CAP : in.cap;
    if (!p.self_lists) {
        // entries of a list assembled in LDS: k <= 16 the first 128 (16.6 KiB: four or five blocks per CU), 16 < k <= 32 the whole
        // list up to 640 entries (lists of 150-400 are the rule there)
        // (a rank of 8 of C3 — 2^13 cells, room for 1024 entries, lists of ~25 — on one box, ms per pipelined step: nothing staged (rounds
        // 2-5) 0.0290 / 0.0301, 128 entries 0.0266 / 0.0269, 256 entries 0.0274 / 0.0280)
        p.match_waves = in.ncells <= 16384u ? 16 : 8;
        p.stage = in.kt == 1 ? std::min(in.cap, 128u) : in.cap <= CELL_MATCH_STAGED_CAP ? in.cap : 0u;
        p.match_lds = p.stage ? (size_t)64 * (p.stage + 2u) * sizeof(unsigned short) : 0;
        // (12-20 KiB of static LDS in front of it: a staged list of 16 < k <= 32 may ask for more than the default 48 KiB)
        if (in.kt == 2)
            p.match_lds_limit = (size_t)64 * (CELL_MATCH_STAGED_CAP + 2u) * sizeof(unsigned short);
    }
    // Items handed out inside the block (LDS counter, see the kernel) when batches come one at a time: the launch is as long as
    // its busiest wave, and evening the waves out takes 6-8 % off it (alone, ms: 0.0433 -> 0.0408 at 2^21 rows, 0.060 -> 0.055 at
    // 2^22, 0.1176 -> 0.1094 at C3; one batch at a time 0.0855 -> 0.0828, 0.102 -> 0.097, 0.1677 -> 0.160).  With batches in
    // flight on several slots the next batch's kernels fill the gaps early finishers leave, and the fixed deal's cheaper prologue
    // and moving window win: the step is 1-4 % SHORTER with it (0.0415 / 0.0549 / 0.0794 / 0.1233 against 0.0425 / 0.0568 /
    // 0.0831 / 0.1249) — so that is what pipelined callers get.
    // (below two items per wave the counter has nothing to even out: 2^21 rows, one batch at a time, 0.0786 ms fixed / 0.0800 counter)
    // (round 4: the counter form lost its 8 bytes of scratch and requests its first descriptors in front of the LDS fill — 3.6 %
    // shorter alone at C3, 0.1127 against 0.1169 ms between events — and with that it also gives the shorter PIPELINED step on
    // the large shards that keep two blocks per CU, 0.1188-0.1202 against 0.1197-0.1214; a rank of eight stays with the fixed
    // deal, 0.0258-0.0265 against 0.0266-0.0293)
    const bool dyn = in.scan_deal == 2 ||
                     (in.scan_deal == 0 && in.nitems >= 2u * p.grid.nlists && (!in.several_slots || in.ncells > 32768u));
    const int k16 = in.k == 16 ? 16 : 0;
    if (in.rows_u8)   // 8-bit rows (per-cell or bin frames): items from the block's counter only — the fixed deal's form of this
                      // kernel holds 8 bytes of scratch under the register cap (128 in per-cell frames; 80 for the one-frame
                      // scan's two blocks of 12 waves per CU in bin frames)
        p.scan = {true, k16, false, 1, in.centred, false, true};
    else if (in.centred)   // per-cell frames: lists from the match launch
        p.scan = {dyn, k16, false, 1, true, false, false};
    else if (in.kt == 2)   // 16 < k <= 30: run-time k, norms in the fragments (NIF); k 31, 32: no free K-slots — the norm window
        p.scan = {dyn, 0, false, 2, false, in.k <= KNN_NIF_MAX_K, false};
    else
        p.scan = {dyn, k16, p.self_lists, 1, false, false, false};
    // the scan's LDS limit: what its form asks for at a full batch, when that is more than the default 64 KiB (per-cell frames,
    // 16 < k <= 32)
    const size_t full = knn_cells_scan_plan(in.num_cu, 1, in.nitems, in.rec_cap, KNN_CELL_BATCH, p.self_lists, in.kt, in.centred).lds_bytes;
    p.scan_lds_limit = full > (size_t)(64u << 10) ? full : 0;
    // gated on the device: the whole shard exactly when the batch has a query nothing bounds (k = 16: inside the tail kernel)
    p.exact_launch = in.k != 16;
    p.tail_k = in.kt == 1 && (in.k == 16 || in.k == 8) ? in.k : 0;
    p.tail_kt = in.kt;
    p.tail_blocks = (unsigned)in.num_cu * 8u;
    if (p.tail_blocks * KNN_WAVES > in.nitems)
        p.tail_blocks = std::max(2u, (in.nitems + KNN_WAVES - 1u) / KNN_WAVES);
    return p;
}

// The scan's and the tail's CellSelf, according to the scan's form: the self-listing scan, per-cell frames, 8-bit rows in bin frames.
static CellSelf cells_self(const CellQueryPlan &p, const CellIndex &c, const FilterWorkspace &w, int m_padded)
{
    if (p.self_lists)
        return CellSelf{w.lo_tab, w.hi_tab, w.dup, c.sa, m_padded, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f};
    if (p.scan.ctr)
        return CellSelf{nullptr, nullptr, w.dup, 0, 0, c.cell_frame, p.scan.u8 ? c.cell_u8 : nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f};
    if (p.scan.u8)
        return CellSelf{nullptr, nullptr, w.dup, 0, 0, nullptr, nullptr, c.binw, c.bin_ratio, c.bin_er, c.bin_nmax, c.bin_w1};
    return CellSelf{};
}

// Development aid (KNN_MI355X_TRACE_CELLS, read by tools/cells_trace.py): the lists of this batch and how evenly the scan's
// waves are loaded.  Synchronises.
static hipError_t cells_trace_lists(const CellIndex &c, const FilterWorkspace &w, int m, hipStream_t s)
{
    std::vector<unsigned> hc((size_t)c.ncells), ht((size_t)c.ncells + 1);
    FTRY(hipStreamSynchronize(s));
    FTRY(hipMemcpy(hc.data(), w.cell_counts, hc.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    FTRY(hipMemcpy(ht.data(), c.tile_start, ht.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    std::vector<unsigned> sorted(hc);
    std::sort(sorted.begin(), sorted.end());
    const unsigned nwaves = w.nlists;
    std::vector<double> wl((size_t)nwaves, 0.0);
    double total = 0, biggest = 0;
    for (unsigned cell = 0; cell < c.ncells; ++cell) {
        const double steps = (double)((std::min(hc[cell], c.cap + 1u) + 31u) / 32u) * (double)(ht[cell + 1] - ht[cell]);
        wl[cell % nwaves] += steps;   // (plain order: wave w takes cells w, w + nwaves, ...; the scan's scatter spreads them)
        total += steps;
        biggest = std::max(biggest, steps);
    }
    const double wmax = *std::max_element(wl.begin(), wl.end());
    fprintf(stderr, "[knn cells] m %d: %u cells; list length min %u  p10 %u  median %u  p90 %u  max %u; tile steps %.0f in all, %.0f in the largest "
                    "cell; %u waves: %.1f steps each on average, %.0f on the busiest\n", m, c.ncells, sorted.front(), sorted[sorted.size() / 10],
            sorted[sorted.size() / 2], sorted[sorted.size() * 9 / 10], sorted.back(), total, biggest, nwaves, total / nwaves, wmax);
    return hipSuccess;
}

// Where the prep kernel finds the seed tiles of other ranks' cells: the attached seed layer of a cell-range shard; all zero for
// every other index and for a shard nothing is attached to (its bounds then come from its own rows).
static SeedLayer cells_seed_layer(const CellIndex &c)
{
    SeedLayer layer;
    memset(&layer, 0, sizeof layer);
    if (c.geom && c.seed_layer) {
        layer.base = c.seed_layer;
        layer.cpr = c.geom->cells_per_rank;
        layer.tiles = (unsigned)c.geom->seed_tiles;
        layer.nranks = (unsigned)c.geom->nranks;
        for (int r_ = 0; r_ <= c.geom->nranks && r_ <= KNN_MAX_RANKS; ++r_)
            layer.first[r_] = c.geom->first_cell(r_);
        layer.part_bytes = c.geom->part_bytes();
    }
    return layer;
}

// The front half of every cell-pruned pass — a 1-NN batch, a top-K pass, a count pass of <= KNN_CELL_BATCH queries —: the
// slot's workspace and the kernels' LDS limits, the plan's record-list sizes into the workspace, the pass's control words, then
// prep -> match (when the plan has a match launch) -> scan, the scan between the slot's events when `timed`.  b: the driver's
// part of the batch, on workspace w (= b.w); m_padded, self and ctl_next are filled in here.  Behind it the driver finds the
// scan's records in w, and the pass's control words at w.ctl_cur.
// The control words: the slot has two blocks of them and consecutive passes alternate — the prep kernel of a pass clears the
// other block and the record counters for the pass behind it, in every form —, so 1-NN batches, top-K passes and count passes
// may follow one another on a slot in any order: this is the one place that hands a block out.  (The words of the first pass
// were cleared at allocation.)
static hipError_t cells_pass_front(FilterWorkspace &w, CellBatch &b, const CellKernel &scan, CellPrepForm prep, bool timed)
{
    const CellQueryPlan &p = b.p;
    FTRY(ensure_cells_workspace(b.st, w, b.m, p, scan));
    b.m_padded = (b.m + 31) / 32 * 32;
    w.has_rows = false;
    w.pieces = RerankPieces();
    w.nlists = p.grid.nlists;
    w.ovf_cap = p.grid.ovf_cap;
    w.ovf_base = p.grid.ovf_base;
    w.slice = p.grid.slice;
    const unsigned parity = w.cell_batches++ & 1u;
    w.ctl_cur = w.ctl + KNN_CTL_WORDS * (1u + parity);
    b.ctl_next = w.ctl + KNN_CTL_WORDS * (2u - parity);
    b.self = cells_self(p, b.c, w, b.m_padded);
    cells_prep_kernel(prep, p).launch(b);
    FTRY(hipGetLastError());
    if (p.match_waves)
        cells_match_kernel(p.match_waves).launch(b);
    FTRY(hipGetLastError());
    static const bool trace_cells = getenv("KNN_MI355X_TRACE_CELLS") != nullptr;   // (read once: a query may run beside a thread that changes the environment)
    if (trace_cells && !p.self_lists)
        FTRY(cells_trace_lists(b.c, w, b.m, b.s));
    if (timed && w.ev_begin)
        FTRY(hipEventRecord(w.ev_begin, b.s));
    scan.launch(b);
    FTRY(hipGetLastError());
    if (timed && w.ev_end)
        FTRY(hipEventRecord(w.ev_end, b.s));
    return hipSuccess;
}

// The records a pass's scan left in the workspace, as the re-rank kernels of a top-K or a count pass read them: the waves'
// slices, the shared overflow area as a list of one, the out-of-box rows, the layout's norms by position.
static TopkRecords cells_pass_records(const FilterState &st, const FilterWorkspace &w)
{
    TopkRecords rs;
    rs.positions = st.ntiles * 32;
    rs.rec = w.records;
    rs.counts = w.counts;
    rs.nlists = w.nlists;
    rs.slice = w.slice;
    rs.ctl = w.ctl_cur;
    rs.perm = st.cells->perm;
    rs.n_outliers = st.n_outliers;
    rs.outliers = st.outliers;
    rs.ovf_rec = w.records + w.ovf_base;
    rs.ovf_count = w.ctl_cur + KNN_CTL_RECORDS;
    rs.ovf_slice = w.ovf_cap;
    rs.pos_norms = st.ref_norms;
    return rs;
}

// One batch of <= KNN_CELL_BATCH queries, the whole chain: prep -> match -> scan (its waves re-rank their own records) ->
// [rows outside the robust box, exactly] -> the exact scan of the shard, gated on FALLBACK -> the tail kernel (gated: records
// in the shared area, the listed pairs exactly when that area is over-full, the finalisation when the scan could not do it).
// Four launches on clean data at k = 16 (the exact scan of the shard is a branch of the tail kernel there), five otherwise.  out_idx (nullable): int32 indices of the batch, written by whichever block ends it.
hipError_t knn_cells_query(FilterState &st, FilterWorkspace &w, FilterCallOptions opt, int m, const float *q, const float *r,
                           long long base, u64 *keys, int num_cu, bool timed, hipStream_t s, bool init_keys, int *out_idx)
{
    const CellIndex &c = *st.cells;
    const CellQueryPlan p = knn_cells_query_plan({st.k, st.kt, c.centred, c.rows_u8, c.ncells, c.nitems, c.cap, opt.several_slots,
                                                  opt.scan_blocks, opt.scan_deal, opt.cells_lists, m, num_cu, w.rec_cap});
    CellBatch b{st, c, w, p, m, q, r, base, keys, init_keys ? keys : nullptr, CellFinal{c.gids, out_idx, st.n_outliers != 0u ? 1 : 0},
                cells_seed_layer(c), s};
    FTRY(cells_pass_front(w, b, cells_scan_kernel(p.scan), CellPrepForm::Nearest, timed));
    // rows outside the robust box never entered the layouts: exact scan of that (short) list
    FTRY(knn_exact_gather_launch(st.k, m, st.n_outliers, base, q, r, st.outliers, keys, num_cu, nullptr, s));
    if (p.exact_launch)
        FTRY(knn_exact_launch(st.k, m, st.n, base, q, r, keys, num_cu, w.ctl_cur + KNN_CTL_FALLBACK, s));
    cells_tail_launch(b);
    return hipGetLastError();
}

// Top-K on the cell-pruned scan: whether a call takes it and everything one of its passes launches with (host arithmetic:
// nothing allocated or launched; tests/test_cells_topk_logic.py checks it on the CPU through knn_debug_cells_topk_plan).
// Served: a resident, non-sharded index whose cell-sorted layout is in the shard's frame — fp16 rows not centred, or 8-bit rows in
// bin frames —, k <= 32, m >= 5, out-of-box rows at most half a query's candidate room; and a cell-range shard (always fp16, not
// centred, KT 1) under the same conditions when the call carries KNN_QUERY_TOPK_PARTIAL (shard_partial: the lists are then what
// the global top-K needs of this rank, not the rank's own top-K) and topk_cells is 1.  Per-cell frames (fp16 centred, or 8-bit rows in
// each cell's own frame; k <= 16, not sharded): under the same conditions when the call carries KNN_QUERY_TOPK_FRAMES (frames_flag)
// and topk_cells is 1 — the pass then has the per-cell-frame prep form and scan grid (prep_ctr, scan.ctr: knn_cells_query_plan's
// choice for a centred layout).  Not served (they keep the exact top-K): per-cell frames without the flag, cell-range shards
// without theirs, grid indexes, m < 5.
// Policy (topk_cells = 0): declines for now (see below); topk_cells = 1 serves every such call.
CellTopkPlan knn_cells_topk_plan(const CellTopkInputs &in)
{
    CellTopkPlan t;
    const CellQueryInputs &qi = in.q;
    if (in.K < 1 || in.K > KNN_TOPK_MAX || qi.m < 1)
        return t;
    // candidate room: the filter top-K's rule (knn_topk_ccap, from the caller).  The K-th seed bound admits about K times the 1-NN
    // bound's rows, nearly each its own record, but the re-rank's distance gate (knn_topk_gate) lets about one key of a record's
    // sixteen through
    t.ccap = in.ccap;
    // per-cell frames (fp16 centred, or 8-bit rows in each cell's own frame): only for a call that carries KNN_QUERY_TOPK_FRAMES
    const bool frames = qi.centred && in.frames_flag && !in.sharded && !in.bins && qi.kt == 1 && qi.k <= 16;
    const bool one_frame = !qi.centred && (!qi.rows_u8 || in.bins);
    const bool layout = in.has_cells && (!in.sharded || in.shard_partial) && !in.other_path && (frames || one_frame) && qi.kt >= 1 &&
                        qi.kt <= 2 && qi.k <= 32;
    const bool call = qi.m >= 5 && t.ccap >= 64u && in.n_outliers <= t.ccap / 2u;
    // Policy (0) declines every call for now: the issue's condition for sending a (shape, K) to this path by default is a measured
    // win over the path it replaces, and those A/B figures (profiles/r13_cells_topk.txt) are not taken yet.  Where it will start
    // once they are: `policy_from`, the 1-NN size rule of k, and never under `cells` = 2.
    const bool policy_measured = false;
    const bool policy_from = in.cells_option != 2 && in.n >= knn_cells_size_rule(qi.k);
    // (a cell-range shard: on request only — nobody has measured either side there, profiles/shard_topk_timing.txt will)
    const bool policy = in.topk_cells == 1 || (in.topk_cells == 0 && !in.sharded && policy_measured && policy_from);
    t.use = layout && call && policy && in.topk_cells != 2;
    if (!t.use)
        return t;
    t.passes = (qi.m + KNN_CELL_BATCH - 1) / KNN_CELL_BATCH;
    t.pass_m = std::min(qi.m, KNN_CELL_BATCH);
    // a pass is a 1-NN batch up to the scan: the same prep shape, match launch, grid, record lists and LDS — with the match
    // launch always (the self-listing scan has no record-only form)
    CellQueryInputs bi = qi;
    bi.m = t.pass_m;
    bi.cells_lists = 1;
    t.batch = knn_cells_query_plan(bi);
    t.scan = t.batch.scan;
    t.scan.k = 0;   // (no inline re-rank: one instantiation per shape)
    return t;
}

// The passes of a count call (knn_index_count_within on the cell-pruned way): the top-K pass plan at K = 1 on a one-frame layout —
// prep shape, match launch, the record-only scan's grid and lists.  knn_count_route has chosen the way; here only the shapes are
// made (use false: the layout has none), and knn_cells_query_count's guard holds the pass to them.
CellTopkPlan knn_cells_count_plan(const CellTopkInputs &in)
{
    CellTopkInputs t = in;
    t.K = 1;
    t.topk_cells = 1;
    t.shard_partial = t.sharded;
    t.frames_flag = false;
    t.other_path = false;
    t.n_outliers = 0u;   // (a count has no candidate list for them to crowd)
    t.ccap = 64u;
    return knn_cells_topk_plan(t);
}

hipError_t knn_cells_query_topk(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const TopkCall &call)
{
    const CellIndex &c = *st.cells;
    const CellQueryPlan &p = tp.batch;
    const int m = call.m;
    hipStream_t s = call.stream;
    if (!tp.use || m > tp.pass_m || tp.scan.self || tp.scan.ctr != c.centred || p.prep_ctr != c.centred || call.ccap != tp.ccap ||
        call.gids != c.gids || (c.geom && (!c.gids || call.base != 0)))
        return hipErrorInvalidValue;
    // A cell-range shard (KNN_QUERY_TOPK_PARTIAL): the K-th seed bound over the rows of the GLOBAL set the seed layer reaches — the
    // prep kernel scores a seed cell of another rank from the layer's tiles, as the 1-NN form does —, and gids on the keys from the
    // moment they are candidates (the select sorts them, a fold compares them with other ranks'): CellFinal stays empty, nothing is
    // translated behind the select, while a 1-NN batch on the same slot keeps translating in its own last kernel.
    CellBatch b{st, c, w, p, m, call.q, call.r, call.base, call.keys, nullptr, CellFinal{nullptr, nullptr, 0}, cells_seed_layer(c), s,
                call.K, call.max_dist2};
    FTRY(hipMemsetAsync(call.ccount, 0, (size_t)m * sizeof(unsigned), s));
    FTRY(cells_pass_front(w, b, cells_records_kernel(tp.scan), call.max_dist2 < INFINITY ? CellPrepForm::TopkWithin : CellPrepForm::Topk,
                          timed));
    // every row of every record with v0's arithmetic -> the queries' candidate lists, behind the distance gate knn_topk_gate(Dup_q)
    // (the slices, then the shared overflow area as a list of one), the out-of-box rows, the select; all of them look at FALLBACK, which a query nothing bounds, fewer than K
    // real seed rows, an over-full record area or candidate list raise
    TopkRecords rs = cells_pass_records(st, w);
    rs.gate_dup = w.dup;
    rs.inv_sigma2 = (float)(1.0 / ((double)st.sigma * (double)st.sigma));
    FTRY(knn_topk_filter_finish(call, rs));
    // gated: the exact top-K answers a pass that raised FALLBACK; it folds into the keys the select left alone (no limit: the caller
    // clips a radius call's lists)
    return knn_exact_topk_launch(call, w.ctl_cur + KNN_CTL_FALLBACK, false);
}

// One pass of <= KNN_CELL_BATCH queries of a count call (knn_index_count_within with KNN_QUERY_COUNT_CELLS; DESIGN §4.6 "Counts
// within a radius"): count prep (the radius cap alone: no seed scoring) -> match -> record-only scan, both unchanged -> count
// re-rank of the slices and of the shared overflow area -> out-of-box rows -> commit, gated on no FALLBACK -> the exact count,
// gated on FALLBACK.  call.scratch (the pass's part of the slot's count scratch) is zero on entry.
hipError_t knn_cells_query_count(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const CountCall &call)
{
    const CellIndex &c = *st.cells;
    const CellQueryPlan &p = tp.batch;
    const int m = call.m;
    if (!tp.use || m > tp.pass_m || tp.scan.self || tp.scan.ctr || c.centred || p.prep_ctr || !(call.max_dist2 < INFINITY) || !call.scratch)
        return hipErrorInvalidValue;
    // (no keys, no gids, the empty seed layer: counts of a cell-range shard are its own rows' and simply add across ranks)
    const SeedLayer no_layer = {nullptr, 0u, 0u, 0u, 0ull, {0u}};
    CellBatch b{st, c, w, p, m, call.q, call.r, 0ll, nullptr, nullptr, CellFinal{nullptr, nullptr, 0}, no_layer, call.stream, 1, call.max_dist2};
    b.radii = call.radii;
    FTRY(cells_pass_front(w, b, cells_records_kernel(tp.scan), call.radii ? CellPrepForm::CountEach : CellPrepForm::Count, timed));
    FTRY(knn_count_records_finish(call, cells_pass_records(st, w), call.scratch));
    // gated: the exact count — a routed self call: the self-scan, a masked one: the masked scan — answers a pass that raised FALLBACK (its scratch was not committed)
    return knn_gated_count_launch(call, w.ctl_cur + KNN_CTL_FALLBACK);
}

// One pass of <= KNN_CELL_BATCH own rows of a cluster call's link sweep (knn_index_self_cluster_within_routed with
// KNN_QUERY_COUNT_CELLS; DESIGN §4.6 "Clusters on the cell-pruned way"): the count pass unchanged up to its finish — count prep ->
// match -> record-only scan, Q = R + first * k —, then the link re-rank of the slices and of the shared overflow area -> out-of-box
// rows (knn_cluster_routed.hip; nothing to commit) -> the exact link sweep of the pass's window, gated on FALLBACK.
hipError_t knn_cells_cluster_link(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const ClusterPass &pass)
{
    const CellIndex &c = *st.cells;
    const CellQueryPlan &p = tp.batch;
    const ClusterCall &call = pass.c;
    const int m = pass.m;
    if (!tp.use || m < 1 || m > tp.pass_m || tp.scan.self || tp.scan.ctr || c.centred || p.prep_ctr || !(call.max_dist2 < INFINITY) ||
        call.n != st.n || call.k != st.k || pass.first < 0 || pass.first + m > call.n)
        return hipErrorInvalidValue;
    const SeedLayer no_layer = {nullptr, 0u, 0u, 0u, 0ull, {0u}};
    CellBatch b{st, c, w, p, m, call.r + (size_t)pass.first * call.k, call.r, 0ll, nullptr, nullptr, CellFinal{nullptr, nullptr, 0}, no_layer,
                call.stream, 1, call.max_dist2};
    FTRY(cells_pass_front(w, b, cells_records_kernel(tp.scan), CellPrepForm::Count, timed));
    FTRY(knn_cluster_link_records_finish(pass, cells_pass_records(st, w)));
    // gated: the exact sweep of the window answers a pass that raised FALLBACK, over whatever the record kernels left
    return knn_cluster_link_window_launch(call, pass.first, m, w.ctl_cur + KNN_CTL_FALLBACK);
}

// One pass of <= KNN_CELL_BATCH queries of a list call (knn_index_list_within with KNN_QUERY_COUNT_CELLS; DESIGN §4.6 "Lists within
// a radius"): the count pass unchanged up to its finish — count prep -> match -> record-only scan —, then the list re-rank of the
// slices and of the shared overflow area -> out-of-box rows, all reserving in call.scratch (on entry a copy of call.fill) and
// storing behind it -> commit, gated on no FALLBACK -> the exact list, gated on FALLBACK, from the untouched call.fill.
hipError_t knn_cells_query_list(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const ListCall &call)
{
    const CellIndex &c = *st.cells;
    const CellQueryPlan &p = tp.batch;
    const int m = call.m;
    if (!tp.use || m > tp.pass_m || tp.scan.self || tp.scan.ctr || c.centred || p.prep_ctr || !(call.max_dist2 < INFINITY) || !call.scratch ||
        call.gids != c.gids || (c.geom && (!c.gids || call.base != 0)))
        return hipErrorInvalidValue;
    // (the empty seed layer: the lists of a cell-range shard are its own rows' and simply append across ranks)
    const SeedLayer no_layer = {nullptr, 0u, 0u, 0u, 0ull, {0u}};
    CellBatch b{st, c, w, p, m, call.q, call.r, 0ll, nullptr, nullptr, CellFinal{nullptr, nullptr, 0}, no_layer, call.stream, 1, call.max_dist2};
    b.radii = call.radii;
    FTRY(cells_pass_front(w, b, cells_records_kernel(tp.scan), call.radii ? CellPrepForm::CountEach : CellPrepForm::Count, timed));
    FTRY(knn_list_records_finish(call, cells_pass_records(st, w)));
    // gated: the exact list — a routed self call: the self-scan, a masked one: the masked scan — answers a pass that raised
    // FALLBACK (its scratch cursor was not committed)
    return knn_gated_list_launch(call, w.ctl_cur + KNN_CTL_FALLBACK);
}

// Test hook (host arithmetic, no GPU): knn_threshold's Dup for a seed score u — out = {thr, Dup as the prep kernel stores it (fp32,
// rounded up), knn_topk_gate of that Dup: the largest v0 distance a top-K row can have}.
extern "C" int knn_debug_topk_gate(int k, float sigma, double amax, double bmax, double nmax, double u, double mq, double out[3])
{
    if (k < 1 || k > 32 || !(sigma > 0.0f) || !out)
        return -1;   // KNN_EINVAL
    const BoundConsts cst = knn_bound_consts(k, knn_kt_of(k), sigma, amax, bmax, nmax);
    double dup = 0.0;
    out[0] = knn_threshold(cst, u, mq, &dup);
    dup *= 1.0 + 1e-6;
    float dupf = (float)dup;
    if ((double)dupf < dup)
        dupf = nextafterf(dupf, INFINITY);
    out[1] = dupf;
    out[2] = knn_topk_gate(dupf, (float)(1.0 / ((double)sigma * (double)sigma)));
    return 0;
}

// Test hook (host arithmetic, no GPU): the same three values for a radius call — knn_threshold_within's threshold and capped Dup as
// the prep kernel's WR form stores it, and the re-rank's gate of that Dup (slightly above max_dist2 where the radius binds: the
// exact cut is the clip's).  A query nothing bounds (u and max_dist2 both +INF) gives {+INF, +INF, +INF}.
extern "C" int knn_debug_within_bound(int k, float sigma, double amax, double bmax, double nmax, double u, double mq, float max_dist2,
                                      double out[3])
{
    if (k < 1 || k > 32 || !(sigma > 0.0f) || !(max_dist2 >= 0.0f) || !out)
        return -1;   // KNN_EINVAL
    const BoundConsts cst = knn_bound_consts(k, knn_kt_of(k), sigma, amax, bmax, nmax);
    double dup = 0.0;
    out[0] = knn_threshold_within(cst, u, mq, max_dist2, &dup);
    dup *= 1.0 + 1e-6;
    float dupf = (float)dup;
    if ((double)dupf < dup)
        dupf = nextafterf(dupf, INFINITY);
    out[1] = dupf;
    out[2] = knn_topk_gate(dupf, (float)(1.0 / ((double)sigma * (double)sigma)));
    return 0;
}

// Test hook (host arithmetic, no GPU): the prep kernel's K-th seed score (knn_seed_kth.h) of `nseed` seed scores and `nwide`
// scores of the wide sample (32 per tile, padded with +INF here), as a block of `pw` waves selects it.
extern "C" int knn_debug_seed_kth(const float *seed, int nseed, const float *wide, int nwide, int K, int pw, float *out)
{
    if (nseed < 0 || nwide < 0 || (nseed && !seed) || (nwide && !wide) || K < 1 || K > KNN_TOPK_MAX || (pw != 2 && pw != 4) || !out)
        return -1;   // KNN_EINVAL
    std::vector<float> a((size_t)(nseed + 31) / 32 * 32, INFINITY), b((size_t)(nwide + 31) / 32 * 32, INFINITY);
    std::copy(seed, seed + nseed, a.begin());
    std::copy(wide, wide + nwide, b.begin());
    *out = knn_seed_kth_host(a.data(), (int)a.size() / 32, b.data(), (int)b.size() / 32, K, pw);
    return 0;
}

// Test hook (host arithmetic, no GPU): the per-cell-frame top-K prep form's conversion of one seed score (knn_frame_dup.h: the
// kernel's own lines) for one cell frame and one fp32 query row — out = {Dup in the shard's units, 1 if far}.
extern "C" int knn_debug_frame_dup(int k, const float frame[KNN_CELL_FRAME_WORDS], const float *query_row, float u, float out[2])
{
    if (k < 1 || k > 16 || !frame || !query_row || !out || !(frame[16] > 0.0f) || !(frame[17] > 0.0f))
        return -1;   // KNN_EINVAL
    float fr[KNN_CELL_FRAME_WORDS];
    std::copy(frame, frame + KNN_CELL_FRAME_WORDS, fr);
    _Float16 b[16];
    const KnnFrameQuery fq = knn_frame_query(k, fr, query_row, b);
    out[0] = fabsf(u) < INFINITY ? knn_frame_dup(k, fr[16], fr[17], fr[18], fr[19], fq, u) : INFINITY;   // (the kernel converts finite scores only)
    out[1] = fq.far ? 1.0f : 0.0f;
    return 0;
}

// Test hook (host arithmetic, no GPU): one row through the 8-bit rows' quantiser (knn_u8_code — what knn_cells_recentre_kernel
// does per coordinate, v = (row - centre) x scale in fp32) -> its codes, the largest per-coordinate err and the eta of
// knn_bound_consts_u8(k, 1, scale, amax, err, nmax) for a query of largest |coordinate| amax.
extern "C" int knn_debug_u8_row(int k, const float *row, const float *centre, float scale, double amax, unsigned char *codes,
                                double out[2])
{
#pragma clang fp contract(off)
    if (k < 1 || k > 16 || !row || !centre || !codes || !out)
        return -1;   // KNN_EINVAL
    float er = 0.0f, nmax = 0.0f;
    for (int d = 0; d < k; ++d) {
        const float v = (row[d] - centre[d]) * scale;
        float rh, e;
        codes[d] = (unsigned char)knn_u8_code(v, rh, e);
        er = std::max(er, e);
        nmax = nmax + rh * rh;
    }
    out[0] = er;
    out[1] = knn_bound_consts_u8(k, 1, scale, amax, er, nmax).eta;
    return 0;
}

// Test hooks (host arithmetic, no GPU) for the 8-bit rows in bin frames.  knn_debug_u8_bin_row: one row through knn_u8_bin_code
// (what knn_cells_bin_rows_kernel does per coordinate) with the centre of the shard's frame, the scale sigma 2^e and the cell's
// offsets w -> its codes and the largest err.  knn_debug_u8_bin_threshold: knn_u8_bin_threshold of one query given its fp16 B
// operand in the bins' units (16 values, as bits).
extern "C" int knn_debug_u8_bin_row(int k, const float *row, const float *centre, float scale, const float *w, unsigned char *codes,
                                    double *err)
{
    if (k < 1 || k > 16 || !row || !centre || !w || !codes || !err)
        return -1;   // KNN_EINVAL
    float er = 0.0f;
    for (int d = 0; d < k; ++d) {
        float rh, e;
        codes[d] = (unsigned char)knn_u8_bin_code(row[d], centre[d], scale, w[d], rh, e);
        er = std::max(er, e);
    }
    *err = er;
    return 0;
}

extern "C" int knn_debug_u8_bin_threshold(int k, const unsigned short *b_bits, float dup, float ratio, float er, float nmax, float w1,
                                          float *thr)
{
    if (k < 1 || k > 16 || !b_bits || !thr)
        return -1;   // KNN_EINVAL
    h8 b0, b1;
    for (int j = 0; j < 8; ++j) {
        b0[j] = __builtin_bit_cast(_Float16, b_bits[j]);
        b1[j] = __builtin_bit_cast(_Float16, b_bits[8 + j]);
    }
    *thr = knn_u8_bin_threshold(k, b0, b1, dup, ratio, er, nmax, w1);
    return 0;
}
