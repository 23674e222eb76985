// knn_masked.hip — queries over a subset of the rows (include/knn_mi355x.h 2g; DESIGN §4.6 "Over a subset of the rows"):
// knn_index_query_topk_masked, knn_index_count_within_masked, knn_mask_set_rows.
//
// The subset is a bit mask over the shard's local rows: bit i % 32 of word i / 32 admits row i.  The two scans are the skeletons of
// knn_exact_topk_kernel<KC, true> and knn_exact_count_kernel<KC> (knn_exact.hip) — one wave per block, lanes = queries, rows as
// wave-uniform scalar loads, v0's arithmetic — with one change in the row loop: the block walks the mask words of its slice, four
// at a time, and visits the set bits of every non-zero word in ascending order.  The mask words, the bit positions and the row
// addresses are wave-uniform: a zero word costs no row load, a set bit costs what a row costs the unmasked scan.  A granule of 1024 rows
// that admits nothing is not walked at all: the walk jumps over runs of them through the prefix below.
//
// Slices hold equal numbers of ADMITTED rows (knn_mask_split.h).  A call first counts the admitted rows of every granule of 1024
// rows and turns the counts into a 64-bit exclusive prefix (knn_counts_to_offsets_kernel); block b of S finds the granule its cut
// falls into from the prefix by a binary search every lane performs identically, and the row inside it from that granule's 32
// words — no host synchronisation, and S is the unmasked scan's number, so the slot's per-slice lists are sized as before.  A mask is the
// caller's and may change between calls: nothing is kept.
//
// Behind a pruned way of a routed masked call (2l) the count's whole sequence is gated on a device word: every kernel of it — the
// granule counts, the prefix (a gated twin of knn_counts_to_offsets_kernel around the same block body), the scan — returns at once
// unless *gate != 0, so the query path never synchronises with the host.  gate null: the launches of 2g, unchanged.
#include "knn_masked_dev.h"
#include "knn_slice_launch.h"

// counts[g] <- the admitted rows of granule g: one mask word per thread (bits at and beyond n dropped), a granule per 32 lanes.
__global__ __launch_bounds__(KNN_BLOCK) void knn_mask_granule_counts_kernel(const unsigned *__restrict__ mask, long long n, long long G,
                                                                           unsigned *__restrict__ counts,
                                                                           const unsigned *__restrict__ gate)
{
    if (gate && *gate == 0u)
        return;
    const long long w = (long long)blockIdx.x * KNN_BLOCK + threadIdx.x;
    const unsigned v = knn_mask_word(mask, n, w);
    unsigned c = (unsigned)__popc(v);
#pragma unroll
    for (int off = KNN_MASK_GRANULE_WORDS / 2; off > 0; off >>= 1)
        c += __shfl_xor(c, off, KNN_MASK_GRANULE_WORDS);
    const long long g = w / KNN_MASK_GRANULE_WORDS;
    if ((threadIdx.x & (KNN_MASK_GRANULE_WORDS - 1)) == 0 && g < G)
        counts[g] = c;
}

// knn_counts_to_offsets_kernel behind a gate: the prefix of the granule counts of a gated masked scan.  One block.
__global__ __launch_bounds__(KNN_BLOCK) void knn_mask_prefix_gated_kernel(const unsigned *__restrict__ counts, int m,
                                                                         u64 *__restrict__ offsets, const unsigned *__restrict__ gate)
{
    if (*gate == 0u)   // (block-uniform: every thread leaves, or every thread reaches the block's barriers)
        return;
#include "knn_counts_to_offsets_body.inc"
}

// The mask bit of every listed row in 0 .. n - 1 <- value: one atomic on the row's word (rows may repeat and share words).
__global__ __launch_bounds__(KNN_BLOCK) void knn_mask_set_rows_kernel(long long n, const unsigned *__restrict__ rows, long long count,
                                                                     int value, unsigned *__restrict__ mask)
{
    const long long stride = (long long)gridDim.x * KNN_BLOCK;
    for (long long i = (long long)blockIdx.x * KNN_BLOCK + threadIdx.x; i < count; i += stride) {
        const unsigned row = rows[i];
        if ((long long)row >= n)
            continue;
        const unsigned bit = 1u << (row & 31u);
        if (value)
            atomicOr(&mask[row >> 5], bit);
        else
            atomicAnd(&mask[row >> 5], ~bit);
    }
}

// knn_masked_topk_kernel<KC> — knn_exact_topk_kernel<KC, true> over the admitted rows of the block's slice: the sorted LDS column,
// the K-th key in a register and the min(column[K - 1], lim) rule as there (lim = KNN_KEY_INIT: no radius).  An empty slice writes
// a padding list.  grid = (slices, query groups of 64).
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_masked_topk_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                  int m, long long n, int K, const unsigned *__restrict__ mask,
                                                                  const u64 *__restrict__ P, int G, long long base,
                                                                  const unsigned *__restrict__ gids, u64 *__restrict__ part, u64 lim)
{
#pragma clang fp contract(off)
    extern __shared__ u64 masked_lst[];   // [K][KNN_WAVE]
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    for (int t = 0; t < K; ++t)
        masked_lst[t * KNN_WAVE + lane] = kKeyInit;
    u64 kth = lim < kKeyInit ? lim : kKeyInit;
    const float *__restrict__ qp = Q + (size_t)qa * k;
    long long r0, r1;
    masked_slice(mask, n, P, G, r0, r1);
    masked_walk(mask, P, G, r0, r1, [&](long long i) {
        const float acc = lane_row_dist2<KC>(qv, qp, R + (size_t)i * k, k);
        const u64 key = pack_key(acc, (unsigned)i);
        if (key < kth) {
            int p = K - 1;
            while (p > 0) {
                const u64 prev = masked_lst[(p - 1) * KNN_WAVE + lane];
                if (prev < key)
                    break;
                masked_lst[p * KNN_WAVE + lane] = prev;
                --p;
            }
            masked_lst[p * KNN_WAVE + lane] = key;
            kth = masked_lst[(K - 1) * KNN_WAVE + lane];
            kth = kth < lim ? kth : lim;
        }
    });
    if (q >= m)
        return;
    u64 *__restrict__ out = part + ((size_t)blockIdx.x * m + q) * K;
    for (int t = 0; t < K; ++t) {
        const u64 key = masked_lst[t * KNN_WAVE + lane];
        const unsigned row = (unsigned)key;
        const bool real = (key >> 32) < 0x7F800000ull;
        const unsigned g = gids ? (real ? gids[row] : 0u) : (unsigned)(base + (long long)row);
        out[t] = real ? ((key & 0xFFFFFFFF00000000ull) | (u64)g) : kKeyInit;
    }
}

// knn_masked_count_kernel<KC> — knn_exact_count_kernel<KC> over the admitted rows of the block's slice: one counter per lane, one
// atomicAdd at the end when it is not zero.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_masked_count_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                   int m, long long n, const unsigned *__restrict__ mask,
                                                                   const u64 *__restrict__ P, int G, float max_dist2,
                                                                   unsigned *__restrict__ counts, const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    unsigned cnt = 0u;
    const float *__restrict__ qp = Q + (size_t)qa * k;
    long long r0, r1;
    masked_slice(mask, n, P, G, r0, r1);
    masked_walk(mask, P, G, r0, r1, [&](long long i) {
        const float acc = lane_row_dist2<KC>(qv, qp, R + (size_t)i * k, k);
        cnt += acc < INFINITY && acc <= max_dist2 ? 1u : 0u;   // (NaN fails both compares)
    });
    if (q < m && cnt != 0u)
        atomicAdd(&counts[q], cnt);
}

MaskedPlan knn_masked_plan(int k, int m, int K, long long n, int num_cu, bool init)
{
    MaskedPlan p;
    if (m <= 0)
        return p;
    const SlicePlan sp = knn_slice_plan(m, K, n, num_cu);   // (the unmasked scan's chunks, slices, LDS and per-slice lists)
    p.chunk_m = sp.chunk_m;
    p.chunks = sp.chunks;
    if (n <= 0) {   // an empty shard: an init top-K fills the keys, everything else launches nothing
        p.launches = K > 0 && init ? 1 : 0;
        return p;
    }
    p.granules = (n + KNN_MASK_GRANULE_ROWS - 1) / KNN_MASK_GRANULE_ROWS;
    p.slices = sp.slices;
    p.lds_bytes = sp.lds_bytes;
    p.counts_off = (size_t)(p.granules + 1) * sizeof(u64);
    p.mask_bytes = p.counts_off + (((size_t)p.granules * sizeof(unsigned) + 7) & ~(size_t)7);
    p.part_bytes = sp.part_bytes;
    p.launches = 2 + (long long)p.chunks * (K > 0 ? 2 : 1);
    return p;
}

namespace {
// counts and prefix of the call's mask into the slot's scratch: once per call, ahead of every chunk's scan
hipError_t masked_prefix_launch(const MaskedPlan &p, long long n, const unsigned *mask, u64 *scratch, hipStream_t s,
                                const unsigned *gate = nullptr)
{
    unsigned *counts = (unsigned *)((char *)scratch + p.counts_off);
    const long long words = p.granules * KNN_MASK_GRANULE_WORDS;
    hipLaunchKernelGGL(knn_mask_granule_counts_kernel, dim3((unsigned)knn_divup(words, KNN_BLOCK)), dim3(KNN_BLOCK), 0, s, mask, n,
                       p.granules, counts, gate);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (!gate)
        return knn_counts_to_offsets_launch(counts, (int)p.granules, scratch, s);
    hipLaunchKernelGGL(knn_mask_prefix_gated_kernel, dim3(1), dim3(KNN_BLOCK), 0, s, (const unsigned *)counts, (int)p.granules, scratch, gate);
    return hipGetLastError();
}
}  // namespace

hipError_t knn_masked_prefix_launch(const MaskedPlan &p, long long n, const unsigned *mask, u64 *scratch, hipStream_t s,
                                    const unsigned *gate)
{
    if (n <= 0 || !mask || !scratch || p.granules > (1ll << 22))
        return hipErrorInvalidValue;
    return masked_prefix_launch(p, n, mask, scratch, s, gate);
}

hipError_t knn_masked_topk_launch(const TopkCall &c, const MaskedPlan &p, const unsigned *mask, u64 *scratch)
{
    const int K = c.K;
    hipStream_t s = c.stream;
    if (c.m <= 0 || c.n <= 0 || K < 1 || K > KNN_TOPK_MAX || !mask || !scratch || p.granules > (1ll << 22))
        return hipErrorInvalidValue;
    hipError_t e = masked_prefix_launch(p, c.n, mask, scratch, s);
    if (e != hipSuccess)
        return e;
    if (c.ev0 && (e = hipEventRecord(c.ev0, s)) != hipSuccess)
        return e;
    const u64 lim = c.limit_key();
    e = knn_slice_chunks(c.m, c.n, c.num_cu, KnnTopkSlices{K}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        if (KnnTopkSlices{K}.part_bytes(ch.slices, mc) > c.part_bytes)
            return hipErrorInvalidValue;
        const dim3 grid = ch.grid, block(KNN_WAVE);
        const size_t lds = KnnTopkSlices{K}.lds_bytes();
        const float *qc = c.q + (size_t)ch.c0 * c.k;
#define KNN_MASKED_TOPK(KCV)                                                                                                    \
    hipLaunchKernelGGL(knn_masked_topk_kernel<KCV>, grid, block, lds, s, qc, c.r, c.k, mc, c.n, K, mask, (const u64 *)scratch, \
                       (int)p.granules, c.base, c.gids, c.part, lim)
        KNN_KC_SWITCH(c.k, KNN_MASKED_TOPK)
#undef KNN_MASKED_TOPK
        const hipError_t el = hipGetLastError();
        if (el != hipSuccess)
            return el;
        return knn_topk_select_launch(c.part, (int)ch.slices, mc, K, c.keys + (size_t)ch.c0 * K, c.init, s);
    });
    if (e != hipSuccess)
        return e;
    if (c.ev1 && (e = hipEventRecord(c.ev1, s)) != hipSuccess)
        return e;
    return hipSuccess;
}

hipError_t knn_masked_count_launch(const CountCall &c, const MaskedPlan &p, const unsigned *mask, u64 *scratch, const unsigned *gate)
{
    hipStream_t s = c.stream;
    if (c.m <= 0 || c.n <= 0 || !mask || !scratch || p.granules > (1ll << 22) || c.radii || c.self_first >= 0)
        return hipErrorInvalidValue;
    hipError_t e = masked_prefix_launch(p, c.n, mask, scratch, s, gate);
    if (e != hipSuccess)
        return e;
    if (!gate && c.ev0 && (e = hipEventRecord(c.ev0, s)) != hipSuccess)
        return e;
    e = knn_slice_chunks(c.m, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const dim3 grid = ch.grid, block(KNN_WAVE);
        const float *qc = c.q + (size_t)ch.c0 * c.k;
#define KNN_MASKED_COUNT(KCV)                                                                                                   \
    hipLaunchKernelGGL(knn_masked_count_kernel<KCV>, grid, block, 0, s, qc, c.r, c.k, mc, c.n, mask, (const u64 *)scratch,     \
                       (int)p.granules, c.max_dist2, c.counts + ch.c0, gate)
        KNN_KC_SWITCH(c.k, KNN_MASKED_COUNT)
#undef KNN_MASKED_COUNT
        return hipGetLastError();
    });
    if (e != hipSuccess)
        return e;
    if (!gate && c.ev1 && (e = hipEventRecord(c.ev1, s)) != hipSuccess)
        return e;
    return hipSuccess;
}

hipError_t knn_mask_set_rows_launch(long long n, const unsigned *rows, long long count, int value, unsigned *mask, hipStream_t s)
{
    if (count <= 0 || n <= 0)
        return hipSuccess;
    long long blocks = (count + KNN_BLOCK - 1) / KNN_BLOCK;
    if (blocks > 8192)
        blocks = 8192;
    hipLaunchKernelGGL(knn_mask_set_rows_kernel, dim3((unsigned)blocks), dim3(KNN_BLOCK), 0, s, n, rows, count, value, mask);
    return hipGetLastError();
}
