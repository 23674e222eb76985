// knn_select.hip — top-K beyond 64 (knn_index_query_topk_large; DESIGN §4.6 "Top-K beyond 64"): the exact K smallest packed keys
// per query for K up to KNN_TOPK_LARGE_MAX, on the index's fp32 rows.
//
//   select  per query the K-th smallest candidate key T, by an MSB-first radix select over the 64-bit key: per pass one scan of
//           the shard that counts, per query, the candidates under the query's prefix by their next 8 bits (the block's
//           histogram in LDS, flushed with integer atomics), and one pick launch that walks the bins (knn_radix_pick.h);
//   fill    one more scan: a candidate with key <= T reserves a place of its query's K and stores its key there;
//   sort    one block per query sorts what was stored and pads the rest with KNN_KEY_INIT;
//   fold    a call without KNN_QUERY_INIT_KEYS made its lists in the slot's scratch: one block per query merges them into the
//           caller's keys.
//
// Every scan is knn_exact_count_kernel<KC>'s loop (knn_exact.hip): lanes = queries, coordinates in VGPRs, rows as wave-uniform
// scalar loads, v0's arithmetic under fp contract(off); a candidate is a row whose distance E is finite and E <= max_dist2.
// The sequence of launches per chunk of queries is knn_select_round's (knn_slice_launch.h), shared with the select over a subset
// of the rows (knn_masked_lists.hip); this file hands it its two scans and keeps the pieces that do not look at rows.
#include "knn_exact_dev.h"
#include "knn_radix_pick.h"
#include "knn_slice_launch.h"

// One pass of the select: grid (slices, waves of queries), KNN_SELECT_WAVES waves per block.  The block's waves hold the SAME 64
// queries and split the slice's rows; a candidate whose key lies under its query's prefix adds one to hist[digit][lane] in LDS —
// bin-major, so the 64 lanes of an add fall into 64 consecutive words whatever their digits: no bank conflict.  At the end of
// the slice the non-zero bins are added to the per-query histograms ghist[bin * mcp + query]: integer atomics, the order of the
// slices does not matter.  A query that is resolved (need = 0) or beyond m takes no part.
// gate (null on pass 0): the pass returns at once unless *gate != 0 — no query was left open by the pass before.
template <int KC>
__global__ __launch_bounds__(KNN_SELECT_BLOCK) void knn_select_hist_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                          int m, long long n, long long rows_per_slice, float max_dist2,
                                                                          long long base, const unsigned *__restrict__ gids, int pass,
                                                                          const u64 *__restrict__ prefix, const unsigned *__restrict__ need,
                                                                          unsigned *__restrict__ ghist, long long mcp,
                                                                          const unsigned *__restrict__ gate)
{
    __shared__ unsigned hist[KNN_SELECT_HIST_WORDS];
    if (gate && *gate == 0u)
        return;
    for (unsigned w = threadIdx.x; w < KNN_SELECT_HIST_WORDS; w += KNN_SELECT_BLOCK)
        hist[w] = 0u;
    __syncthreads();
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x & (KNN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / KNN_WAVE));   // (uniform: the rows stay scalar loads)
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    const bool live = q < m && (pass == 0 || need[qa] != 0u);
    const u64 pre = pass == 0 ? 0ull : prefix[qa];
    // the slice, and this wave's share of it
    const long long s0 = (long long)blockIdx.x * rows_per_slice;
    const long long s1 = min(n, s0 + rows_per_slice);
    const long long share = (s1 - s0 + KNN_SELECT_WAVES - 1) / KNN_SELECT_WAVES;
    const long long i0 = min(s1, s0 + wave * share);
    const long long i1 = min(s1, i0 + share);
    const float *__restrict__ r = R + (size_t)i0 * k;
    const float *__restrict__ qp = Q + (size_t)qa * k;
    for (long long i = i0; i < i1; ++i, r += k) {
        const float acc = lane_row_dist2<KC>(qv, qp, r, k);
        if (live && acc < INFINITY && acc <= max_dist2) {   // (NaN fails both compares)
            const u64 key = pack_key(acc, gids ? gids[i] : (unsigned)(base + i));
            if (knn_radix_match(key, pre, pass))
                atomicAdd(&hist[knn_radix_digit(key, pass) * KNN_WAVE + lane], 1u);
        }
    }
    __syncthreads();
    unsigned *__restrict__ mine = ghist + (size_t)blockIdx.y * KNN_WAVE;
    for (unsigned w = threadIdx.x; w < KNN_SELECT_HIST_WORDS; w += KNN_SELECT_BLOCK) {
        const unsigned c = hist[w];
        if (c != 0u)
            atomicAdd(&mine[(size_t)(w / KNN_WAVE) * mcp + (w % KNN_WAVE)], c);
    }
}

// The pick of one pass: one thread per query walks its bins (knn_radix_pick), fixes the digit, lowers need, clears the histogram
// for the next pass, and — when the query stays open — raises the next pass's gate word.  Pass 0 starts every query at
// (prefix 0, need K); the state words are zero on entry.
__global__ __launch_bounds__(KNN_BLOCK) void knn_select_pick_kernel(unsigned *__restrict__ ghist, long long mcp, int m, int pass, int K,
                                                                   u64 *__restrict__ prefix, unsigned *__restrict__ need,
                                                                   unsigned *__restrict__ gates)
{
    if (pass != 0 && gates[pass] == 0u)
        return;
    const int q = blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (q >= m)
        return;
    unsigned nd = pass == 0 ? (unsigned)K : need[q];
    if (nd == 0u)   // resolved: it added nothing to its histogram
        return;
    u64 pre = pass == 0 ? 0ull : prefix[q];
    const bool open = knn_radix_pick(ghist + q, (u64)mcp, pass, pre, nd);
    for (unsigned b = 0; b < KNN_RADIX_BINS; ++b)
        ghist[(size_t)b * mcp + q] = 0u;
    prefix[q] = pre;
    need[q] = nd;
    if (open)   // (pass < 7: the last pass resolves)
        gates[pass + 1] = 1u;
}

// The fill: knn_exact_list_kernel's skeleton (one wave per block, the count scan's slices).  A candidate with key <= T[q]
// reserves p = cursor[q]++ and stores at list[q * K + p] when p < K.  The select leaves at most K such rows; the guard stays:
// nothing is ever stored outside a query's K places.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_select_fill_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k, int m,
                                                                  long long n, long long rows_per_slice, float max_dist2, long long base,
                                                                  const unsigned *__restrict__ gids, const u64 *__restrict__ T,
                                                                  unsigned *__restrict__ cursor, int K, u64 *__restrict__ list)
{
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    const u64 t = T[qa];
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const float *__restrict__ r = R + (size_t)i0 * k;
    const float *__restrict__ qp = Q + (size_t)qa * k;
    for (long long i = i0; i < i1; ++i, r += k) {
        const float acc = lane_row_dist2<KC>(qv, qp, r, k);
        if (q < m && acc < INFINITY && acc <= max_dist2) {   // (NaN fails both compares)
            const u64 key = pack_key(acc, gids ? gids[i] : (unsigned)(base + i));
            if (key <= t) {
                const unsigned p = atomicAdd(&cursor[q], 1u);
                if (p < (unsigned)K)
                    list[(size_t)q * K + p] = key;
            }
        }
    }
}

// One block per query: the first min(cursor[q], K) keys of its list ascending (sort_network, in LDS), the rest KNN_KEY_INIT.
__global__ __launch_bounds__(KNN_BLOCK) void knn_topk_large_sort_kernel(const unsigned *__restrict__ cursor, int K, u64 *list)
{
    __shared__ u64 lds[KNN_TOPK_LARGE_MAX];
    const unsigned q = blockIdx.x;
    const unsigned cnt = min(cursor[q], (unsigned)K);   // block-uniform
    u64 *a = list + (size_t)q * K;
    for (unsigned i = cnt + threadIdx.x; i < (unsigned)K; i += KNN_BLOCK)
        a[i] = kKeyInit;
    if (cnt < 2u)
        return;
    for (unsigned i = threadIdx.x; i < cnt; i += KNN_BLOCK)
        lds[i] = a[i];
    __syncthreads();
    sort_network(lds, cnt);
    for (unsigned i = threadIdx.x; i < cnt; i += KNN_BLOCK)
        a[i] = lds[i];
}

// One block per query: b <- the K smallest of the sorted lists a and b, sorted.  Both lists are read into LDS before any store,
// which makes the merge safe in place.  A key's place in the merged order is its own index plus its rank in the other list —
// the keys of b below it for a key of a (lower bound), the keys of a not above it for a key of b (upper bound): equal keys
// (padding) get distinct places, a's first.  Keys with place < K are stored; every place below K has exactly one writer.
__device__ __forceinline__ unsigned merge_rank(const u64 *__restrict__ s, unsigned K, u64 key, bool upper)
{
    unsigned lo = 0u, hi = K;   // first place whose key is >= key (lower) / > key (upper)
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        const u64 v = s[mid];
        if (upper ? v <= key : v < key)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(KNN_BLOCK) void knn_topk_merge_large_kernel(int K, const u64 *a, u64 *b)
{
    __shared__ u64 la[KNN_TOPK_LARGE_MAX], lb[KNN_TOPK_LARGE_MAX];
    const size_t off = (size_t)blockIdx.x * K;
    for (unsigned i = threadIdx.x; i < (unsigned)K; i += KNN_BLOCK) {
        la[i] = a[off + i];
        lb[i] = b[off + i];
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < (unsigned)K; i += KNN_BLOCK) {
        const u64 ka = la[i], kb = lb[i];
        const unsigned pa = i + merge_rank(lb, (unsigned)K, ka, false);
        const unsigned pb = i + merge_rank(la, (unsigned)K, kb, true);
        if (pa < (unsigned)K)
            b[off + pa] = ka;
        if (pb < (unsigned)K)
            b[off + pb] = kb;
    }
}

// Slices of one select pass over a chunk of mc queries: two 64 KiB blocks are resident per CU, twice that many are launched
// (the tail of a pass is then a quarter of a block's work), a slice holds at least 128 rows per wave.
long long knn_select_slices(int mc, long long n, int num_cu)
{
    const long long qg = knn_divup(mc, KNN_WAVE);
    long long slices = (long long)num_cu * 4 / qg;
    const long long by_rows = (n + 128 * KNN_SELECT_WAVES - 1) / (128 * KNN_SELECT_WAVES);
    if (slices > by_rows)
        slices = by_rows;
    if (slices > 65535)
        slices = 65535;
    if (slices < 1)
        slices = 1;
    const long long per = (n + slices - 1) / slices;
    return (n + per - 1) / per;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

TopkLargePlan knn_topk_large_plan(int k, int m, int K, long long n, int num_cu, bool init)
{
    TopkLargePlan p;
    const SlicePlan sp = knn_slice_plan(m, n, num_cu, KnnSelectSlices{});
    p.chunks = sp.chunks;
    p.chunk_m = sp.chunk_m;
    p.mcp = sp.groups * KNN_WAVE;
    p.slices = sp.slices;
    p.dist_passes = KNN_RADIX_DIST_PASSES;
    p.index_passes = KNN_RADIX_PASSES - KNN_RADIX_DIST_PASSES;
    p.lds_bytes = sp.lds_bytes;
    const size_t mcp = (size_t)p.mcp;
    p.hist_off = 0;
    p.prefix_off = align256(p.hist_off + (size_t)KNN_RADIX_BINS * mcp * sizeof(unsigned));
    p.need_off = align256(p.prefix_off + mcp * sizeof(u64));
    p.cursor_off = align256(p.need_off + mcp * sizeof(unsigned));
    p.gate_off = align256(p.cursor_off + mcp * sizeof(unsigned));
    p.state_bytes = align256(p.gate_off + (KNN_RADIX_PASSES + 1) * sizeof(unsigned));
    p.list_off = p.state_bytes;
    p.scratch_bytes = p.state_bytes + (init ? 0 : (size_t)p.chunk_m * (size_t)K * sizeof(u64));
    // per chunk: the state's memset, a scan and a pick per pass, the fill, the sort and — a folding call — the merge
    const long long fixed = 1 + 1 + 1 + (init ? 0 : 1);
    p.launches_clean = (long long)p.chunks * (fixed + 2 * p.dist_passes);
    p.launches_ties = (long long)p.chunks * (fixed + 2 * (p.dist_passes + p.index_passes));
    (void)k;
    return p;
}

hipError_t knn_topk_large_launch(const TopkCall &c, const TopkLargePlan &p, const unsigned **tie_word)
{
    if (c.m <= 0 || c.n <= 0 || c.K < 1 || c.K > KNN_TOPK_LARGE_MAX || !c.part || c.part_bytes < p.scratch_bytes)
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    unsigned char *st = (unsigned char *)c.part;
    return knn_select_round(
        c, p, tie_word,
        [&](const SliceChunk &ch, const float *qc, int pass, const unsigned *pass_gate) {
            const int mc = ch.mc;
            const long long mcp = (long long)ch.grid.y * KNN_WAVE;
#define KNN_SELECT_HIST(KCV)                                                                                                       \
    hipLaunchKernelGGL(knn_select_hist_kernel<KCV>, ch.grid, dim3(KNN_SELECT_BLOCK), 0, s, qc, c.r, c.k, mc, c.n, ch.per,         \
                       c.max_dist2, c.base, c.gids, pass, (const u64 *)(st + p.prefix_off), (const unsigned *)(st + p.need_off), \
                       (unsigned *)(st + p.hist_off), mcp, pass_gate)
            KNN_KC_SWITCH(c.k, KNN_SELECT_HIST)
#undef KNN_SELECT_HIST
        },
        [&](const SliceChunk &ch, const float *qc, u64 *list) {
            const int mc = ch.mc;
#define KNN_SELECT_FILL(KCV)                                                                                                 \
    hipLaunchKernelGGL(knn_select_fill_kernel<KCV>, ch.grid, dim3(KNN_WAVE), 0, s, qc, c.r, c.k, mc, c.n, ch.per, c.max_dist2, \
                       c.base, c.gids, (const u64 *)(st + p.prefix_off), (unsigned *)(st + p.cursor_off), c.K, list)
            KNN_KC_SWITCH(c.k, KNN_SELECT_FILL)
#undef KNN_SELECT_FILL
        });
}

// The select's pieces that do not look at rows, for the select over a subset of the rows (knn_masked_lists.hip).
hipError_t knn_select_pick_launch(const TopkLargePlan &p, u64 *scratch, int mc, int pass, int K, hipStream_t s)
{
    if (!scratch || mc <= 0 || mc > p.mcp || pass < 0 || pass >= KNN_RADIX_PASSES || K < 1 || K > KNN_TOPK_LARGE_MAX)
        return hipErrorInvalidValue;
    unsigned char *st = (unsigned char *)scratch;
    hipLaunchKernelGGL(knn_select_pick_kernel, dim3((unsigned)knn_divup(mc, KNN_BLOCK)), dim3(KNN_BLOCK), 0, s,
                       (unsigned *)(st + p.hist_off), (long long)knn_divup(mc, KNN_WAVE) * KNN_WAVE, mc, pass, K,
                       (u64 *)(st + p.prefix_off), (unsigned *)(st + p.need_off), (unsigned *)(st + p.gate_off));
    return hipGetLastError();
}

hipError_t knn_topk_large_sort_launch(const TopkLargePlan &p, const u64 *scratch, int mc, int K, u64 *list, hipStream_t s)
{
    if (!scratch || !list || mc <= 0 || mc > p.mcp || K < 1 || K > KNN_TOPK_LARGE_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_topk_large_sort_kernel, dim3((unsigned)mc), dim3(KNN_BLOCK), 0, s,
                       (const unsigned *)((const unsigned char *)scratch + p.cursor_off), K, list);
    return hipGetLastError();
}

hipError_t knn_topk_merge_large_launch(int m, int K, const u64 *a, u64 *b, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    if (K < 1 || K > KNN_TOPK_LARGE_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_topk_merge_large_kernel, dim3((unsigned)m), dim3(KNN_BLOCK), 0, s, K, a, b);
    return hipGetLastError();
}
