// knn_masked_lists.hip — lists within a radius and top-K beyond 64 over a subset of the rows (include/knn_mi355x.h 2h; DESIGN §4.6
// "Lists and large K over a subset of the rows"): knn_index_list_within_masked, knn_index_query_topk_large_masked.
//
// The subset is knn_masked.hip's bit mask over the shard's local rows, cut into slices of equal numbers of ADMITTED rows
// (knn_mask_split.h) and walked word by word (knn_masked_dev.h).  The three scans here are the skeletons of the unmasked calls'
// scans with that walk in place of the row loop:
//   knn_masked_list_kernel<KC>   knn_exact_list_kernel<KC> (knn_exact.hip): the second pass of masked count -> offsets -> list;
//   knn_masked_hist_kernel<KC>   knn_select_hist_kernel<KC> (knn_select.hip): one pass of the radix select;
//   knn_masked_fill_kernel<KC>   knn_select_fill_kernel<KC>: the rows with key <= T into the query's K places.
// A masked select is a select over the admitted rows: the histograms count admitted candidates only, so the round — memset, pick
// (knn_select_pick_kernel), sort, fold — is the unmasked call's own (knn_select_round, knn_slice_launch.h), handed the two masked
// scans.  Chunks, slices and the KC forms: knn_slice_launch.h, as for every exact slice scan.
#include "knn_masked_dev.h"
#include "knn_radix_pick.h"
#include "knn_slice_launch.h"

// knn_masked_list_kernel<KC> — knn_exact_list_kernel<KC> over the admitted rows of the block's slice: one wave per block, lanes =
// queries, a hit reserves and stores through list_put.  The walk gives the LOCAL row i; the key carries gids[i] or base + i.
// grid = the masked count's for the same call: (knn_count_slices, query groups of 64).
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_masked_list_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                  int m, long long n, const unsigned *__restrict__ mask,
                                                                  const u64 *__restrict__ P, int G, float max_dist2, long long base,
                                                                  const unsigned *__restrict__ gids,
                                                                  const u64 *__restrict__ offsets, unsigned *__restrict__ fill,
                                                                  u64 *__restrict__ keys, const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (gate && *gate == 0u)   // (the exact answer behind a pruned way of a routed masked call, 2l; null: always)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    u64 off;
    const unsigned room = list_room(offsets, (unsigned)qa, off);
    const float *__restrict__ qp = Q + (size_t)qa * k;
    long long r0, r1;
    masked_slice(mask, n, P, G, r0, r1);
    masked_walk(mask, P, G, r0, r1, [&](long long i) {
        const float acc = lane_row_dist2<KC>(qv, qp, R + (size_t)i * k, k);
        if (q < m && acc < INFINITY && acc <= max_dist2)   // (NaN fails both compares)
            list_put(&fill[q], keys, off, room, pack_key(acc, gids ? gids[i] : (unsigned)(base + i)));
    });
}

// knn_masked_hist_kernel<KC> — one pass of the select (knn_select_hist_kernel's histogram, gate and flush) over the admitted rows.
// The block's KNN_SELECT_WAVES waves hold the SAME 64 queries; each walks its OWN slice by admitted rows — wave w of block b takes
// slice b * W + w of gridDim.x * W — so a mask that admits one contiguous range loads every wave alike, where a share of the
// block's rows by position would leave most waves of most blocks idle.
template <int KC>
__global__ __launch_bounds__(KNN_SELECT_BLOCK) void knn_masked_hist_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k,
                                                                          int m, long long n, const unsigned *__restrict__ mask,
                                                                          const u64 *__restrict__ P, int G, float max_dist2,
                                                                          long long base, const unsigned *__restrict__ gids, int pass,
                                                                          const u64 *__restrict__ prefix, const unsigned *__restrict__ need,
                                                                          unsigned *__restrict__ ghist, long long mcp,
                                                                          const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    __shared__ unsigned hist[KNN_SELECT_HIST_WORDS];
    if (gate && *gate == 0u)
        return;
    for (unsigned w = threadIdx.x; w < KNN_SELECT_HIST_WORDS; w += KNN_SELECT_BLOCK)
        hist[w] = 0u;
    __syncthreads();
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x & (KNN_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / KNN_WAVE));   // (uniform: the walk stays scalar)
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    const bool live = q < m && (pass == 0 || need[qa] != 0u);
    const u64 pre = pass == 0 ? 0ull : prefix[qa];
    const float *__restrict__ qp = Q + (size_t)qa * k;
    long long r0, r1;
    masked_wave_slice(mask, n, P, G, KNN_SELECT_WAVES, wave, r0, r1);
    masked_walk(mask, P, G, r0, r1, [&](long long i) {
        const float acc = lane_row_dist2<KC>(qv, qp, R + (size_t)i * k, k);
        if (live && acc < INFINITY && acc <= max_dist2) {   // (NaN fails both compares)
            const u64 key = pack_key(acc, gids ? gids[i] : (unsigned)(base + i));
            if (knn_radix_match(key, pre, pass))
                atomicAdd(&hist[knn_radix_digit(key, pass) * KNN_WAVE + lane], 1u);
        }
    });
    __syncthreads();
    unsigned *__restrict__ mine = ghist + (size_t)blockIdx.y * KNN_WAVE;
    for (unsigned w = threadIdx.x; w < KNN_SELECT_HIST_WORDS; w += KNN_SELECT_BLOCK) {
        const unsigned c = hist[w];
        if (c != 0u)
            atomicAdd(&mine[(size_t)(w / KNN_WAVE) * mcp + (w % KNN_WAVE)], c);
    }
}

// knn_masked_fill_kernel<KC> — knn_select_fill_kernel<KC> over the admitted rows of the block's slice (one wave per block, the
// masked count's slices): an admitted candidate with key <= T[q] reserves p = cursor[q]++ and stores at list[q * K + p] when p < K.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_masked_fill_kernel(const float *__restrict__ Q, const float *__restrict__ R, int k, int m,
                                                                  long long n, const unsigned *__restrict__ mask,
                                                                  const u64 *__restrict__ P, int G, float max_dist2, long long base,
                                                                  const unsigned *__restrict__ gids, const u64 *__restrict__ T,
                                                                  unsigned *__restrict__ cursor, int K, u64 *__restrict__ list)
{
#pragma clang fp contract(off)
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? Q[(size_t)qa * k + d] : 0.0f;
    const u64 t = T[qa];
    const float *__restrict__ qp = Q + (size_t)qa * k;
    long long r0, r1;
    masked_slice(mask, n, P, G, r0, r1);
    masked_walk(mask, P, G, r0, r1, [&](long long i) {
        const float acc = lane_row_dist2<KC>(qv, qp, R + (size_t)i * k, k);
        if (q < m && acc < INFINITY && acc <= max_dist2) {   // (NaN fails both compares)
            const u64 key = pack_key(acc, gids ? gids[i] : (unsigned)(base + i));
            if (key <= t) {
                const unsigned p = atomicAdd(&cursor[q], 1u);
                if (p < (unsigned)K)
                    list[(size_t)q * K + p] = key;
            }
        }
    });
}

MaskedListsPlan knn_masked_lists_plan(int k, int m, int K, long long n, int num_cu, bool init)
{
    MaskedListsPlan p;
    p.cut = knn_masked_plan(k, m, 0, n, num_cu, init);   // granules, chunks, the mask scratch; a list call's slices
    if (m <= 0)
        return p;
    if (n <= 0) {   // an empty shard: an init large call fills the keys, everything else launches nothing
        p.launches = K > 0 && init ? 1 : 0;
        return p;
    }
    if (K > 0) {
        p.sel = knn_topk_large_plan(k, m, K, n, num_cu, init);
        p.slices = p.sel.slices;
        p.slice_waves = KNN_SELECT_WAVES;
        p.lds_bytes = p.sel.lds_bytes;
        p.select_bytes = p.sel.scratch_bytes;
        p.launches = 2 + p.sel.launches_clean;
    } else {
        p.slices = p.cut.slices;
        p.slice_waves = 1;
        p.launches = 2 + (long long)p.cut.chunks;
    }
    return p;
}

hipError_t knn_masked_list_launch(const ListCall &c, const MaskedListsPlan &p, const unsigned *mask, u64 *scratch, const unsigned *gate)
{
    hipStream_t s = c.stream;
    if (c.m <= 0 || c.n <= 0 || !mask || !scratch || !c.offsets || !c.fill || !c.keys || c.radii || c.self_first >= 0)
        return hipErrorInvalidValue;
    hipError_t e = knn_masked_prefix_launch(p.cut, c.n, mask, scratch, s, gate);
    if (e != hipSuccess)
        return e;
    if (!gate && c.ev0 && (e = hipEventRecord(c.ev0, s)) != hipSuccess)
        return e;
    e = knn_slice_chunks(c.m, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0;
        const dim3 grid = ch.grid, block(KNN_WAVE);
        const float *qc = c.q + (size_t)c0 * c.k;
#define KNN_MASKED_LIST(KCV)                                                                                                   \
    hipLaunchKernelGGL(knn_masked_list_kernel<KCV>, grid, block, 0, s, qc, c.r, c.k, mc, c.n, mask, (const u64 *)scratch,     \
                       (int)p.cut.granules, c.max_dist2, c.base, c.gids, c.offsets + c0, c.fill + c0, c.keys, gate)
        KNN_KC_SWITCH(c.k, KNN_MASKED_LIST)
#undef KNN_MASKED_LIST
        return hipGetLastError();
    });
    if (e != hipSuccess)
        return e;
    if (!gate && c.ev1 && (e = hipEventRecord(c.ev1, s)) != hipSuccess)
        return e;
    return hipSuccess;
}

hipError_t knn_masked_large_launch(const TopkCall &c, const MaskedListsPlan &p, const unsigned *mask, u64 *scratch,
                                   const unsigned **tie_word)
{
    if (c.m <= 0 || c.n <= 0 || c.K < 1 || c.K > KNN_TOPK_LARGE_MAX || !mask || !scratch || !c.part || c.part_bytes < p.select_bytes ||
        p.select_bytes < p.sel.state_bytes || p.sel.state_bytes == 0)
        return hipErrorInvalidValue;
    hipStream_t s = c.stream;
    const TopkLargePlan &sp = p.sel;
    unsigned char *st = (unsigned char *)c.part;
    const u64 *P = (const u64 *)scratch;
    const int G = (int)p.cut.granules;
    hipError_t e = knn_masked_prefix_launch(p.cut, c.n, mask, scratch, s);
    if (e != hipSuccess)
        return e;
    return knn_select_round(
        c, sp, tie_word,
        [&](const SliceChunk &ch, const float *qc, int pass, const unsigned *pass_gate) {
            const int mc = ch.mc;
            const long long mcp = (long long)ch.grid.y * KNN_WAVE;
#define KNN_MASKED_HIST(KCV)                                                                                                        \
    hipLaunchKernelGGL(knn_masked_hist_kernel<KCV>, ch.grid, dim3(KNN_SELECT_BLOCK), 0, s, qc, c.r, c.k, mc, c.n, mask, P, G,      \
                       c.max_dist2, c.base, c.gids, pass, (const u64 *)(st + sp.prefix_off), (const unsigned *)(st + sp.need_off), \
                       (unsigned *)(st + sp.hist_off), mcp, pass_gate)
            KNN_KC_SWITCH(c.k, KNN_MASKED_HIST)
#undef KNN_MASKED_HIST
        },
        [&](const SliceChunk &ch, const float *qc, u64 *list) {
            const int mc = ch.mc;
#define KNN_MASKED_FILL(KCV)                                                                                                \
    hipLaunchKernelGGL(knn_masked_fill_kernel<KCV>, ch.grid, dim3(KNN_WAVE), 0, s, qc, c.r, c.k, mc, c.n, mask, P, G,      \
                       c.max_dist2, c.base, c.gids, (const u64 *)(st + sp.prefix_off), (unsigned *)(st + sp.cursor_off), c.K, list)
            KNN_KC_SWITCH(c.k, KNN_MASKED_FILL)
#undef KNN_MASKED_FILL
        });
}
