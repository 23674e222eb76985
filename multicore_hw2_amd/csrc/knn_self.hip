// knn_self.hip — queries about the shard's own rows (include/knn_mi355x.h 2i; DESIGN §4.6 "About the shard's own rows"):
// knn_index_self_topk, knn_index_self_count_within, knn_index_self_list_within.
//
// Query j of a call is LOCAL row first + j of the shard, and that row is no candidate for it: the K nearest OTHER rows, the other
// rows within a radius.  The three scans are the skeletons of knn_exact_topk_kernel<KC, LIM>, knn_exact_count_kernel<KC> and
// knn_exact_list_kernel<KC> (knn_exact.hip) — one wave per block, lanes = queries, rows as wave-uniform scalar loads, v0's
// arithmetic (lane_row_dist2, knn_exact_dev.h) — with two changes.  A lane's coordinates come straight from the resident rows,
// R + (first + q) * k: no queries pointer, nothing uploaded or gathered.  And the block cuts its slice around the only rows that can
// be some lane's own — the window [w0, w0 + 64), w0 = first + 64 * blockIdx.y (knn_self_window.h) — into the rows before it, inside
// it and after it, and runs one row-loop body over the three: only the window's form compares the (wave-uniform) row with the
// lane's own 32-bit local row, everywhere else a row costs what it costs the exact scan.  An excluded row never enters the column,
// the counter or the list; everything behind that — the sorted LDS column and the min(column[K - 1], lim) rule, part[slice][query][K]
// with global numbers, knn_topk_select_launch, list_room / list_put, one atomicAdd per lane — is the plain kernels' own.
//
// knn_self_drop_kernel finishes the top-K's through way (knn_api.cpp): the plain call's K + 1 nearest, self among the candidates,
// become the K nearest others.
//
// knn_self_count_gated_kernel and knn_self_list_gated_kernel are the count and list scans behind a device gate: the exact answer of
// the routed self calls (include/knn_mi355x.h 2k) when the grid gave up or a cell-pruned pass fell back.
#include "knn_self_scan.h"   // self_rows, self_scan, self_scan_one: the row loops (shared with knn_cluster.hip)
#include "knn_slice_launch.h"

// knn_self_topk_kernel<KC, LIM> — knn_exact_topk_kernel<KC, LIM> for the m queries that are the rows first .. first + m - 1.  LIM as
// there: the call has a radius, the K-th key a row is compared with is min(column[K - 1], lim); the plain form never reads `lim`
// (its launcher picks it when the limit key is KNN_KEY_INIT, as knn_exact_topk_launch does).  grid = (slices, query groups of 64).
template <int KC, bool LIM>
__device__ __forceinline__ void self_topk_body(const float *__restrict__ R, int k, long long first, int m, long long n, int K,
                                               long long rows_per_slice, long long base, const unsigned *__restrict__ gids,
                                               u64 *__restrict__ part, u64 lim)
{
#pragma clang fp contract(off)
    extern __shared__ u64 self_lst[];   // [K][KNN_WAVE]
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    const float *__restrict__ qp = R + (size_t)(first + qa) * k;
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? qp[d] : 0.0f;
    for (int t = 0; t < K; ++t)
        self_lst[t * KNN_WAVE + lane] = kKeyInit;
    u64 kth = LIM && lim < kKeyInit ? lim : kKeyInit;
    const unsigned own = (unsigned)(first + q);   // the lane's own local row (lanes beyond m write nothing)
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned row) {
        const u64 key = pack_key(acc, row);
        if (key < kth) {
            int p = K - 1;
            while (p > 0) {
                const u64 prev = self_lst[(p - 1) * KNN_WAVE + lane];
                if (prev < key)
                    break;
                self_lst[p * KNN_WAVE + lane] = prev;
                --p;
            }
            self_lst[p * KNN_WAVE + lane] = key;
            kth = self_lst[(K - 1) * KNN_WAVE + lane];
            if (LIM)
                kth = kth < lim ? kth : lim;
        }
    });
    if (q >= m)
        return;
    u64 *__restrict__ out = part + ((size_t)blockIdx.x * m + q) * K;
    for (int t = 0; t < K; ++t) {
        const u64 key = self_lst[t * KNN_WAVE + lane];
        const unsigned row = (unsigned)key;
        const bool real = (key >> 32) < 0x7F800000ull;
        const unsigned g = gids ? (real ? gids[row] : 0u) : (unsigned)(base + (long long)row);
        out[t] = real ? ((key & 0xFFFFFFFF00000000ull) | (u64)g) : kKeyInit;
    }
}

template <int KC, bool LIM>
__global__ __launch_bounds__(KNN_WAVE) void knn_self_topk_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                long long n, int K, long long rows_per_slice, long long base,
                                                                const unsigned *__restrict__ gids, u64 *__restrict__ part, u64 lim)
{
    self_topk_body<KC, LIM>(R, k, first, m, n, K, rows_per_slice, base, gids, part, lim);
}

// KC = 1 (k <= 16) within 80 scalar registers.  Left alone the compiler takes 84-86 where the exact sibling takes 76; the device
// allocates that as 96 against 80, and a SIMD then holds fewer waves: at k 16, n 2^20, 1024 rows, K 8 — a grid of exactly 8 blocks
// per SIMD — the uncapped call is 0.3-0.4 ms slower than the capped one and than the caller's workaround
// (profiles/self_join_timing.txt holds both builds, taken in one session).  Only KC 1 is capped: from KC 2 on the self kernels and
// their exact siblings both take the compiler's 106, so there a self kernel is in its sibling's position already.
// -DKNN_SELF_KC1_SGPRS=0 builds the uncapped form for that comparison.
#ifndef KNN_SELF_KC1_SGPRS
#define KNN_SELF_KC1_SGPRS 72
#endif
#define KNN_SELF_TOPK_KC1(LIMV)                                                                                                   \
    template <>                                                                                                                   \
    __global__ __launch_bounds__(KNN_WAVE) __attribute__((amdgpu_num_sgpr(KNN_SELF_KC1_SGPRS))) void knn_self_topk_kernel<1, LIMV>(               \
        const float *__restrict__ R, int k, long long first, int m, long long n, int K, long long rows_per_slice, long long base, \
        const unsigned *__restrict__ gids, u64 *__restrict__ part, u64 lim)                                                       \
    {                                                                                                                             \
        self_topk_body<1, LIMV>(R, k, first, m, n, K, rows_per_slice, base, gids, part, lim);                                     \
    }
KNN_SELF_TOPK_KC1(true)
KNN_SELF_TOPK_KC1(false)
#undef KNN_SELF_TOPK_KC1

// knn_self_count_kernel<KC> — knn_exact_count_kernel<KC> for the queries that are the rows first .. first + m - 1: one counter per
// lane, one atomicAdd at the end when it is not zero.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_self_count_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                 long long n, long long rows_per_slice, float max_dist2,
                                                                 unsigned *__restrict__ counts)
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
    unsigned cnt = 0u;
    const unsigned own = (unsigned)(first + q);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned) {
        cnt += acc < INFINITY && acc <= max_dist2 ? 1u : 0u;   // (NaN fails both compares)
    });
    if (q < m && cnt != 0u)
        atomicAdd(&counts[q], cnt);
}

// knn_self_list_kernel<KC> — knn_exact_list_kernel<KC> for the queries that are the rows first .. first + m - 1: a hit reserves and
// stores (list_put).
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_self_list_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                long long n, long long rows_per_slice, float max_dist2,
                                                                long long base, const unsigned *__restrict__ gids,
                                                                const u64 *__restrict__ offsets, unsigned *__restrict__ fill,
                                                                u64 *__restrict__ keys)
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
    u64 off;
    const unsigned room = list_room(offsets, (unsigned)qa, off);
    const unsigned own = (unsigned)(first + q);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan_one<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned row, bool other) {
        if (other && q < m && acc < INFINITY && acc <= max_dist2)   // (NaN fails both compares)
            list_put(&fill[q], keys, off, room, pack_key(acc, gids ? gids[row] : (unsigned)(base + (long long)row)));
    });
}

// A radius per query (include/knn_mi355x.h 2j; DESIGN §4.6 "A radius per query"): knn_self_count_kernel<KC> and
// knn_self_list_kernel<KC> with the lane's own radius.  radii is the CALL's array — radii[j] belongs to query j, local row
// first + j —, so the lane reads radii[q], never radii[its row number]; the launchers advance it with the chunks.  A hit:
// E finite, E <= radii[q] and E <= cap, two fp32 compares (a NaN or negative radius fails the first for every row).
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_self_count_each_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                      long long n, long long rows_per_slice,
                                                                      const float *__restrict__ radii, float cap,
                                                                      unsigned *__restrict__ counts)
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
    const float rad = radii[qa];
    unsigned cnt = 0u;
    const unsigned own = (unsigned)(first + q);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned) {
        cnt += acc < INFINITY && acc <= rad && acc <= cap ? 1u : 0u;   // (NaN — the distance or the radius — fails)
    });
    if (q < m && cnt != 0u)
        atomicAdd(&counts[q], cnt);
}

template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_self_list_each_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                     long long n, long long rows_per_slice,
                                                                     const float *__restrict__ radii, float cap, long long base,
                                                                     const unsigned *__restrict__ gids,
                                                                     const u64 *__restrict__ offsets, unsigned *__restrict__ fill,
                                                                     u64 *__restrict__ keys)
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
    const float rad = radii[qa];
    u64 off;
    const unsigned room = list_room(offsets, (unsigned)qa, off);
    const unsigned own = (unsigned)(first + q);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan_one<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned row, bool other) {
        if (other && q < m && acc < INFINITY && acc <= rad && acc <= cap)   // (NaN — the distance or the radius — fails)
            list_put(&fill[q], keys, off, room, pack_key(acc, gids ? gids[row] : (unsigned)(base + (long long)row)));
    });
}

// The gated twins (include/knn_mi355x.h 2k; DESIGN §4.6 "The radius graph on the pruned ways"): the exact answer behind the grid
// way and behind a cell-pruned pass of a routed self call.  They do nothing unless *gate != 0 — the grid's give-up word, a pass's
// FALLBACK word —, as the gated exact count and list do behind the plain calls.  The bodies are knn_self_count_each_kernel's and
// knn_self_list_each_kernel's, copied: a body shared with those two changed the code the compiler makes of them (tools/isa_same.py),
// and they are to stay as measured.  One difference: radii may be null — the scalar form, every lane's radius the cap.
template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_self_count_gated_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                       long long n, long long rows_per_slice,
                                                                       const float *__restrict__ radii, float cap,
                                                                       unsigned *__restrict__ counts,
                                                                       const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (*gate == 0u)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    const float *__restrict__ qp = R + (size_t)(first + qa) * k;
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? qp[d] : 0.0f;
    const float rad = radii ? radii[qa] : cap;
    unsigned cnt = 0u;
    const unsigned own = (unsigned)(first + q);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned) {
        cnt += acc < INFINITY && acc <= rad && acc <= cap ? 1u : 0u;   // (NaN — the distance or the radius — fails)
    });
    if (q < m && cnt != 0u)
        atomicAdd(&counts[q], cnt);
}

template <int KC>
__global__ __launch_bounds__(KNN_WAVE) void knn_self_list_gated_kernel(const float *__restrict__ R, int k, long long first, int m,
                                                                      long long n, long long rows_per_slice,
                                                                      const float *__restrict__ radii, float cap, long long base,
                                                                      const unsigned *__restrict__ gids,
                                                                      const u64 *__restrict__ offsets, unsigned *__restrict__ fill,
                                                                      u64 *__restrict__ keys, const unsigned *__restrict__ gate)
{
#pragma clang fp contract(off)
    if (*gate == 0u)
        return;
    constexpr int KM = KC > 0 ? 16 * KC : 1;
    const int lane = threadIdx.x;
    const int q = blockIdx.y * KNN_WAVE + lane;
    const int qa = min(q, m - 1);
    const float *__restrict__ qp = R + (size_t)(first + qa) * k;
    float qv[KM];
#pragma unroll
    for (int d = 0; d < KM; ++d)
        qv[d] = KC > 0 && d < k ? qp[d] : 0.0f;
    const float rad = radii ? radii[qa] : cap;
    u64 off;
    const unsigned room = list_room(offsets, (unsigned)qa, off);
    const unsigned own = (unsigned)(first + q);
    const long long i0 = (long long)blockIdx.x * rows_per_slice;
    const long long i1 = min(n, i0 + rows_per_slice);
    const long long w0 = first + (long long)blockIdx.y * KNN_WAVE;
    const long long w1 = min(w0 + KNN_WAVE, first + m);
    self_scan_one<KC>(qv, qp, R, k, i0, i1, w0, w1, own, [&](float acc, unsigned row, bool other) {
        if (other && q < m && acc < INFINITY && acc <= rad && acc <= cap)   // (NaN — the distance or the radius — fails)
            list_put(&fill[q], keys, off, room, pack_key(acc, gids ? gids[row] : (unsigned)(base + (long long)row)));
    });
}

// knn_self_drop_kernel — one wave (block) per query: lists[q][0 .. K] is the plain call's sorted top-(K + 1) for the query that is
// local row first + q, self among the candidates.  The entry that is a real key (high word below +INF's bits) and carries the
// query's own global number goes; when there is none — more than K other rows at or before self's place, or a self-distance that is
// not finite — the last entry goes.  out[q][0 .. K) <- the K that stay, still sorted.
__global__ __launch_bounds__(KNN_WAVE) void knn_self_drop_kernel(const u64 *__restrict__ lists, int K, long long first, long long base,
                                                                const unsigned *__restrict__ gids, u64 *__restrict__ out)
{
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    const long long row = first + q;
    const unsigned self = gids ? gids[row] : (unsigned)(base + row);
    const u64 *__restrict__ in = lists + (size_t)q * (size_t)(K + 1);
    const u64 key = lane <= K ? in[lane] : ~0ull;
    const u64 hit = __ballot(lane <= K && (key >> 32) < 0x7F800000ull && (unsigned)key == self);
    const int pos = hit ? (int)__builtin_ctzll(hit) : K;   // wave-uniform
    if (lane < K)
        out[(size_t)q * K + lane] = lane < pos ? key : in[lane + 1];
}

SelfPlan knn_self_plan(int /*k*/, int m, int K, long long n, int num_cu, bool init)
{
    SelfPlan p;
    if (m <= 0 || n <= 0)
        return p;
    const SlicePlan sp = knn_slice_plan(m, K, n, num_cu);   // (the plain exact scan's chunks, slices, LDS and per-slice lists)
    p.chunk_m = sp.chunk_m;
    p.chunks = sp.chunks;
    p.slices = sp.slices;
    p.groups = sp.groups;
    p.lds_bytes = sp.lds_bytes;
    p.part_bytes = sp.part_bytes;
    // the through way: the plain call's lists [m][K + 1], and behind them — a folding call — the K that stay [m][K]
    if (K > 0 && K + 1 <= KNN_TOPK_MAX)
        p.through_bytes = (size_t)m * (size_t)(K + 1) * sizeof(u64) + (init ? 0 : (size_t)m * (size_t)K * sizeof(u64));
    p.launches = (long long)p.chunks * (K > 0 ? 2 : 1);
    return p;
}

hipError_t knn_self_topk_launch(const TopkCall &c, long long row_first)
{
    const int K = c.K;
    hipStream_t s = c.stream;
    if (c.m <= 0 || K < 1 || K > KNN_TOPK_MAX || row_first < 0 || row_first + c.m > c.n)
        return hipErrorInvalidValue;
    hipError_t e;
    if (c.ev0 && (e = hipEventRecord(c.ev0, s)) != hipSuccess)
        return e;
    const u64 lim = c.limit_key();
    const bool within = lim < kKeyInit;
    e = knn_slice_chunks(c.m, c.n, c.num_cu, KnnTopkSlices{K}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0, per = ch.per;
        if (KnnTopkSlices{K}.part_bytes(ch.slices, mc) > c.part_bytes)
            return hipErrorInvalidValue;
        if (per > 0xFFFFFFFFll)   // (the kernels count a slice's rows in 32 bits)
            return hipErrorInvalidValue;
        const dim3 grid = ch.grid, block(KNN_WAVE);
        const size_t lds = KnnTopkSlices{K}.lds_bytes();
#define KNN_SELF_TOPK(KCV)                                                                                                          \
    if (within)                                                                                                                     \
        hipLaunchKernelGGL((knn_self_topk_kernel<KCV, true>), grid, block, lds, s, c.r, c.k, row_first + c0, mc, c.n, K, per, c.base, \
                           c.gids, c.part, lim);                                                                                    \
    else                                                                                                                            \
        hipLaunchKernelGGL((knn_self_topk_kernel<KCV, false>), grid, block, lds, s, c.r, c.k, row_first + c0, mc, c.n, K, per, c.base, \
                           c.gids, c.part, lim)
        KNN_KC_SWITCH(c.k, KNN_SELF_TOPK)
#undef KNN_SELF_TOPK
        const hipError_t el = hipGetLastError();
        if (el != hipSuccess)
            return el;
        return knn_topk_select_launch(c.part, (int)ch.slices, mc, K, c.keys + (size_t)c0 * K, c.init, s);
    });
    if (e != hipSuccess)
        return e;
    if (c.ev1 && (e = hipEventRecord(c.ev1, s)) != hipSuccess)
        return e;
    return hipSuccess;
}

hipError_t knn_self_count_launch(const CountCall &c, long long row_first, const unsigned *gate)
{
    hipStream_t s = c.stream;
    if (c.m <= 0 || row_first < 0 || row_first + c.m > c.n)
        return hipErrorInvalidValue;
    hipError_t e;
    if (!gate && c.ev0 && (e = hipEventRecord(c.ev0, s)) != hipSuccess)   // (a gated scan is not its way's dominant kernel)
        return e;
    e = knn_slice_chunks(c.m, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0, per = ch.per;
        if (per > 0xFFFFFFFFll)   // (the kernels count a slice's rows in 32 bits)
            return hipErrorInvalidValue;
        const dim3 grid = ch.grid, block(KNN_WAVE);
#define KNN_SELF_COUNT(KCV)                                                                                                          \
    if (gate)      /* the gated twin: scalar form and radii alike */                                                                 \
        hipLaunchKernelGGL(knn_self_count_gated_kernel<KCV>, grid, block, 0, s, c.r, c.k, row_first + c0, mc, c.n, per,               \
                           c.radii ? c.radii + c0 : nullptr, c.max_dist2, c.counts + c0, gate);                                      \
    else if (c.radii)   /* a radius per query: the radii advance with the chunk */                                                   \
        hipLaunchKernelGGL(knn_self_count_each_kernel<KCV>, grid, block, 0, s, c.r, c.k, row_first + c0, mc, c.n, per, c.radii + c0,  \
                           c.max_dist2, c.counts + c0);                                                                              \
    else                                                                                                                             \
        hipLaunchKernelGGL(knn_self_count_kernel<KCV>, grid, block, 0, s, c.r, c.k, row_first + c0, mc, c.n, per, c.max_dist2, c.counts + c0)
        KNN_KC_SWITCH(c.k, KNN_SELF_COUNT)
#undef KNN_SELF_COUNT
        return hipGetLastError();
    });
    if (e != hipSuccess)
        return e;
    if (!gate && c.ev1 && (e = hipEventRecord(c.ev1, s)) != hipSuccess)
        return e;
    return hipSuccess;
}

hipError_t knn_self_list_launch(const ListCall &c, long long row_first, const unsigned *gate)
{
    hipStream_t s = c.stream;
    if (c.m <= 0 || row_first < 0 || row_first + c.m > c.n)
        return hipErrorInvalidValue;
    hipError_t e;
    if (!gate && c.ev0 && (e = hipEventRecord(c.ev0, s)) != hipSuccess)   // (a gated scan is not its way's dominant kernel)
        return e;
    e = knn_slice_chunks(c.m, c.n, c.num_cu, KnnCountSlices{}, [&](const SliceChunk &ch) {
        const int mc = ch.mc;
        const long long c0 = ch.c0, per = ch.per;
        if (per > 0xFFFFFFFFll)   // (the kernels count a slice's rows in 32 bits)
            return hipErrorInvalidValue;
        const dim3 grid = ch.grid, block(KNN_WAVE);
#define KNN_SELF_LIST(KCV)                                                                                                              \
    if (gate)      /* the gated twin: scalar form and radii alike */                                                                    \
        hipLaunchKernelGGL(knn_self_list_gated_kernel<KCV>, grid, block, 0, s, c.r, c.k, row_first + c0, mc, c.n, per,                   \
                           c.radii ? c.radii + c0 : nullptr, c.max_dist2, c.base, c.gids, c.offsets + c0, c.fill + c0, c.keys, gate);   \
    else if (c.radii)   /* a radius per query: the radii advance with the chunk */                                                      \
        hipLaunchKernelGGL(knn_self_list_each_kernel<KCV>, grid, block, 0, s, c.r, c.k, row_first + c0, mc, c.n, per, c.radii + c0,      \
                           c.max_dist2, c.base, c.gids, c.offsets + c0, c.fill + c0, c.keys);                                           \
    else                                                                                                                                \
        hipLaunchKernelGGL(knn_self_list_kernel<KCV>, grid, block, 0, s, c.r, c.k, row_first + c0, mc, c.n, per, c.max_dist2, c.base, c.gids, \
                           c.offsets + c0, c.fill + c0, c.keys)
        KNN_KC_SWITCH(c.k, KNN_SELF_LIST)
#undef KNN_SELF_LIST
        return hipGetLastError();
    });
    if (e != hipSuccess)
        return e;
    if (!gate && c.ev1 && (e = hipEventRecord(c.ev1, s)) != hipSuccess)
        return e;
    return hipSuccess;
}

hipError_t knn_self_drop_launch(int m, int K, const u64 *lists, long long row_first, long long base, const unsigned *gids, u64 *out,
                                hipStream_t s)
{
    if (m <= 0 || K < 1 || K + 1 > KNN_TOPK_MAX || !lists || !out || row_first < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_self_drop_kernel, dim3((unsigned)m), dim3(KNN_WAVE), 0, s, lists, K, row_first, base, gids, out);
    return hipGetLastError();
}
