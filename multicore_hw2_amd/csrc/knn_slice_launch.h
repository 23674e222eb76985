// knn_slice_launch.h — the launch layer the exact slice scans share (knn_exact.hip: top-K, count and list, scalar and each;
// knn_select.hip; knn_masked.hip; knn_masked_lists.hip; knn_self.hip; knn_cluster.hip).  Every such scan is one wave per block,
// lanes = queries, rows as wave-uniform scalar loads, and is launched the same way: the queries in chunks of <= KNN_TOPK_CHUNK,
// the shard's rows in `slices` equal runs of `per` rows (the last shorter), grid = (slices, query groups of 64), the kernel in its
// KC form for the call's k.  Here, once: the switch over the KC forms, the chunk walk under a slice rule, and the fields every
// plan of such a call reports.  Host arithmetic and templates only: nothing here allocates or launches.
#pragma once

#include "knn_common.h"
#include "knn_radix_pick.h"   // KNN_RADIX_BINS: the select block's histogram

// The kernel form for k dimensions: KC = ceil(k / 16) chunks of 16 coordinates in registers up to k = 128, beyond it the generic
// form KC = 0.  CALL(KC) is a statement (or an if / else chain of launches) that names a kernel's <KC> instance.
#define KNN_KC_SWITCH(k, CALL)   \
    switch (((k) + 15) / 16) {   \
    case 1: CALL(1); break;      \
    case 2: CALL(2); break;      \
    case 3: CALL(3); break;      \
    case 4: CALL(4); break;      \
    case 5: CALL(5); break;      \
    case 6: CALL(6); break;      \
    case 7: CALL(7); break;      \
    case 8: CALL(8); break;      \
    default: CALL(0); break;     \
    }

// The slice rules: how many slices one chunk of mc queries cuts n rows into, and what a plan reports with them — the scan's LDS
// and, for the top-K scan, the bytes of its per-slice lists [slices][mc][K].
struct KnnCountSlices {   // count, list, fill and link scans (knn_count_slices)
    long long operator()(int mc, long long n, int num_cu) const { return knn_count_slices(mc, n, num_cu); }
    size_t lds_bytes() const { return 0; }
    size_t part_bytes(long long, int) const { return 0; }
};
struct KnnTopkSlices {    // the top-K scan of K <= KNN_TOPK_MAX (knn_topk_slices)
    int K;
    long long operator()(int mc, long long n, int num_cu) const { return knn_topk_slices(mc, K, n, num_cu); }
    size_t lds_bytes() const { return (size_t)K * KNN_WAVE * sizeof(u64); }
    size_t part_bytes(long long slices, int mc) const { return (size_t)slices * (size_t)mc * (size_t)K * sizeof(u64); }
};
struct KnnSelectSlices {  // a histogram pass of the radix select (knn_select_slices)
    long long operator()(int mc, long long n, int num_cu) const { return knn_select_slices(mc, n, num_cu); }
    size_t lds_bytes() const { return KNN_SELECT_HIST_WORDS * sizeof(unsigned); }
    size_t part_bytes(long long, int) const { return 0; }
};

// One chunk of a call's queries (the cluster sweep's "queries" are the shard's rows: long long) and its cut of the shard's rows.
struct SliceChunk {
    long long c0 = 0;        // the chunk's first query
    int mc = 0;              // its queries, <= KNN_TOPK_CHUNK
    long long slices = 0;    // the rule's slices for mc queries
    long long per = 0;       // rows of a slice: ceil(n / slices)
    dim3 grid;               // (slices, ceil(mc / KNN_WAVE))
};

// The chunk that starts at query c0 of m, n > 0 rows.
template <class Rule>
inline SliceChunk knn_slice_chunk(long long c0, long long m, long long n, int num_cu, const Rule &rule)
{
    SliceChunk ch;
    ch.c0 = c0;
    ch.mc = m - c0 < KNN_TOPK_CHUNK ? (int)(m - c0) : KNN_TOPK_CHUNK;
    ch.slices = rule(ch.mc, n, num_cu);
    ch.per = (n + ch.slices - 1) / ch.slices;
    ch.grid = dim3((unsigned)ch.slices, (unsigned)knn_divup(ch.mc, KNN_WAVE));
    return ch;
}

// each(chunk) for every chunk of m queries in order; stops at the first error and returns it.
template <class Rule, class F>
inline hipError_t knn_slice_chunks(long long m, long long n, int num_cu, const Rule &rule, F &&each)
{
    for (long long c0 = 0; c0 < m; c0 += KNN_TOPK_CHUNK) {
        const hipError_t e = each(knn_slice_chunk(c0, m, n, num_cu, rule));
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// What the plans of these calls report (SelfPlan, MaskedPlan, TopkLargePlan, ClusterPlan, CountPlan), from the same chunks.
// m > 0.  n <= 0: the chunks alone.  part_bytes: the first chunk's lists or the last's — the last, of fewer queries, may cut the
// rows finer; the chunks between are the first's.
struct SlicePlan {
    int chunks = 0, chunk_m = 0;     // launch sequences; queries of the first
    long long slices = 0, groups = 0;   // the first chunk's grid
    size_t lds_bytes = 0, part_bytes = 0;
};
template <class Rule>
inline SlicePlan knn_slice_plan(long long m, long long n, int num_cu, const Rule &rule)
{
    SlicePlan p;
    p.chunks = knn_divup(m, KNN_TOPK_CHUNK);
    p.chunk_m = m < KNN_TOPK_CHUNK ? (int)m : KNN_TOPK_CHUNK;
    if (n <= 0)
        return p;
    const SliceChunk first = knn_slice_chunk(0, m, n, num_cu, rule);
    const SliceChunk last = knn_slice_chunk((long long)(p.chunks - 1) * KNN_TOPK_CHUNK, m, n, num_cu, rule);
    p.slices = first.slices;
    p.groups = first.grid.y;
    p.lds_bytes = rule.lds_bytes();
    p.part_bytes = std::max(rule.part_bytes(first.slices, first.mc), rule.part_bytes(last.slices, last.mc));
    return p;
}
// ... for a call that is a top-K (K > 0) or a count / list (K <= 0) by its K.
inline SlicePlan knn_slice_plan(long long m, int K, long long n, int num_cu)
{
    return K > 0 ? knn_slice_plan(m, n, num_cu, KnnTopkSlices{K}) : knn_slice_plan(m, n, num_cu, KnnCountSlices{});
}

// The radix select of one large top-K call (knn_topk_large_launch, knn_select.hip; knn_masked_large_launch, knn_masked_lists.hip),
// chunk by chunk: the state's memset, per pass a histogram scan and the pick, the fill, the sort and — a folding call — the merge
// into the caller's keys.  c.ev0 is recorded behind the first chunk's memset, c.ev1 ahead of the last chunk's sort.  The two
// callers differ in the rows their scans walk:
//   hist(chunk under the select rule, the chunk's queries, pass, the pass's gate word or null)   launches one histogram scan;
//   fill(chunk under the count rule, the chunk's queries, list)                                  launches the fill.
// p: the plan the state in c.part is laid out by.  *tie_word <- the device word that is non-zero when the index word's passes ran
// on the last chunk.
template <class Hist, class Fill>
inline hipError_t knn_select_round(const TopkCall &c, const TopkLargePlan &p, const unsigned **tie_word, Hist &&hist, Fill &&fill)
{
    hipStream_t s = c.stream;
    unsigned char *st = (unsigned char *)c.part;
    const unsigned *gates = (const unsigned *)(st + p.gate_off);
    const hipError_t err = knn_slice_chunks(c.m, c.n, c.num_cu, KnnSelectSlices{}, [&](const SliceChunk &ch) {
        const float *qc = c.q + (size_t)ch.c0 * c.k;
        u64 *keys = c.keys + (size_t)ch.c0 * c.K;
        u64 *list = c.init ? keys : (u64 *)(st + p.list_off);
        hipError_t e = hipMemsetAsync(st, 0, p.state_bytes, s);
        if (e != hipSuccess)
            return e;
        if (c.ev0 && ch.c0 == 0)
            (void)hipEventRecord(c.ev0, s);
        for (int pass = 0; pass < KNN_RADIX_PASSES; ++pass) {
            hist(ch, qc, pass, pass == 0 ? (const unsigned *)nullptr : gates + pass);
            if ((e = hipGetLastError()) != hipSuccess)
                return e;
            if ((e = knn_select_pick_launch(p, c.part, ch.mc, pass, c.K, s)) != hipSuccess)
                return e;
        }
        fill(knn_slice_chunk(ch.c0, c.m, c.n, c.num_cu, KnnCountSlices{}), qc, list);
        if ((e = hipGetLastError()) != hipSuccess)
            return e;
        if (c.ev1 && ch.c0 + ch.mc == c.m)
            (void)hipEventRecord(c.ev1, s);
        if ((e = knn_topk_large_sort_launch(p, c.part, ch.mc, c.K, list, s)) != hipSuccess)
            return e;
        return c.init ? hipSuccess : knn_topk_merge_large_launch(ch.mc, c.K, list, keys, s);
    });
    if (err == hipSuccess && tie_word)
        *tie_word = gates + KNN_RADIX_DIST_PASSES;
    return err;
}
