// knn_common.h — shared declarations of the knn_mi355x library internals (gfx950 only).
#pragma once
#include <atomic>

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>

#define KNN_WAVE 64

typedef unsigned long long u64;

static constexpr u64 kKeyInit = 0x7F80000000000000ull;  // (+INF, index 0)

static inline int knn_divup(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- exact VALU kernels (knn_exact.hip) -----------------------------------
// Folds the nearest reference of refs[0..n_local) (global index base + i) for each of the m
// queries into keys[] with a 64-bit unsigned atomic min.  Every distance is computed with the
// v0 arithmetic (reference core.cu:44-49).  If `gate` is non-null the kernels return at once
// unless *gate != 0 (device-side fallback switch, so the query path never syncs with the host).
hipError_t knn_exact_launch(int k, int m, long long n_local, long long base, const float *q_dev,
                            const float *r_dev, u64 *keys_dev, int num_cu, const unsigned *gate,
                            hipStream_t stream);

// Exact scan of the rows listed in list_dev[0..count) (global index = base + row).
hipError_t knn_exact_gather_launch(int k, int m, unsigned count, long long base, const float *q_dev,
                                   const float *r_dev, const unsigned *list_dev, u64 *keys_dev, int num_cu,
                                   const unsigned *gate, hipStream_t stream);

// Exact re-rank of the filter's candidate records (see knn_rerank_kernel).
// Record lists [list_base[i], list_base[i+1]) belong to piece i of the batch, whose records number their
// queries from qrow_base[i] (see knn_filter_query_plan); unused entries have list_base = ~0.
struct RerankPieces {
    unsigned list_base[4] = {0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    unsigned qrow_base[4] = {0u, 0u, 0u, 0u};
    int n = 1;
};

// perm (nullable): records name positions of a permuted layout; perm[position] = row (~0u = padding), and n
// is then the number of positions.
// ovf_cap != 0: records[ovf_base ..) hold ctl[KNN_CTL_RECORDS] more records (capped at ovf_cap) that belong to no list.
hipError_t knn_rerank_launch(int k, long long n, const float *q_dev, const float *r_dev, long long base,
                             const u64 *records, const unsigned short *record_rows, const unsigned *counts,
                             unsigned nlists, unsigned slice, unsigned *ctl, u64 *keys, RerankPieces pieces,
                             hipStream_t stream, const unsigned *perm = nullptr, unsigned ovf_base = 0u,
                             unsigned ovf_cap = 0u);

hipError_t knn_keys_fill_launch(u64 *keys_dev, int m, hipStream_t stream);
hipError_t knn_keys_unpack_launch(const u64 *keys_dev, int m, int *out_dev, hipStream_t stream);
hipError_t knn_synth_fill_launch(float *dst, long long count, u64 seed, long long first,
                                 hipStream_t stream);

// ---- top-K (knn_exact.hip) ---------------------------------------------------
#define KNN_TOPK_MAX 64        // largest K of knn_index_query_topk
#define KNN_TOPK_CHUNK 65536   // queries per scan launch of the exact top-K (bounds the per-slice lists)
// Bytes of the per-slice list buffer the exact top-K scan of m queries, K neighbours, n rows uses (part of a workspace slot).
size_t knn_topk_part_bytes(int m, int K, long long n, int num_cu);
// The limit key of a radius: a key is within max_dist2 >= 0 (not NaN; -0 counts as 0) exactly when it is below
// (bits(max_dist2) + 1) << 32 — the fp32 compare E <= max_dist2 on the key's high word, equality inside.  +INF gives a key above
// KNN_KEY_INIT: no limit.
static inline u64 knn_topk_limit_key(float max_dist2)
{
    unsigned bits;
    memcpy(&bits, &max_dist2, sizeof bits);
    return ((u64)(bits & 0x7FFFFFFFu) + 1ull) << 32;
}
// One top-K call (knn_index_query_topk, knn_index_query_topk_within) as every way that answers it takes it: query_topk
// (knn_api.cpp) fills it once, the launchers read it and add only what is their own.
struct TopkCall {
    int k = 0, m = 0, K = 0;       // dimension, queries, neighbours per query
    long long n = 0, base = 0;     // the shard's rows; global number of row 0 ...
    const unsigned *gids = nullptr;   // ... or, cell-range shards (base 0), of every row; null: base + row
    const float *q = nullptr, *r = nullptr;   // device [m][k], [n][k]
    u64 *keys = nullptr;           // device [m][K]: written (init) or folded into, sorted lists
    int init = 0;
    int num_cu = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // nullable: bracket the way's dominant kernel
    float max_dist2 = INFINITY;    // the radius, squared (>= 0, never -0); +INF: a plain call
    // the slot's scratch (knn_topk_scratch_plan): the exact top-K scan's per-slice lists; the filter ways' candidate lists
    // [m][ccap] and counters [m] — on the grid way cand is a folding call's lists [m][K], ccount null
    u64 *part = nullptr;
    size_t part_bytes = 0;
    u64 *cand = nullptr;
    unsigned *ccount = nullptr;
    unsigned ccap = 0;

    bool within() const { return max_dist2 < INFINITY; }
    // the one place a radius becomes a limit key: only keys below it are candidates; KNN_KEY_INIT = none
    u64 limit_key() const { return within() ? knn_topk_limit_key(max_dist2) : kKeyInit; }
    // the same call writing its lists to `lists` from scratch (a way whose answer something behind it turns into the keys)
    TopkCall writing(u64 *lists) const
    {
        TopkCall c = *this;
        c.keys = lists;
        c.init = 1;
        return c;
    }
    // queries [q0, q0 + mb) of the call: a pass of the cell-pruned way
    TopkCall pass(int q0, int mb) const
    {
        TopkCall c = *this;
        c.m = mb;
        c.q = q + (size_t)q0 * k;
        c.keys = keys + (size_t)q0 * K;
        c.cand = cand + (size_t)q0 * ccap;
        c.ccount = ccount + q0;
        return c;
    }
};
// c.keys[m][K] <- the K smallest of (keys unless init, this shard's finite-distance rows), sorted; v0 arithmetic.  c.part:
// c.part_bytes of scratch (knn_topk_part_bytes), stream-ordered.
// gate != nullptr: the launches do nothing unless *gate != 0 (the filter top-K's FALLBACK word, the grid's give-up word).
// limit: the scan carries the call's radius — only rows whose key is below c.limit_key() are candidates; false: every row is (the
// ways that clip behind).  The keys the call folds into are the caller's and are not clipped.
hipError_t knn_exact_topk_launch(const TopkCall &c, const unsigned *gate, bool limit);
// keys[j] <- lists[j] with every key >= lim turned into KNN_KEY_INIT (init), or the K smallest of that and keys[j] (a fold).
hipError_t knn_topk_clip_launch(int m, int K, const u64 *lists, u64 lim, u64 *keys, int init, hipStream_t stream);
// Filter top-K: umin[0][q] <- K-th smallest finite per-block minimum (one row for knn_thr_kernel).
hipError_t knn_topk_umin_launch(float *umin, int nb, int m_padded, int K, hipStream_t stream);
// The records side of a filter top-K batch: what the scan left in its workspace and the layout it scanned.
struct TopkRecords {
    long long positions = 0;       // rows the records can name (a cell-sorted layout: its padded positions)
    const u64 *rec = nullptr;      // nlists slices of `slice` records; counts[i]: records list i produced (may exceed slice)
    const unsigned short *rec_rows = nullptr;   // nullable: a row mask next to every record
    const unsigned *counts = nullptr;
    unsigned nlists = 0, slice = 0;
    unsigned *ctl = nullptr;       // the batch's control words (FALLBACK)
    RerankPieces pieces;
    const unsigned *perm = nullptr;   // nullable: the records name positions of a permuted layout
    unsigned n_outliers = 0;       // rows outside the robust box: never in the scan, every one a candidate
    const unsigned *outliers = nullptr;
    // the cell-pruned scan's shared overflow area, re-ranked as a list of one: ovf_count records (a device word) at ovf_rec,
    // room ovf_slice — more than that raises FALLBACK
    const u64 *ovf_rec = nullptr;
    const unsigned *ovf_count = nullptr;
    unsigned ovf_slice = 0;
    // the cell-pruned top-K's distance gate: the pass's Dup_q values and sigma^-2 (knn_topk_gate); null: every finite key is a
    // candidate (the filter top-K).  With the gate: the layout's norms by position (+INF: padding, out-of-box rows — not
    // re-ranked), and c.gids (cell-range shards, base 0) become the candidates' index half
    const float *gate_dup = nullptr;
    float inv_sigma2 = 0.0f;
    const float *pos_norms = nullptr;
};
// Filter top-K after the scan: records + outlier rows -> per-query candidate lists (overflow -> FALLBACK), then, unless
// FALLBACK, c.keys <- K smallest of (keys unless init, candidates).
hipError_t knn_topk_filter_finish(const TopkCall &c, const TopkRecords &rs);
// b[j] <- the K smallest of a[j] and b[j] (both sorted lists of K keys), sorted.
hipError_t knn_topk_merge_launch(int m, int K, const u64 *a, u64 *b, hipStream_t stream);

// ---- counts within a radius (knn_index_count_within; DESIGN §4.6 "Counts within a radius") -------------------------------------
// One count call as every way that answers it takes it: count_within (knn_api.cpp) fills it once.
struct CountCall {
    int k = 0, m = 0;
    long long n = 0;               // the shard's rows
    const float *q = nullptr, *r = nullptr;   // device [m][k], [n][k]
    unsigned *counts = nullptr;    // device [m], the caller's: every way ADDS to it (an init call zeroes it ahead of the way's launches)
    float max_dist2 = INFINITY;    // the radius, squared (>= 0, never -0; +INF: every row with a finite distance)
    int num_cu = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // nullable: bracket the way's dominant kernel
    unsigned *scratch = nullptr;   // the slot's count scratch [m] (the grid and cell ways; the exact way does not use it)
    // nullable; a call with a radius per query (2j): device [m], query j's radius.  max_dist2 is then the call's cap, and a row is
    // a hit when E <= radii[j] and E <= max_dist2; every way launches its each-form kernels (knn_each_radius.h)
    const float *radii = nullptr;
    // >= 0: a routed call about the shard's own rows (2k): query j is LOCAL row self_first + j (q = r + self_first * k), which is
    // no candidate for itself; the grid and cell ways launch their self forms and the gated self-scan.  -1: a plain call
    long long self_first = -1;
    // nullable; a routed call over a subset of the rows (2l): device (n + 31) / 32 words, bit i % 32 of word i / 32 admits LOCAL
    // row i.  The grid and cell ways launch their masked forms and the gated masked scan, which works in mask_scratch (the slot's
    // mask scratch, MaskedPlan::mask_bytes).  Not with radii, not with self_first >= 0
    const unsigned *mask = nullptr;
    u64 *mask_scratch = nullptr;

    // queries [q0, q0 + mb) of the call: a pass of the cell-pruned way (the mask belongs to the rows, not to the queries: it stays)
    CountCall pass(int q0, int mb) const
    {
        CountCall c = *this;
        c.m = mb;
        c.q = q + (size_t)q0 * k;
        c.counts = counts + q0;
        c.scratch = scratch + q0;
        c.radii = radii ? radii + q0 : nullptr;
        c.self_first = self_first < 0 ? -1 : self_first + q0;   // (the own rows advance with the queries)
        return c;
    }
};
// Slices of the shard the exact count scan splits one chunk of mc queries into: the K <= 16 top-K scan's rule (about 32 waves
// per CU, >= 1024 rows each) without the list room.  Host arithmetic only.
long long knn_count_slices(int mc, long long n, int num_cu);
// c.counts[j] += #{rows of the shard with a finite v0 distance E <= c.max_dist2}.  gate != nullptr: the launches do nothing unless
// *gate != 0 (the grid way's give-up word).
hipError_t knn_exact_count_launch(const CountCall &c, const unsigned *gate);
// counts[j] += scratch[j] for j < m unless *giveup != 0: the grid way's commit, the opposite gate of the exact count behind it.
hipError_t knn_count_commit_launch(int m, const unsigned *scratch, unsigned *counts, const unsigned *giveup, hipStream_t stream);
// A cell-pruned count pass behind its record-only scan: every row of every record (the slices, then the shared overflow area as a
// list of one; rs.perm and rs.pos_norms set, rs.gate_dup unused) and every out-of-box row with v0's arithmetic -> qcount[j] (the
// pass's scratch, zero on entry), then the commit, gated on no FALLBACK.  An over-full record area raises FALLBACK.
hipError_t knn_count_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount);

// ---- lists within a radius (knn_index_list_within; DESIGN §4.6 "Lists within a radius") -----------------------------------------
// One list call as every way that answers it takes it: the count call's fields, where the hits go and the number a key carries.
// knn_index_list_within (knn_api.cpp) fills it once.
struct ListCall {
    int k = 0, m = 0;
    long long n = 0, base = 0;     // the shard's rows; global number of row 0 ...
    const unsigned *gids = nullptr;   // ... or, cell-range shards (base 0), of every row; null: base + row
    const float *q = nullptr, *r = nullptr;   // device [m][k], [n][k]
    const u64 *offsets = nullptr;  // device [m + 1], the caller's: segment j of keys is [offsets[j], offsets[j + 1])
    unsigned *fill = nullptr;      // device [m], the caller's cursor: every way ADDS this shard's hits (an init call zeroes it first)
    u64 *keys = nullptr;           // device, the caller's: a hit that reserved place p < room is stored at keys[offsets[j] + p]
    float max_dist2 = INFINITY;    // the radius, squared (>= 0, never -0; +INF: every row with a finite distance)
    int num_cu = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // nullable: bracket the way's dominant kernel
    unsigned *scratch = nullptr;   // the slot's count scratch [m]: the scratch cursor of the grid and cell ways (the exact way does not use it)
    const float *radii = nullptr;  // nullable; a radius per query, device [m], max_dist2 the cap: as CountCall::radii
    long long self_first = -1;     // >= 0: a routed call about the shard's own rows, as CountCall::self_first
    const unsigned *mask = nullptr;   // nullable; a routed call over a subset of the rows, as CountCall::mask ...
    u64 *mask_scratch = nullptr;      // ... and the slot's mask scratch (MaskedListsPlan::cut.mask_bytes)

    // queries [q0, q0 + mb) of the call: a pass of the cell-pruned way (offsets are absolute: keys stays; so does the mask, which
    // belongs to the rows)
    ListCall pass(int q0, int mb) const
    {
        ListCall c = *this;
        c.m = mb;
        c.q = q + (size_t)q0 * k;
        c.offsets = offsets + q0;
        c.fill = fill + q0;
        c.scratch = scratch + q0;
        c.radii = radii ? radii + q0 : nullptr;
        c.self_first = self_first < 0 ? -1 : self_first + q0;   // (the own rows advance with the queries)
        return c;
    }
};
// Every row of the shard with a finite v0 distance E <= c.max_dist2 reserves p = c.fill[j]++ and, when p is below the segment's
// room, stores its key at c.keys[c.offsets[j] + p].  Slices and chunks of queries as knn_exact_count_launch.  gate != nullptr: the
// launches do nothing unless *gate != 0.
hipError_t knn_exact_list_launch(const ListCall &c, const unsigned *gate);
// fill[j] = cursor[j] for j < m unless *giveup != 0: the commit of the grid way and of a cell-pruned pass, the opposite gate of the
// exact list behind it.
hipError_t knn_list_commit_launch(int m, const unsigned *cursor, unsigned *fill, const unsigned *giveup, hipStream_t stream);
// A cell-pruned list pass behind its record-only scan (knn_count_records_finish's walk): every hit reserves its place in c.scratch
// — on entry a copy of c.fill — and stores its key behind it; then the commit, gated on no FALLBACK.
hipError_t knn_list_records_finish(const ListCall &c, const TopkRecords &rs);
// offsets[0] = 0, offsets[j + 1] = offsets[j] + counts[j]: one block, a 64-bit running sum over chunks of the counts.
hipError_t knn_counts_to_offsets_launch(const unsigned *counts, int m, u64 *offsets, hipStream_t stream);
// The first min(fill[j], room of segment j) keys of every segment ascending: one block per segment, a bitonic network in LDS up to
// KNN_SORT_LDS_KEYS keys and in global memory beyond.
#define KNN_SORT_LDS_KEYS 4096
hipError_t knn_keys_sort_segments_launch(int m, const u64 *offsets, const unsigned *fill, u64 *keys, hipStream_t stream);
// dist2[j] = the float in the high word of keys[j * K + column] (a padding key: +INF), j < m: a column of a top-K call's lists as
// the radii of a call with a radius per query (knn_keys_column_dist2).
hipError_t knn_keys_column_dist2_launch(const u64 *keys, int m, int K, int column, float *dist2, hipStream_t stream);
// knn_count_records_finish and knn_list_records_finish for a pass that carries radii (c.radii; knn_each.hip): the same walks with
// the radius of the record's own query, the same commit.  The plain functions hand such a pass over after their own checks.
hipError_t knn_count_each_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount);
hipError_t knn_list_each_records_finish(const ListCall &c, const TopkRecords &rs);
// ... and for a pass of a routed call about the shard's own rows (c.self_first >= 0; knn_self_routed.hip): the same walks, a
// candidate whose LOCAL row is the record's query's own (c.self_first + the pass's query number) dropped; c.radii null: every
// query's radius is c.max_dist2.  The plain functions hand such a pass over after their own checks, ahead of the each-forms.
hipError_t knn_count_self_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount);
hipError_t knn_list_self_records_finish(const ListCall &c, const TopkRecords &rs);
// ... and for a pass of a routed call over a subset of the rows (c.mask; knn_masked_routed.hip): the scalar forms' walks, a candidate
// whose LOCAL row's bit in c.mask is clear dropped.  The plain functions hand such a pass over first of all; with c.radii or
// c.self_first >= 0 it is hipErrorInvalidValue.
hipError_t knn_count_masked_records_finish(const CountCall &c, const TopkRecords &rs, unsigned *qcount);
hipError_t knn_list_masked_records_finish(const ListCall &c, const TopkRecords &rs);

// ---- top-K beyond 64 (knn_select.hip; knn_index_query_topk_large; DESIGN §4.6 "Top-K beyond 64") --------------------------------
#define KNN_TOPK_LARGE_MAX 4096   // largest K of knn_index_query_topk_large (= KNN_SORT_LDS_KEYS: a list sorts in LDS)
#define KNN_SELECT_WAVES 8        // waves of a select block: they hold the same 64 queries and split the slice's rows
#define KNN_SELECT_BLOCK (KNN_SELECT_WAVES * KNN_WAVE)
#define KNN_SELECT_HIST_WORDS (KNN_RADIX_BINS * KNN_WAVE)   // a select block's LDS histogram [bin][lane]: 64 KiB (KNN_RADIX_BINS: knn_radix_pick.h)
// Everything one large call launches with and the slot's scratch it needs: the one place both are decided
// (knn_debug_topk_large_plan shows it).  The scratch, per chunk of <= KNN_TOPK_CHUNK queries (mcp = the chunk's queries rounded up
// to whole waves): the per-query histograms [256][mcp] unsigned (bin-major), prefix [mcp] u64, need [mcp], cursor [mcp], the
// passes' gate words [8], and — a folding call — the chunk's lists [chunk_m][K].
struct TopkLargePlan {
    int chunks = 0, chunk_m = 0;     // launches sequences; queries of the largest chunk
    long long mcp = 0;               // chunk_m rounded up to a multiple of KNN_WAVE
    long long slices = 0;            // blocks along the rows of one select pass (the largest chunk)
    int dist_passes = 0, index_passes = 0;
    size_t lds_bytes = 0;            // static LDS of the select kernel: the block's histogram
    size_t hist_off = 0, prefix_off = 0, need_off = 0, cursor_off = 0, gate_off = 0, state_bytes = 0, list_off = 0;
    size_t scratch_bytes = 0;
    long long launches_clean = 0, launches_ties = 0;   // launches that do work: no query's cut inside a distance class / some
};
TopkLargePlan knn_topk_large_plan(int k, int m, int K, long long n, int num_cu, bool init);
// c.keys[m][K] <- the K smallest of (keys unless c.init, this shard's candidates: finite v0 distance E <= c.max_dist2), sorted,
// padded with KNN_KEY_INIT; 1 <= K <= KNN_TOPK_LARGE_MAX.  c.part: p.scratch_bytes of the slot's scratch, stream-ordered.
// *tie_word <- the device word that is non-zero when the index word's passes ran on the last chunk.
hipError_t knn_topk_large_launch(const TopkCall &c, const TopkLargePlan &p, const unsigned **tie_word);
// b[j] <- the K smallest of a[j] and b[j] (sorted lists of K <= KNN_TOPK_LARGE_MAX keys), sorted, in place: one block per query.
hipError_t knn_topk_merge_large_launch(int m, int K, const u64 *a, u64 *b, hipStream_t stream);
// ---- queries over a subset of the rows (knn_masked.hip; DESIGN §4.6 "Over a subset of the rows") --------------------------------
// The slices of the exact top-K scan for one chunk of mc queries (knn_exact.hip's rule, what knn_topk_part_bytes sizes `part` by).
long long knn_topk_slices(int mc, int K, long long n, int num_cu);
// keys[q] <- the K smallest of (keys[q] unless init, lists[0][q] .. lists[nl - 1][q]), sorted: knn_topk_select_kernel, the fold of
// a scan's per-slice lists [nl][m][K].
hipError_t knn_topk_select_launch(const u64 *lists, int nl, int m, int K, u64 *keys, int init, hipStream_t stream);
// Everything one masked call launches with and the slot's scratch it needs: the one place both are decided
// (knn_debug_masked_plan shows it).  K = 0: a count call.  The mask scratch: the prefix P [granules + 1] u64, then the granules'
// admitted rows [granules] unsigned.
struct MaskedPlan {
    long long granules = 0;          // ceil(n / 1024)
    long long slices = 0;            // blocks along the rows for the first chunk of queries: the unmasked exact scan's number
    int chunks = 0, chunk_m = 0;     // launch sequences of <= KNN_TOPK_CHUNK queries; queries of the first
    size_t lds_bytes = 0;            // dynamic LDS of the scan: the top-K's sorted columns [K][64] u64; a count has none
    size_t counts_off = 0, mask_bytes = 0;   // where the granule counts start in the mask scratch; its bytes
    size_t part_bytes = 0;           // the top-K scan's per-slice lists (knn_topk_part_bytes); a count has none
    long long launches = 0;          // kernel launches of an init call: granule counts, prefix, per chunk the scan (and the select)
};
MaskedPlan knn_masked_plan(int k, int m, int K, long long n, int num_cu, bool init);
// c.keys[m][K] <- the K smallest of (keys unless c.init, the rows of the shard whose mask bit is set and whose v0 distance E is
// finite and <= c.max_dist2), sorted, padded with KNN_KEY_INIT; 1 <= K <= KNN_TOPK_MAX.  mask: (c.n + 31) / 32 words, bit i % 32
// of word i / 32 admits local row i.  scratch: p.mask_bytes; c.part: p.part_bytes; both stream-ordered.  c.n > 0.
hipError_t knn_masked_topk_launch(const TopkCall &c, const MaskedPlan &p, const unsigned *mask, u64 *scratch);
// c.counts[j] += the number of those rows.  c.n > 0.  gate != nullptr: every kernel of the sequence — the prefix's too — returns at
// once unless *gate != 0 (the exact answer behind a pruned way of a routed masked call); the call's events are not recorded then.
hipError_t knn_masked_count_launch(const CountCall &c, const MaskedPlan &p, const unsigned *mask, u64 *scratch,
                                   const unsigned *gate = nullptr);
// The mask bits of rows[0 .. count) that lie in 0 .. n - 1 <- value (0 or 1).
hipError_t knn_mask_set_rows_launch(long long n, const unsigned *rows, long long count, int value, unsigned *mask, hipStream_t stream);
// The granule counts and their prefix of one call's mask into the mask scratch (p.mask_bytes): what every masked call launches
// first, once, ahead of every chunk and pass.  n > 0.  gate: as knn_masked_count_launch's.
hipError_t knn_masked_prefix_launch(const MaskedPlan &p, long long n, const unsigned *mask, u64 *scratch, hipStream_t stream,
                                    const unsigned *gate = nullptr);

// ---- lists and top-K beyond 64 over a subset of the rows (knn_masked_lists.hip; DESIGN §4.6 "Lists and large K over a subset of
// the rows") ------------------------------------------------------------------------------------------------------------------
// The select's pieces that do not look at rows (knn_select.hip), shared with the select over a subset: the slices of one pass over
// a chunk of mc queries; the pick of one pass and the sort of the filled lists on the state in `scratch` (laid out by p).
long long knn_select_slices(int mc, long long n, int num_cu);
hipError_t knn_select_pick_launch(const TopkLargePlan &p, u64 *scratch, int mc, int pass, int K, hipStream_t stream);
hipError_t knn_topk_large_sort_launch(const TopkLargePlan &p, const u64 *scratch, int mc, int K, u64 *list, hipStream_t stream);
// Everything a masked list call (K = 0) or a masked large call (1 <= K <= KNN_TOPK_LARGE_MAX) launches with and the slot's scratch
// it needs: the one place both are decided (knn_debug_masked_lists_plan shows it).  cut: the masked count's plan for the same
// inputs — granules, chunks, the mask scratch and, for a list call, the slices: the count pass and the list pass cut the shard
// identically.  sel: the unmasked large call's plan — the select's state and a fold's lists in the slot's large scratch.
struct MaskedListsPlan {
    MaskedPlan cut;
    TopkLargePlan sel;               // a list call: all zero
    long long slices = 0;            // blocks along the rows of the first chunk's scan: knn_count_slices / the select's slices
    int slice_waves = 0;             // waves of a block that each take their own admitted-row slice: 1 / KNN_SELECT_WAVES
    size_t lds_bytes = 0;            // LDS of the scan: none / the select block's histogram
    size_t select_bytes = 0;         // bytes of the slot's large scratch: 0 / sel.scratch_bytes
    long long launches = 0;          // an init call whose index passes stay gated off: granule counts, prefix, and per chunk the
                                     // list scan / sel.launches_clean (the state's memset counted as there)
};
MaskedListsPlan knn_masked_lists_plan(int k, int m, int K, long long n, int num_cu, bool init);
// knn_exact_list_launch's contract over the rows whose mask bit is set.  scratch: p.cut.mask_bytes, stream-ordered.  c.n > 0.
// gate: as knn_masked_count_launch's.
hipError_t knn_masked_list_launch(const ListCall &c, const MaskedListsPlan &p, const unsigned *mask, u64 *scratch,
                                  const unsigned *gate = nullptr);
// knn_topk_large_launch's contract over the rows whose mask bit is set.  scratch: p.cut.mask_bytes; c.part: p.select_bytes.  c.n > 0.
hipError_t knn_masked_large_launch(const TopkCall &c, const MaskedListsPlan &p, const unsigned *mask, u64 *scratch,
                                   const unsigned **tie_word);

// ---- queries about the shard's own rows (knn_self.hip; DESIGN §4.6 "About the shard's own rows") --------------------------------
// Everything one self call launches with and the slot's scratch it needs: the one place both are decided (knn_debug_self_plan
// shows it).  m: the call's rows (its queries); K >= 1: a top-K call, K <= 0: a count or a list call.  Chunks, slices, LDS and the
// per-slice lists are the plain exact scan's for m queries, so the slot's buffers are sized as before.
struct SelfPlan {
    int chunks = 0, chunk_m = 0;     // launch sequences of <= KNN_TOPK_CHUNK rows; rows of the first
    long long slices = 0;            // blocks along the shard's rows for the first chunk: knn_topk_slices / knn_count_slices
    long long groups = 0;            // query groups of 64 of the first chunk: the grid's other side, one window each
    size_t lds_bytes = 0;            // dynamic LDS of the scan: the top-K's sorted columns [K][64] u64; count and list have none
    size_t part_bytes = 0;           // the top-K scan's per-slice lists; count and list have none
    long long launches = 0;          // kernel launches of an init call on the self-scan: per chunk the scan (and the select)
    size_t through_bytes = 0;        // top-K, K + 1 <= KNN_TOPK_MAX: the through way's lists [m][K + 1], plus [m][K] for a folding call
};
SelfPlan knn_self_plan(int k, int m, int K, long long n, int num_cu, bool init);
// The three exact self-scans: the contracts of knn_exact_topk_launch (limit = true), knn_exact_count_launch and
// knn_exact_list_launch with query j = local row row_first + j of the shard, which is no candidate for itself (identity by local
// row number: other copies of the row stay candidates).  c.q is not read.  0 <= row_first, row_first + c.m <= c.n.
hipError_t knn_self_topk_launch(const TopkCall &c, long long row_first);
// gate != nullptr (count and list): the launches do nothing unless *gate != 0 — the exact answer behind the grid way and behind a
// cell-pruned pass of a routed self call, as knn_exact_count_launch's gate; the call's events are not recorded then.
hipError_t knn_self_count_launch(const CountCall &c, long long row_first, const unsigned *gate = nullptr);
hipError_t knn_self_list_launch(const ListCall &c, long long row_first, const unsigned *gate = nullptr);
// The exact answer behind a pruned way, gated: the masked scan for a routed masked call (c.mask; the plan is host arithmetic on the
// pass's own m — the mask scratch's layout depends on the rows alone), the self-scan for a routed self call (c.self_first >= 0),
// else the exact count / list.
static inline hipError_t knn_gated_count_launch(const CountCall &c, const unsigned *gate)
{
    if (c.mask)
        return knn_masked_count_launch(c, knn_masked_plan(c.k, c.m, 0, c.n, c.num_cu, false), c.mask, c.mask_scratch, gate);
    return c.self_first >= 0 ? knn_self_count_launch(c, c.self_first, gate) : knn_exact_count_launch(c, gate);
}
static inline hipError_t knn_gated_list_launch(const ListCall &c, const unsigned *gate)
{
    if (c.mask)
        return knn_masked_list_launch(c, knn_masked_lists_plan(c.k, c.m, 0, c.n, c.num_cu, false), c.mask, c.mask_scratch, gate);
    return c.self_first >= 0 ? knn_self_list_launch(c, c.self_first, gate) : knn_exact_list_launch(c, gate);
}
// out[j][0 .. K) <- lists[j][0 .. K] (sorted, K + 1 <= KNN_TOPK_MAX keys) without the real key that carries the global number of
// local row row_first + j (base + row, or gids[row]) — without the last key when there is none.
hipError_t knn_self_drop_launch(int m, int K, const u64 *lists, long long row_first, long long base, const unsigned *gids, u64 *out,
                                hipStream_t stream);

// ---- MFMA filter + exact re-rank (knn_filter.hip) ---------------------------
// Device-side control words of one filter query (FilterState::ctl).
enum {
    KNN_CTL_FALLBACK = 0,  // != 0: the exact kernels must scan the whole shard (filter unusable)
    KNN_CTL_RECORDS = 1,   // records appended to the SHARED overflow area behind the waves' slices (cell-pruned path)
    // words 2..4 are the out[0..2] window of knn_frag_kernel for the query batch
    KNN_CTL_AMAX = 2,      // float bits: max |scaled query coordinate| in fp16
    KNN_CTL_QNMAX = 3,     // float bits: max fp32 squared norm of the fp16 query rows
    KNN_CTL_QBAD = 4,      // != 0: a query coordinate is non-finite or out of fp16 range
    KNN_CTL_CELLS = 5,     // != 0: this batch went through the cell-pruned scan
    KNN_CTL_WIDE_SEEDS = 6,  // cell-pruned path: queries whose seed cells held no row (bounded by a strided sample instead)
    KNN_CTL_DENSE_CELLS = 7, // cell-pruned path: cells whose query list outgrew its LDS room (scored against the whole batch)
    KNN_CTL_EXACT_CELLS = 8, // cell-pruned path, != 0: more candidates than the record buffers hold (the fp16 scores cannot tell
                             // the rows of a tight cluster apart): the listed (cell, query) pairs are evaluated exactly instead
    KNN_CTL_SCAN_DONE = 9,   // cell-pruned path: blocks of the scan that have finished (the last one finalises a clean batch)
    KNN_CTL_TAIL_DONE = 10,  // cell-pruned path: blocks of the tail kernel that have finished
    KNN_CTL_DEFERRED = 11,   // cell-pruned path, != 0: some wave of the scan left a long record list to the tail kernel
    KNN_CTL_TOTAL = 12,      // cell-pruned path: records the scan's waves have published so far (steps of 64 per wave)
    KNN_CTL_WORDS = 13
};

#define KNN_SLOTS 8  // independent query workspaces per index: up to eight batches may be in flight
#define KNN_RECORD_CAPACITY (1u << 22)   // records a workspace holds (FilterWorkspace::records: 8 B each + 2 B row mask)
#define KNN_MAX_LISTS (1u << 16)         // record lists (= scan waves) a workspace has counters for (FilterWorkspace::counts)

// Per-batch scratch of the filter path (one per slot).
struct FilterWorkspace {
    int m_cap = 0;
    void *qry_frags = nullptr; // device [qtiles][kt][64] x 16 B: B operands (-2 * scaled query)
    float *qry_norms = nullptr;// device [qtiles*32]
    float *qry_amax = nullptr; // device [qtiles*32]: max |scaled fp16 coordinate| of each query
    float *thr = nullptr;      // device [4][qtiles*32]: thresholds | margins | floors | running thresholds (ordered uints) — the
                               // last three feed the deep-K scan's in-launch tightening (knn_filter.hip, "running thresholds")
    unsigned *ctl = nullptr;   // device [3][KNN_CTL_WORDS]: block 0 = the full-scan path (reset by its fragment kernel);
                               // blocks 1, 2 alternate between the batches of the cell-pruned path, whose first
                               // kernel clears the block the NEXT batch will use (no reset launch, no race with
                               // the flags its own waves raise)
    unsigned *ctl_cur = nullptr; // the block the most recent batch on this slot used (statistics)
    unsigned cell_batches = 0; // cell-pruned batches issued on this slot (picks the ctl block)
    u64 *records = nullptr;    // device [rec_cap]: nlists slices of `slice` records, one per wave
    RerankPieces pieces;
    bool has_rows = false;     // the last scan wrote a row mask next to every record
    unsigned rec_cap = 0;
    unsigned *counts = nullptr;// device [nlists]: records each wave produced (may exceed slice)
    unsigned nlists = 0, slice = 0;
    unsigned ovf_base = 0, ovf_cap = 0; // cell-pruned path: records [ovf_base, ovf_base + ovf_cap) take what a wave's slice
                               // cannot hold (a thousand copies of one query all hit the same tile); 0 = none
    float *umin = nullptr;     // device [sample blocks][m_padded]: per-block minima of the sample pass
    size_t umin_cap = 0;       // floats allocated in umin
    unsigned *qpart = nullptr; // device [3 * query blocks]: {max |coord|, max norm, #bad} per block
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;  // optional: bracket the filter kernel
    // cell-pruned scan (CellIndex): per-cell query lists and the per-query pruning tables of the batch
    unsigned *cell_counts = nullptr;       // device [ncells]
    unsigned short *cell_lists = nullptr;  // device [ncells][cap]
    float *dup = nullptr;                  // device [m_cap]: largest scaled squared distance a candidate can have
    float *lo_tab = nullptr, *hi_tab = nullptr;  // device [m_cap][2^sa], [2^(bits-sa)][m_cap]
    float *lo_min = nullptr;               // device [2^sa / 64][m_cap]: the smallest of every 64 consecutive entries of a query's low table
    int cell_m_cap = 0;
};

// 16-wide K steps of the fp16 layouts for dimension k: 1, 2, 4, 8 (register / LDS-tiled scans), 16 and 32 (LDS-tiled scan with
// two / one block of queries per wave: the B operands of k = 512 fill a wave's registers), beyond that a multiple of 8 (K walked
// in chunks of 128 dimensions, knn_filter_chunked_kernel); 0 = no filter for this k.
#define KNN_FILTER_MAX_K 4096
#define KNN_CELL_ITEM_TILES 18     // two passes of the scan (CELL_TILES_PER_PASS = 9)
static inline int knn_kt_of(int k)
{
    return k < 1 ? 0 : k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 4 : k <= 128 ? 8 : k <= 256 ? 16 : k <= 512 ? 32
         : k <= KNN_FILTER_MAX_K ? 8 * ((k + 127) / 128) : 0;
}

// Global geometry of a CELL-RANGE sharded set (round 4; include/knn_mi355x.h, knn_geom_*): ONE grid for the whole reference
// set — cuts, centre and scale from a sample of the global set, identical on every rank — whose cell codes are split into
// contiguous ranges, one per rank.  A rank's index sorts ITS rows into ITS cells of that grid, so the ranks' scans add up to
// the scan of one GPU holding everything (index-range shards re-grid n / N rows at 1 / N of the resolution and do 3.5x the
// work at N = 8: profiles/r04_shard_sim.txt).
#define KNN_SEED_HEADER_BYTES 256u
// Rank r of nranks owns the codes [first(r), first(r + 1)) of a grid of ncells cells, first(r) = r ncells / nranks rounded
// down to a multiple of gran (whole entries of the high pruning table; first(nranks) = ncells).
__host__ __device__ static inline unsigned knn_shard_first_cell(unsigned r, unsigned ncells, unsigned nranks, unsigned gran)
{
    if (r >= nranks)
        return ncells;
    return (unsigned)((unsigned long long)r * ncells / nranks) / gran * gran;
}
__host__ __device__ static inline unsigned knn_shard_owner(unsigned code, unsigned ncells, unsigned nranks, unsigned gran)
{
    unsigned r = (unsigned)((unsigned long long)code * nranks / ncells);
    if (r >= nranks)
        r = nranks - 1u;
    while (r > 0u && code < knn_shard_first_cell(r, ncells, nranks, gran))
        --r;
    while (r + 1u < nranks && code >= knn_shard_first_cell(r + 1u, ncells, nranks, gran))
        ++r;
    return r;
}
struct ShardGeom {
    int k = 0, bits = 0, sa = 0, nranks = 1;
    int seed_tiles = 2;              // tiles of every cell each rank replicates (the seed layer)
    unsigned char nb[16] = {0}, shift[16] = {0};
    unsigned ncells = 0;             // 2^bits, all ranks together
    unsigned cells_per_rank = 0;     // the LARGEST rank's cells (a part of the seed layer has room for that many)
    long long n_global = 0;
    float bounds[16 * 15];           // ascending cuts of every dimension (+INF beyond a dimension's bins)
    float center[16];
    float sigma = 1.0f;
    unsigned first_cell(int rank) const { return knn_shard_first_cell((unsigned)rank, ncells, (unsigned)nranks, 1u << sa); }
    unsigned cells_of(int rank) const { return first_cell(rank + 1) - first_cell(rank); }
    // bytes of ONE rank's part of the seed layer: header (bmax, nmax) | [cpr][T][64] fragments | [cpr][T][32] split norms
    size_t part_bytes() const { return KNN_SEED_HEADER_BYTES + (size_t)cells_per_rank * (size_t)seed_tiles * (1024u + 128u); }
};

// Cell-sorted layout of the references (k <= 16): see the head of knn_cells.hip.
struct CellIndex {
    int bits = 0, sa = 0;            // cells = 2^bits; low pruning table = 2^sa entries
    int lbits = 0;                   // bits of a local cell number (= bits unless the index is a cell-range shard)
    unsigned char nb[16] = {0}, shift[16] = {0};
    unsigned ncells = 0, cap = 0;    // cap: queries a cell's list can hold per batch
    float *bounds = nullptr;         // device [16][15]: ascending cuts of every dimension
    unsigned *tile_start = nullptr;  // device [ncells + 1]: first 32-row tile of each cell in the layout
    unsigned *perm = nullptr;        // device [ntiles * 32]: row held by each layout position (~0u = padding)
    unsigned max_cell_rows = 0;
    // what the scan's waves take one at a time: (cell << 48) | (tiles << 40) | first tile — a run of at most
    // KNN_CELL_ITEM_TILES tiles of ONE cell.  Cells without rows have no item; a cell of many rows (clustered data the
    // quantile cuts do not spread) has several, all scored against the same list
    unsigned long long *items = nullptr;
    unsigned nitems = 0;
    // build only (freed once the rows are placed): the shard's rows grouped by the top 8 bits of their cell code — 256
    // buckets of consecutive cells — as 64-byte records + (code << 32 | row); null: the one-pass placement is used
    float *tmp_rows = nullptr;
    unsigned long long *tmp_meta = nullptr;
    unsigned *bucket_start = nullptr;   // device [257]: first record of each bucket
    // the FAST build (round 5; CellBuild::Fast): buckets of fixed room, filled to bucket_fill[b]; the cells' tile
    // ranges and the items come from a device prefix — build_res = {tiles, items, rows of the largest cell, bucket overflow}
    // is read by the caller together with the placement's statistics, ONE synchronisation for the whole build
    float h_bounds[16 * 15];            // (host sources of the fast build's asynchronous copies: they must outlive the call)
    unsigned h_bucket_start[257];
    unsigned bucket_cap = 0;            // records a bucket has room for
    unsigned *bucket_fill = nullptr;    // device [256] (inside the block `bucket_start` points to)
    unsigned *build_res = nullptr;      // device [4]   (likewise)
    // cell-range shards (knn_index_create_sharded): global number of every local row, ascending (borrowed); null: base + row
    const unsigned *gids = nullptr;
    // cell-range shards: `bits`, `nb`, `shift`, `sa`, `bounds` are the GLOBAL grid's; this index holds cells
    // [cell_base, cell_base + ncells) of it under local numbers 0 .. ncells - 1 (cell_base is a multiple of 2^sa)
    unsigned cell_base = 0;
    const ShardGeom *geom = nullptr;      // (borrowed: outlives the index)
    const unsigned char *seed_layer = nullptr;   // device: every rank's part, nranks x geom->part_bytes() (borrowed)
    // per-cell frames (round 5, clustered data; knn_cells_recentre): the fragments of cell c are fp16((row - centre_c) x scale_c)
    // instead of the shard's one frame — cell_frame[c] = { centre[16] (the rows' own units), scale_c = sigma 2^e, 2^e,
    // max |fragment coordinate| of the cell, max fragment norm of the cell }; tile_cell[t] = the cell tile t belongs to
    bool centred = false;
    float *cell_frame = nullptr;          // device [ncells][KNN_CELL_FRAME_WORDS]
    unsigned *tile_cell = nullptr;        // device [ntiles]
    // 8-bit rows (option `cells_rows`; needs per-cell frames): the scan reads these instead of the fp16 fragments and their
    // norms — rows8 u8 [tile][64 lanes][8], byte j of a lane = 128 + round(128 v) of the lane's K-slot j, v the row in its
    // cell's frame, so the row the scan scores is (code - 128) / 128; norms8 fp32 [tiles * 32] = that row's squared norm
    // (+INF on padding rows and rows outside the robust box); cell_u8[c] = { max over the cell's coordinates of
    // knn_u8_code's err, max norms8 of the cell }.  The fp16 fragments stay: the prep kernel's seeds.
    bool rows_u8 = false;
    unsigned char *rows8 = nullptr;       // device [ntiles][64][8]
    float *norms8 = nullptr;              // device [ntiles * 32]
    float *cell_u8 = nullptr;             // device [ncells][2] (bin frames: [2], the shard's largest err and N'')
    // 8-bit rows in per-dimension bin frames (option `cells_u8_frame`, knn_filter_dev.h knn_u8_bin_code): the layout stays in the
    // shard's one frame (centred = false: the fp16 fragments are the prep kernel's, untouched); rows8 hold the rows' offsets
    // from their cell's w_c at scale sigma 2^e, norms8 = N'' = |w_c + r^|^2; binw fp16 [ncells][16] = w_c (0 beyond k)
    bool bins = false;
    void *binw = nullptr;                 // device [ncells][16] fp16
    float bin_ratio = 1.0f, bin_er = 0.0f, bin_nmax = 0.0f, bin_w1 = 0.0f;
};
#define KNN_CELL_FRAME_WORDS 20
#define KNN_NIF_MAX_K 30   // 16 < k <= 30: the cell-sorted fragments carry the rows' norms in K-slots 30, 31 (knn_cells.hip: cell_tile_step_nif)

// The options of one filter query, filled from the global options by knn_index_query / knn_index_query_topk and passed by value:
// nothing of a call stays in the index.  (Whether the call is pruned is not an option here: knn_query_route decides it.)
struct FilterCallOptions {
    // the dense scan (knn_filter_query_plan)
    int force_qt = 0;          // "filter_qt": query tiles per wave of the register scan at k <= 16 (0 = pick by m)
    int force_rounds = 0;      // "filter_rounds": blocks per resident slot of the register scan (k <= 32; k 33 .. 128 below 16
                               // query tiles); 0 = one
    int chain_policy = 0;      // "filter_chain": scans of different slots (k <= 512; k > 512 never chains): 0 auto (chained from
                               // 2^19 tiles), 1 always chained, 2 never
    int run_thresholds = 0;    // LDS-tiled scan at k 65 .. 512 (at k <= 128 from 16 query tiles): 0 / 1 thresholds tighten during
                               // the launch and the sample pass thins out, 2 they stay as the sample pass left them
    int sample_stride = 0;     // LDS-tiled scan (k 33 .. 512; at k <= 128 from 16 query tiles): tiles the sample pass skips between
                               // two it scores; 0 = library policy
    int topk = 0;              // K of a top-K call (the threshold comes from the K-th smallest per-block sample minimum); 0 = 1-NN
    // the cell-pruned scan (knn_cells_query_plan)
    bool several_slots = false;// the index's recent calls named more than one workspace slot: batches are in flight side by side
    int scan_blocks = 0;       // blocks per CU: 0 auto (one for small shards when several_slots, else two), 1, 2
    int scan_deal = 0;         // 0 auto (block counter unless several_slots), 1 fixed deal, 2 items from a block counter
    int cells_lists = 0;       // who lists a cell's queries: 0 auto, 1 knn_cells_match_kernel, 2 the scan's own waves
};

struct FilterState {
    bool usable = false;       // references finite and in a sane range: filter layouts exist
    int k = 0, kt = 0;         // real dimension; 16-wide K steps (padded k = 16 * kt)
    long long n = 0;           // references in the shard
    long long ntiles = 0;      // ceil(n / 32)
    float sigma = 1.0f;        // power-of-two scale
    float bmax = 0.0f;         // max |scaled fp16 reference coordinate|
    float nmax = 0.0f;         // max fp32 squared norm of the fp16 reference rows
    float *center = nullptr;   // device [16*kt]
    void *ref_frags = nullptr; // device [ntiles][kt][64] x 16 B: A operands in MFMA lane order
    float *ref_norms = nullptr;// device [ntiles*32] (+INF for padding rows)
    unsigned *ref_norms2 = nullptr; // cell-sorted layouts only, device [ntiles*32]: the same norms as two fp16 halves
                               // (hi | mid * 2^11 << 16) — the prep kernel rebuilds the C tile of its seed scores from
                               // them with one extra MFMA: one register per tile in flight instead of 16 (knn_cells.hip)
    unsigned *outliers = nullptr; // device: rows outside the robust box (excluded from the filter, scanned exactly)
    unsigned n_outliers = 0;
    CellIndex *cells = nullptr;   // non-null: the layout is cell-sorted (ntiles counts its padded tiles)
    FilterWorkspace ws[KNN_SLOTS];
    // The slots' big scan kernels are chained through this event: two of them sharing the CUs run
    // 15 % slower than back to back; only the small preparation kernels are meant to overlap.
    hipEvent_t scan_done = nullptr;
    bool scan_recorded = false;
};

// ---- cell-pruned form of the filter (knn_cells.hip) -----------------------------------------
#define KNN_CELLS_AUTO_MAX_K 25   // library policy: cell-sorted layouts for resident indexes up to this dimension (`cells` = 1: up to 32)
#define KNN_CELL_BATCH 1024   // queries per pass: their B operands + thresholds sit in 36 KiB of LDS (68 KiB for 16 < k <= 32)
#ifdef __cplusplus
#include <vector>
// The build of a cell-sorted layout (knn_cells.hip, "the build"): plan, strategy, staging; the finish is knn_filter.hip's.
enum class CellBuild { Fast, Counted, OnePass, None };   // None: no cell-sorted layout from this build
// Where the build's frame and rows come from: the strided sample of resident rows (and cell-range shards), the full-range
// statistics of resident rows (after the sampled frame was declined), or host rows that an ingest is still copying.
enum class CellRows { Sample, FullRange, Host };
bool knn_cells_plan(CellIndex &plan, int k, long long n, const float *samp, long long samples, const ShardGeom *geom, int rank);
CellBuild knn_cells_first_build(const CellIndex &plan, int k, long long n, int cells_build, CellRows rows);
CellBuild knn_cells_next_build(CellBuild how, CellRows rows);
// A staged layout: what the placement (knn_cells_place_rows) needs besides the CellIndex.
struct CellStaging {
    CellIndex *c = nullptr;      // null: the shard does not suit the cells
    long long ntiles = 0;        // the layout's tiles (the fast build: room for them — its build_res holds the count)
    unsigned *code = nullptr;    // device [n]: every row's cell (counted build, one-pass placement)
    unsigned *fill = nullptr;    // device [ncells]: the placement's fill counters, zeroed
    void release();              // frees the build scratch (code, fill, the CellIndex's buckets); the layout stays
};
void knn_cells_release_build_scratch(CellIndex &c);
// rows = CellRows::Host: the scatter is left to the ingest (knn_cells_fast_scatter).  *bad_rows_out: see cells_stage_counted.
hipError_t knn_cells_stage(CellStaging &stg, const CellIndex &plan, CellBuild how, CellRows rows, int k, long long n, const float *r_dev,
                           hipStream_t s, unsigned *bad_rows_out = nullptr);
// The fast build in stages (knn_cells_stage for CellRows::Host: everything allocated and uploaded, nothing scattered yet).
hipError_t knn_cells_fast_scatter(CellIndex &c, int k, const float *r_dev, long long row0, long long row1, hipStream_t s);
hipError_t knn_cells_fast_finish(CellIndex &c, unsigned *counts, hipStream_t s);
#endif
// The two tests of knn_cells_match_kernel, fp32 with one rounding each.  knn_cell_listed: query q stays on cell (h, l)'s list —
// its lower bound lo[q][l] + hi[h][q] is not above Dup_q.  knn_cell_queued: q enters the queue of a block of 64 cells, lo_min the
// smallest of the block's 64 low entries as stored.  fl(a + b) does not decrease when b grows, so the smallest entry gives the
// smallest of the 64 sums: queued <=> listed for at least one cell of the block (tests/test_match_prefilter_logic.py).
__host__ __device__ static inline bool knn_cell_listed(float lo, float hi, float dup)
{
    return !(lo + hi > dup);
}
__host__ __device__ static inline bool knn_cell_queued(float lo_min, float hi, float dup)
{
    return knn_cell_listed(lo_min, hi, dup);
}

// Sizes of one scan launch of the cell-pruned path (knn_cells.hip; host arithmetic only).
struct CellScanPlan {
    unsigned blocks = 0, waves = 0, nlists = 0, slice = 0, ovf_base = 0, ovf_cap = 0;
    size_t lds_bytes = 0;
};
CellScanPlan knn_cells_scan_plan(int num_cu, int blocks_per_cu, unsigned nitems, unsigned rec_cap, int m_padded,
                                 bool self_lists = false, int kt = 1, bool centred = false);
bool knn_cells_lists_policy(unsigned ncells, bool several_slots);
// Every choice and size one batch of the cell-pruned query launches with (knn_cells_query_plan; host arithmetic only).
struct CellQueryInputs {
    int k = 0, kt = 1;
    bool centred = false, rows_u8 = false;      // per-cell frames; 8-bit rows (in bin frames when not centred)
    unsigned ncells = 0, nitems = 0, cap = 0;   // the index's cells, work items and room per list of queries
    bool several_slots = false;
    int scan_blocks = 0, scan_deal = 0, cells_lists = 0;   // the options (FilterCallOptions)
    int m = 0, num_cu = 0;
    unsigned rec_cap = 0;
};
struct CellScanForm {   // knn_cells_scan_kernel<dyn, k, self, kt, ctr, nif, u8>; u8: it reads the 8-bit rows
    bool dyn = false;
    int k = 0;
    bool self = false;
    int kt = 1;
    bool ctr = false, nif = false, u8 = false;
};
struct CellQueryPlan {
    int prep_pw = 4, prep_kt = 1;   // knn_cells_prep_kernel<pw, 2, kt, ctr>
    bool prep_ctr = false;
    bool self_lists = false;        // the scan's waves list their own items: no match launch
    int match_waves = 0;            // knn_cells_match_kernel<16> or <8>; 0 with self_lists
    unsigned stage = 0;             // entries of a list the match kernel assembles in LDS
    size_t match_lds = 0;
    CellScanForm scan;
    CellScanPlan grid;              // the scan's grid, record lists and LDS
    unsigned list_cap = 0;
    int tail_k = 0, tail_kt = 1;    // knn_cells_tail_kernel<k, kt>
    unsigned tail_blocks = 0;
    bool exact_launch = false;      // the gated exact scan of the shard is a launch of its own (k != 16)
    size_t scan_lds_limit = 0, match_lds_limit = 0;   // the variants' dynamic-LDS attribute (0: the default)
};
CellQueryPlan knn_cells_query_plan(const CellQueryInputs &in);
// Top-K on the cell-pruned scan (knn_cells_topk_plan; host arithmetic only): whether a call takes it, and every choice and size
// of one of its passes.  DESIGN §4.6.
struct CellTopkInputs {
    CellQueryInputs q;             // the index and the options as for a 1-NN batch; q.m = the CALL's queries (passes of KNN_CELL_BATCH)
    int K = 1;
    long long n = 0;               // rows of the shard
    int topk_cells = 0;            // option: 0 policy, 1 wherever the layout allows it, 2 never
    int cells_option = 0;          // option `cells` (2: the caller asked for full scans)
    bool has_cells = false;        // a cell-sorted layout exists
    bool bins = false;             // its 8-bit rows are in per-dimension bin frames (with q.rows_u8)
    bool sharded = false;          // cell-range shard
    bool shard_partial = false;    // ... whose call carries KNN_QUERY_TOPK_PARTIAL (the only top-K a cell-range shard prunes)
    bool other_path = false;       // the grid index or a forced exact path answers this index
    bool frames_flag = false;      // the call carries KNN_QUERY_TOPK_FRAMES (the only top-K a layout in per-cell frames prunes)
    unsigned n_outliers = 0;
    unsigned ccap = 0;             // knn_topk_ccap(K, q.m), from the caller (knn_query_route)
};
struct CellTopkPlan {
    bool use = false;              // false: the call stays on the path it had (filter top-K or exact top-K)
    int passes = 0, pass_m = 0;    // passes of <= KNN_CELL_BATCH queries; the first pass's queries
    CellQueryPlan batch;           // prep_pw / prep_kt, the match launch, the scan's grid and record lists, list_cap, LDS limits
    CellScanForm scan;             // knn_cells_records_kernel<dyn, kt, nif, u8> (self: never); ctr: knn_cells_frame_records_kernel<dyn, u8>
    unsigned ccap = 0;             // candidate keys a query has room for
    // (the launches behind the scan are knn_cells_query_topk's fixed sequence: nothing of them is a choice)
};
// rows from which the library builds a cell-sorted layout by policy (1-NN: the pruned scan wins from there; knn_api.cpp)
static inline long long knn_cells_size_rule(int k)
{
    return k <= 12 ? (1ll << 19) : k <= 16 ? (1ll << 20) : k <= 21 ? (1ll << 22) : k <= 23 ? (1ll << 23)
         : k <= KNN_CELLS_AUTO_MAX_K ? (1ll << 24) : (1ll << 62);
}
// candidate keys a query of a top-K call of m queries has room for (the filter top-K's and the cell-pruned top-K's lists)
static inline unsigned knn_topk_ccap(int K, int m)
{
    return (unsigned)std::min<long long>(4096 + 128 * (long long)K, ((long long)32 << 20) / m);
}
CellTopkPlan knn_cells_topk_plan(const CellTopkInputs &in);
// the passes of a count call on the cell-pruned way: knn_cells_topk_plan at K = 1 on a one-frame layout (in: the call's route inputs)
CellTopkPlan knn_cells_count_plan(const CellTopkInputs &in);

// ---- which path answers a call, and what an index is built with (knn_api.cpp; host arithmetic only) ---------------------------
// knn_query_route is the ONE place a call's path is chosen (DESIGN, "which path answers a call"): nothing is allocated or
// launched, no global is read — the options are inputs.  tests/test_route_logic.py restates the rules on the CPU through
// knn_debug_query_route.
enum class QueryWay { Exact = 1, Filter = 2, Grid = 3, Cells = 4 };   // the values are knn_index_last_stats' [0]
struct QueryRouteInputs {
    // the index, the call and the options `cells` (t.cells_option), `topk_cells` and the scan's, as the cell-pruned top-K's plan
    // takes them: t.q.m = the call's queries, t.K = K (0: a 1-NN call), t.n > 0 (an empty shard is answered before any route),
    // t.has_cells = filter layouts exist AND are cell-sorted.  t.other_path and t.ccap are the route's to fill.
    // Invariant: a cell-range shard (t.sharded) has no grid index — knn_index_create_sharded never builds one.
    CellTopkInputs t;
    bool filter_usable = false;    // the index has filter layouts
    bool has_grid = false;         // ... a grid index (k <= 4)
    bool filter_wanted = false;    // its creator asked for the layouts below the size the library builds them from
    bool init_keys = false;        // KNN_QUERY_INIT_KEYS
    int path = 0;                  // option `path`
    bool topk_grid = false;        // KNN_QUERY_TOPK_GRID: the grid index may answer this top-K call
};
struct QueryRoute {
    QueryWay way = QueryWay::Exact;
    bool fill_keys_first = false;  // 1-NN: the keys are set to (+INF, 0) by a launch of their own ahead of the path's
    unsigned ccap = 0;             // top-K: candidate keys per query (the filter's lists and the pruned scan's)
    CellTopkPlan topk;             // top-K: knn_cells_topk_plan's answer (use == (way == Cells))
};
QueryRoute knn_query_route(const QueryRouteInputs &in);
// What a count call launches with (knn_count_route in knn_api.cpp: the ONE place its way is chosen; host arithmetic only,
// knn_debug_count_plan).  The default is the exact count scan; the grid and the cell-pruned scan answer on request by flag.
struct CountRouteInputs {
    int k = 0, m = 0;
    long long n = 0;               // rows of the shard (> 0)
    bool radius_finite = false;
    bool flag_grid = false, flag_cells = false;   // KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS
    bool has_grid = false;         // the index has a grid index
    bool has_cells = false;        // ... a cell-sorted layout
    bool centred = false, rows_u8 = false, bins = false, sharded = false;   // as CellTopkInputs
    int path = 0, cells_option = 0;
    int num_cu = 0;
    long long radius_rings = 0;    // the rings the radius spans on the grid (knn_grid_radius_rings)
};
struct CountPlan {
    QueryWay way = QueryWay::Exact;
    int passes = 0, pass_m = 0;    // Cells: passes of <= KNN_CELL_BATCH queries; the first pass's queries
    int rmax = 0;                  // Grid: rings a query walks before it gives up (knn_grid_topk_plan's rule at K = 1)
    unsigned blocks = 0;
    int waves = 0;                 // Grid: the kernel's blocks, waves per block (one query each)
    long long slices = 0;          // slices of the exact count scan for the call's first chunk of queries
    size_t scratch_bytes = 0;      // the slot's count scratch: [m] unsigned on the grid and cell ways, none on the exact way
};
CountPlan knn_count_route(const CountRouteInputs &in);
// What a slot's three top-K buffers must hold for a call (host arithmetic only; knn_debug_topk_scratch): `part` the exact top-K
// scan's per-slice lists — on the cell-pruned way also at a pass's and at the last pass's queries, whose gated exact top-K sizes
// its lists by them —, `cand` the filter ways' candidate lists [m][knn_topk_ccap] + counters [m] or a folding grid call's lists,
// `lists` the unclipped lists [m][K] of a radius call on the ways that clip behind.
struct TopkScratchInputs {
    QueryWay way = QueryWay::Exact;
    int m = 0, K = 0;
    long long n = 0;
    int num_cu = 0;
    bool init = false, within = false;
    int pass_m = 0;                // QueryWay::Cells: CellTopkPlan::pass_m
    size_t grid_scratch_bytes = 0; // QueryWay::Grid: GridTopkPlan::scratch_bytes
};
struct TopkScratchPlan {
    size_t part_bytes = 0, cand_bytes = 0, lists_bytes = 0;
};
TopkScratchPlan knn_topk_scratch_plan(const TopkScratchInputs &in);

// What index_create_impl builds, decided up front.  What only the run can tell stays there: no streams for an ingest, a grid
// build that rules the grid out, a cell sort under the copy that reports unusable, no memory for the layouts.
enum class IngestForm { CopyThenBuild = 0, LayoutsUnderCopy = 1, CellsUnderCopy = 2 };
struct IndexBuildInputs {
    int k = 0;
    long long n_local = 0;
    bool refs_on_device = false;
    int build_filter = -1;         // 1 the MFMA filter layouts, 2 cell-sorted, 0 none, -1 library policy
    int build_grid = -1;           // (k <= 4) 1 the grid index, 0 none, -1 library policy
    int path = 0, cells = 0, ingest = 0, cells_build = 0;   // the options
};
struct IndexBuildPlan {
    bool filter_wanted = false;    // knn_index::filter_wanted
    bool want_cells = false;       // the layouts are cell-sorted
    int build_filter = 0;          // resolved: never -1
    bool grid_planned = false;     // the grid index is tried first (a shard it serves gets no MFMA layouts)
    bool want_layouts = false;
    IngestForm ingest = IngestForm::CopyThenBuild;   // host rows: how they reach the device
};
IndexBuildPlan knn_index_build_plan(const IndexBuildInputs &in);
// Every choice and size one batch of the dense filter query launches with (knn_filter_query_plan in knn_filter.hip; host
// arithmetic only).  The scan comes in three forms: pieces of the batch on the register scan (knn_filter_kernel, k <= 32, and
// k <= 128 below 16 query tiles), the LDS-tiled scan (knn_filter_tiled_kernel, k <= 512) and the chunked-K scan
// (knn_filter_chunked_kernel, k > 512).
struct FilterQueryInputs {
    int kt = 1;                // the index's K-steps (knn_kt_of)
    long long ntiles = 0;
    int m = 0, num_cu = 0;
    unsigned rec_cap = 0;      // records a workspace holds
    FilterCallOptions opt;     // (its topk: K, 0 = 1-NN)
};
enum class FilterForm { Pieces, Tiled, Chunked };
struct FilterPiece {           // query tiles [begin, begin + count), scanned by one launch whose waves keep qt tiles
    int qt = 0, begin = 0, count = 0;
    unsigned gx = 0, gy = 0;   // the scan's grid (the chunked form: ranges x query groups, launched as one dimension)
    unsigned list_base = 0;    // its first record list
};
struct FilterQueryPlan {
    bool ok = false;           // false: nothing to launch with (no record lists, too many, kt not a multiple of CHK_KC)
    FilterForm form = FilterForm::Pieces;
    int kt = 1;                // KT of the form (the chunked form: the run-time kt)
    int npieces = 0;           // the pieces form: up to four; the others: one, the whole batch
    FilterPiece pieces[4];
    unsigned nlists = 0, slice = 0;
    long long stride = 1;      // the sample pass scores every stride-th tile
    unsigned sample_blocks = 0;// the sample grid's x (its y: the piece's gy)
    size_t umin_floats = 0;    // per-block minima the sample pass writes
    int topk = 0;              // > 0: the K-th smallest per-block minimum (knn_topk_umin_kernel) feeds the thresholds
    int thr_nb = 0;            // sample rows knn_thr_kernel folds
    bool thr_running = false;  // knn_thr_kernel also writes margins, floors and running thresholds
    bool scan_running = false; // the scan is handed the running thresholds
    bool in_chain = false;     // the scan takes part in the slots' chain (FilterState::scan_done)
    bool chained = false;      // ... and waits on the last recorded scan and records its own
    bool has_rows = false;     // the scan writes a row mask next to every record
    RerankPieces rerank;
};
FilterQueryPlan knn_filter_query_plan(const FilterQueryInputs &in);
hipError_t knn_cells_place_rows(FilterState &st, const float *r_dev, const unsigned *code, unsigned *fill, unsigned *out,
                                unsigned ocap, hipStream_t s);
void knn_cells_free(CellIndex *&c);
// rows_u8: also the 8-bit rows; frames_wanted: per-cell frames are wanted on their own (else, without room for the 8-bit rows,
// the layout stays in the shard's one frame)
hipError_t knn_cells_recentre(FilterState &st, const float *r, hipStream_t s, bool rows_u8 = false, bool frames_wanted = true);
bool knn_cells_sample_is_clustered(const float *samp, long long samples, int k, float sigma);
bool knn_cells_sample_is_uniform_like(const float *samp, long long samples, int k);
hipError_t knn_cells_maybe_recentre(FilterState &st, const float *r, const float *samp, long long samples, hipStream_t s);
extern std::atomic<int> g_knn_cells_centre;
extern std::atomic<long long> g_knn_cells_centred_builds;
extern std::atomic<int> g_knn_cells_rows;
extern std::atomic<long long> g_knn_cells_u8_builds;
extern std::atomic<int> g_knn_cells_u8_frame;
extern std::atomic<long long> g_knn_cells_u8_bin_builds;
void knn_cells_workspace_free(FilterWorkspace &w);
// One batch of <= KNN_CELL_BATCH queries already prepared by the filter's query-fragment kernel: seed, thresholds,
// match, scan (records in w, as the full scan leaves them).  Asynchronous.
// init_keys: the batch's keys are set to (+INF, 0) by the first kernel of the chain.
hipError_t knn_cells_query(FilterState &st, FilterWorkspace &w, FilterCallOptions opt, int m, const float *q_dev, const float *r_dev,
                           long long base, u64 *keys, int num_cu, bool timed, hipStream_t s, bool init_keys, int *out_idx = nullptr);
// One pass of <= KNN_CELL_BATCH queries of a top-K call (c: TopkCall::pass): prep (K-th seed bound) -> match -> record-only scan
// -> re-rank of the slices and of the shared overflow area -> out-of-box rows -> select -> the exact top-K, gated on FALLBACK and
// without the limit.  c.max_dist2 finite (a radius call, one-frame layouts): the prep kernel caps Dup_q with the radius
// (knn_threshold_within).  timed: the pass records the call's events around its scan.
hipError_t knn_cells_query_topk(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const TopkCall &c);
// One pass of <= KNN_CELL_BATCH queries of a count call (c: CountCall::pass; c.max_dist2 finite, one-frame layouts): count prep
// (the radius cap alone) -> match -> record-only scan -> count re-rank -> out-of-box rows -> commit (no FALLBACK) -> the exact
// count, gated on FALLBACK.  tp: knn_cells_count_plan's pass shapes.
hipError_t knn_cells_query_count(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const CountCall &c);
// One pass of a list call (c: ListCall::pass): the count pass up to its finish, then the list re-rank and out-of-box rows (they
// reserve in c.scratch, a copy of c.fill, and store behind it) -> commit (no FALLBACK) -> the exact list, gated on FALLBACK, from
// the untouched c.fill over the same places.
hipError_t knn_cells_query_list(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const ListCall &c);

// Builds the filter layouts for refs[0..n) (device, AoS).  Synchronous.  Leaves st.usable false
// (and returns hipSuccess) when the data rules the filter out.
// pooled device memory for the CURRENT device (knn_api.cpp); knn_dev_free waits for the device first
hipError_t knn_dev_alloc(void **p, size_t bytes);
hipError_t knn_dev_free(void *p);
// bracket a run of knn_dev_free calls on this thread with ONE device-wide wait (current device)
void knn_dev_free_begin_synced();
void knn_dev_free_end_synced();

// ---- uniform-grid index for k <= 4 (knn_grid.hip) -------------------------------------------
struct GridState;
// *out stays null (hipSuccess) when the data rules the grid out.  Synchronous.
hipError_t knn_grid_build(GridState **out, int k, long long n, const float *r_dev, hipStream_t stream);
void knn_grid_free(GridState *&gs);
// Asynchronous; *gate_out = device word that is != 0 afterwards iff some query left the grid search
// unfinished (the caller queues the gated brute-force scan behind it).
hipError_t knn_grid_query(const GridState *gs, int slot, int m, const float *q_dev, long long base, u64 *keys_dev,
                          const unsigned **gate_out, hipStream_t stream);
// Top-K on the grid index (KNN_QUERY_TOPK_GRID; knn_grid_topk_kernel): what a call launches with.  Host arithmetic only.
struct GridTopkPlan {
    bool use = false;          // the grid answers the call (everything below is 0 otherwise)
    int rmax = 0;              // rings a query walks before it gives up
    unsigned blocks = 0;
    int waves = 0;             // per block: one query each
    size_t scratch_bytes = 0;  // a folding call's lists [m][K] (the slot's cand buffer: knn_topk_scratch_plan)
    int launches = 0;          // of a folding call: grid kernel, gated exact top-K (scan + select per chunk), fold
};
// radius_rings (knn_index_query_topk_within): the rings the radius spans (knn_grid_radius_rings); 0 = a plain call.
GridTopkPlan knn_grid_topk_plan(int k, int K, int m, bool has_grid, int path, bool flag, long long radius_rings = 0);
// The rings a radius of max_dist2 (squared, >= 0) spans on the grid: ceil(radius / the narrowest live axis' cell width) + 1,
// capped at 2^30; a degenerate axis (one cell) is ignored, 0 when every axis is.  Sizes the plan's rmax only.
long long knn_grid_radius_rings(const GridState *gs, float max_dist2);
// c.init 0: the kernel's lists go to c.cand (>= plan.scratch_bytes) and are merged into c.keys.  A radius call (c.within()):
// only rows with v0 distance <= c.max_dist2 are candidates, in the grid kernel and in the gated exact top-K behind it; a query
// stops as soon as the face bound passes the radius.
hipError_t knn_grid_query_topk(const GridState *gs, const GridTopkPlan &plan, int slot, const TopkCall &c, const unsigned **gate_out);
// Counts on the grid index (KNN_QUERY_COUNT_GRID; knn_grid_count_kernel): c.scratch [m] receives the kernel's counts, the commit
// (no give-up) or the gated exact count (give-up) adds the batch to c.counts.  rmax: CountPlan::rmax.
hipError_t knn_grid_query_count(const GridState *gs, int rmax, int slot, const CountCall &c, const unsigned **gate_out);
// Lists on the grid index (KNN_QUERY_COUNT_GRID; knn_grid_list_kernel): c.scratch [m] starts as a copy of c.fill, the walk reserves
// in it and stores the keys behind it; the commit (no give-up) copies it to c.fill, or the gated exact list (give-up) answers the
// batch from the untouched c.fill over the same places.
hipError_t knn_grid_query_list(const GridState *gs, int rmax, int slot, const ListCall &c, const unsigned **gate_out);
void knn_grid_info(const GridState *gs, long long info[4]);

// ---- clusters of the radius graph (knn_cluster.hip, knn_grid.hip; DESIGN §4.6 "Clusters of the radius graph") -------------------
// One knn_index_self_cluster_within call behind its degree step, as the launches below take it.  parent is the caller's labels
// array: the degrees on entry to knn_cluster_core_launch, the union-find forest (parent[i] = a core row <= i of i's set, -1 for a
// row that is not core) from there to knn_cluster_flatten_launch, the labels behind it.
struct ClusterCall {
    int k = 0;
    long long n = 0;               // the shard's rows, <= INT_MAX
    const float *r = nullptr;      // device [n][k]
    float max_dist2 = INFINITY;    // the radius, squared (>= 0, never -0; +INF: every row with a finite distance)
    int min_pts = 1;
    int num_cu = 0;
    hipStream_t stream = nullptr;
    int *parent = nullptr;         // device [n]
    unsigned *core = nullptr;      // device [(n + 31) / 32]: bit i % 32 of word i / 32 = row i is core (the caller's core_dev or slot scratch)
    u64 *best = nullptr;           // device [n], slot scratch: the smallest key (distance bits, row) of a core row within the radius
};
// Everything a call launches and the slot scratch it needs (host arithmetic only; knn_debug_cluster_plan shows it).
struct ClusterPlan {
    int chunks = 0;                  // launches of the exact link sweep: chunks of <= KNN_TOPK_CHUNK rows
    long long slices = 0;            // blocks along the shard's rows of the first chunk's sweep (knn_count_slices)
    long long launches_exact = 0;    // kernel launches of the whole call on the exact way: degrees, core, links, flatten
    long long launches_grid = 0;     // ... on the grid way: + the grid kernels, the count's commit, the gated exact twins
    size_t scratch_bytes = 0;        // best [n] u64 + the core mask words when the caller passes no core_dev
    size_t count_bytes = 0;          // the grid way's count scratch [n] unsigned (the routed self count's own)
};
ClusterPlan knn_cluster_plan(long long n, int num_cu, bool own_mask);
// parent[i] (holding deg(i)) <- i when deg(i) + 1 >= c.min_pts, else -1; c.core <- the core bits, the words' bits at and beyond
// n zero; c.best[i] <- KNN_KEY_INIT.
hipError_t knn_cluster_core_launch(const ClusterCall &c);
// The link sweep on the exact way: for every pair of core rows i < j within the radius unite(i, j); for every row j that is not
// core, c.best[j] <- the smallest key of a core row within the radius.  gate != nullptr: the launches do nothing unless
// *gate != 0 (behind the grid sweep: its give-up word).
hipError_t knn_cluster_link_launch(const ClusterCall &c, const unsigned *gate);
// The same sweep on the grid (knn_grid.hip): one wave per row walks its rings; *gate_out = the batch's give-up word, on which the
// caller gates knn_cluster_link_launch behind it.  rmax: CountPlan::rmax at the call's radius.
hipError_t knn_grid_cluster_link(const GridState *gs, int rmax, int slot, const ClusterCall &c, const unsigned **gate_out);
// parent -> labels: a core row's root, a border row's (c.best[i] holds a key) nearest core row's root, -1 for every other row.
hipError_t knn_cluster_flatten_launch(const ClusterCall &c);
// The link sweep on the cell-pruned way (include/knn_mi355x.h 2n; knn_cluster_routed.hip): one pass of <= KNN_CELL_BATCH own rows.
struct ClusterPass {
    ClusterCall c;
    long long first = 0;   // the pass's first own row
    int m = 0;             // its rows
};
// The exact sweep of the window of own rows first .. first + m - 1 against all c.n rows, gated (gate != nullptr): what
// knn_cluster_link_launch does for the shard's rows, for a pass's.
hipError_t knn_cluster_link_window_launch(const ClusterCall &c, long long first, int m, const unsigned *gate);
// A pass behind its record-only scan: the link re-rank of the slices and of the shared overflow area, the out-of-box rows; no commit.
hipError_t knn_cluster_link_records_finish(const ClusterPass &p, const TopkRecords &rs);
// One pass: the count pass's front unchanged (Q = R + first * k) -> knn_cluster_link_records_finish -> the gated exact twin on the
// pass's window.  tp: knn_cells_count_plan's pass shapes.
hipError_t knn_cells_cluster_link(FilterState &st, FilterWorkspace &w, const CellTopkPlan &tp, bool timed, const ClusterPass &p);
// The link sweep of the whole shard in passes of KNN_CELL_BATCH own rows (knn_cells_cluster_link).
hipError_t knn_filter_cluster_link_cells(FilterState &st, const CellTopkPlan &tp, int slot, const ClusterCall &c);

// ---- minimum spanning forest of the radius graph (knn_forest.hip, knn_forest_pick.h, knn_grid.hip; DESIGN §4.6 "Minimum spanning
// forest") ------------------------------------------------------------------------------------------------------------------------
// ROUNDS(n) = max(1, ceil(log2 n)): the unfinished components at least halve in every Borůvka round.
inline int knn_forest_rounds(long long n)
{
    int t = 0;
    while (t < 62 && (1ll << t) < n)
        ++t;
    return t < 1 ? 1 : t;
}
// One knn_index_self_forest_within call, as the launches below take it.  labels is the caller's array: the union-find forest
// (labels[i] = a row <= i of i's component) during the call, depth 1 — the answer — behind knn_forest_labels_launch.
struct ForestCall {
    int k = 0;
    long long n = 0;               // the shard's rows, 1 .. INT_MAX
    const float *r = nullptr;      // device [n][k]
    float max_dist2 = INFINITY;    // the radius, squared (>= 0, never -0; +INF: every pair with a finite distance)
    int num_cu = 0;
    hipStream_t stream = nullptr;
    int rounds = 0;                // knn_forest_rounds(n): all of them are queued
    int *labels = nullptr;         // device [n]
    u64 *edge_keys = nullptr;      // device [n]: E's bits << 32 | i
    unsigned *edge_hi = nullptr;   // device [n]: j
    unsigned *count = nullptr;     // device [2]: edges; rounds that added one
    // the slot's scratch (knn_forest_layout):
    u64 *cand = nullptr;           // [n] the round's candidate keys
    u64 *pick1 = nullptr;          // [n] a root's smallest (E's bits << 32 | lo)
    unsigned *pick2 = nullptr;     // [n] the smallest hi among the offers that match it
    unsigned *done = nullptr;      // [(n + 31) / 32] bit i: row i found no candidate in some round
    unsigned *words = nullptr;     // [2 * rounds + 2]: the gates of rounds 0 .. rounds, the rounds' give-up words, the statistics word
    // round t's kernels run when *gate(t) != 0; round t - 1's emit raises it (round 0: no gate)
    const unsigned *gate(int t) const { return t > 0 ? words + t : nullptr; }
    unsigned *raise(int t) const { return words + t + 1; }                   // what round t's emit raises
    unsigned *giveup(int t) const { return words + rounds + 1 + t; }         // round t's grid scan: some row passed rmax rings
    unsigned *stat() const { return words + 2 * rounds + 1; }               // the give-up word of the last round that ran
};
// Everything a call launches and the slot scratch it needs (host arithmetic only; knn_debug_forest_plan shows it).
struct ForestPlan {
    int rounds = 0;
    int chunks = 0;                  // launches of one round's exact scan: chunks of <= KNN_TOPK_CHUNK rows
    long long slices = 0;            // blocks along the shard's rows of the first chunk's scan (knn_count_slices)
    long long launches_exact = 0;    // kernel launches of the whole call on the exact way: per round flatten, the scan's chunks, two offers, emit, hook; the last flatten
    long long launches_grid = 0;     // ... on the grid way: per round the grid scan as well, the exact scan gated on its give-up word
    size_t cand_off = 0, pick1_off = 0, pick2_off = 0, done_off = 0, words_off = 0;
    size_t zero_bytes = 0;           // done bits and words: zeroed at the start of every call
    size_t scratch_bytes = 0;
};
ForestPlan knn_forest_plan(long long n, int num_cu);
void knn_forest_layout(ForestCall &c, const ForestPlan &p, void *scratch);
// count <- {0, 0}; the done bits and the words <- 0.  (Two memsets, no kernel.)
hipError_t knn_forest_begin_launch(const ForestCall &c, const ForestPlan &p);
// Round t's flatten: labels[i] <- i (t == 0) or root(i); cand, pick1, pick2 <- empty; the statistics word <- 0.
hipError_t knn_forest_flatten_launch(const ForestCall &c, int t);
// Round t's exact scan: cand[i] <- min(cand[i], the smallest key of a row of another component within the radius).  also: a
// second gate (the round's give-up word behind the grid scan), null on the exact way.
hipError_t knn_forest_scan_launch(const ForestCall &c, int t, const unsigned *also);
// Round t's scan on the grid (knn_grid.hip): one wave per row walks its rings.  rmax: CountPlan::rmax at the call's radius.
hipError_t knn_grid_forest_scan(const GridState *gs, int rmax, const ForestCall &c, int t);
// Round t's pick and hook: offer 1 (which also marks the rows without a candidate done), offer 2, emit, hook.
hipError_t knn_forest_pick_launch(const ForestCall &c, int t);
// Behind the last round: labels[i] <- root(i) when that round added an edge (else they are depth 1 already).  Labels alone.
hipError_t knn_forest_labels_launch(const ForestCall &c);

// ---- RCCL exchange step (knn_rccl.cpp; librccl is dlopen'ed at first use) -------------------
#ifdef __cplusplus
#include <string>
int knn_rccl_available(std::string *why);
int knn_rccl_version();
int knn_rccl_comm_sets();   // communicator sets this process has created (0 or 1)
int knn_rccl_allreduce_min(int ndev, const int *devices, u64 *const *keys, int m, const hipStream_t *streams,
                           std::string &err, u64 *const *recv = nullptr);
#endif

// want_cells: also sort the layout into cells (k <= 32, large shards; see CellIndex); cells_build: option `cells_build`.
// geom != null (cell-range shard `rank`): centre, scale and cuts are the global grid's; the layout is always cell-sorted.
hipError_t knn_filter_build(FilterState &st, int k, long long n, const float *r_dev, hipStream_t stream, bool want_cells = false,
                            int cells_build = 0, const ShardGeom *geom = nullptr, int rank = 0, unsigned *bad_rows_out = nullptr);
// The global grid of a cell-range sharded set from a sample of it (host rows, samples x k): false when the set does not suit
// (k > 16, too few rows per rank for a cell-sorted layout, a degenerate or non-finite sample).
bool knn_geom_cells(ShardGeom &g, int k, long long n_global, int nranks, const float *sample, long long samples, int seed_tiles);   // (the grid part of it)
bool knn_geom_from_sample(ShardGeom &g, int k, long long n_global, int nranks, const float *sample, long long samples,
                          int seed_tiles);
// owner[i] = rank whose cell range holds rows[i] (device arrays).
hipError_t knn_geom_assign_launch(const ShardGeom &g, const float *rows_dev, long long n, int *owner_dev, hipStream_t s);
// This rank's part of the seed layer, written into the whole-layer buffer `layer_dev` (device; the caller all-gathers the parts).
hipError_t knn_cells_seed_export(const FilterState &st, int rank, unsigned char *layer_dev, hipStream_t s);
// != 0 when gids[0 .. n) is not strictly ascending (device array).  Synchronous.
hipError_t knn_gids_check(const unsigned *gids_dev, long long n, unsigned *bad_out, hipStream_t s);
// Host rows -> device rows (r_dev, n x k floats) + filter layouts, chunk by chunk under the copy.  Synchronous.
hipError_t knn_filter_build_from_host(FilterState &st, int k, long long n, float *r_dev, const float *r_host,
                                      hipStream_t copy, hipStream_t compute);
// Host rows -> device rows + CELL-SORTED layouts, the fast build's bucket pass under the copy.  Always leaves the rows on the
// device; st.usable says whether the layouts stand (else the caller builds from the resident rows).  Synchronous.
hipError_t knn_filter_build_cells_from_host(FilterState &st, int k, long long n, float *r_dev, const float *r_host,
                                            hipStream_t copy, hipStream_t compute);
// Rows of the first of the (at most two) copies both ingests ship a shard of n rows x k floats in, a multiple of `granule` rows
// or n (one piece).  Host arithmetic only; knn_debug_ingest_head_rows.
long long knn_ingest_head_rows(int k, long long n, long long granule);
void knn_filter_free(FilterState &st);
// Asynchronous on `stream`: sample pre-pass + MFMA filter + exact re-rank + gated exact fallback.
// init_keys: the keys are written from scratch ((+INF, 0) first) instead of min-folded into what they hold.
// out_idx (nullable): the int32 indices of the batch as well (no separate unpack launch on the cell-pruned path).
// pruned: the cell-pruned scan answers the call (knn_query_route's QueryWay::Cells), else the full scan.
hipError_t knn_filter_query(FilterState &st, FilterCallOptions opt, bool pruned, int slot, int m, const float *q_dev, const float *r_dev,
                            long long base, u64 *keys_dev, int num_cu, hipStream_t stream,
                            hipEvent_t ev_begin, hipEvent_t ev_end, bool init_keys = false, int *out_idx = nullptr);
// opt.topk = c.K (1 .. KNN_TOPK_MAX).  A radius call reaches it as a plain one: the caller clips its lists behind.
hipError_t knn_filter_query_topk(FilterState &st, FilterCallOptions opt, int slot, const TopkCall &c);
// Top-K on the cell-pruned scan, the whole call in passes of KNN_CELL_BATCH queries (knn_cells_query_topk; c.ccap = tp.ccap).  A
// radius call: one-frame layouts cap their bound with it; the lists are NOT cut at it here (the gate lies slightly above): the
// caller clips them.
hipError_t knn_filter_query_topk_cells(FilterState &st, const CellTopkPlan &tp, int slot, const TopkCall &c);
// Counts on the cell-pruned scan (KNN_QUERY_COUNT_CELLS), the whole call in passes of KNN_CELL_BATCH queries (knn_cells_query_count).
// c.scratch [c.m] is zeroed here, once per call.
hipError_t knn_filter_query_count_cells(FilterState &st, const CellTopkPlan &tp, int slot, const CountCall &c);
// Lists on the cell-pruned scan (KNN_QUERY_COUNT_CELLS), the whole call in passes of KNN_CELL_BATCH queries (knn_cells_query_list).
hipError_t knn_filter_query_list_cells(FilterState &st, const CellTopkPlan &tp, int slot, const ListCall &c);
// Test hook: raw filter scores S[m][n] (row-major) and the per-query thresholds for a query
// batch, plus {sigma, eta, rho, amax, bmax}.  Synchronous.
hipError_t knn_filter_debug(FilterState &st, int m, const float *q_dev, const float *r_dev,
                            float *scores_dev, float *thr_out_dev, float *qnorm_out_dev,
                            double consts_host[8], hipStream_t stream);
