/*
 * knn_mi355x.h — C-ABI of libknn_mi355x.so: brute-force nearest-neighbour
 * search (1-NN, squared L2, fp32, first-minimum tie-break) on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE hot path of wu-kan/multicore-hw2: the
 * global cudaCallback() of reference sources/src/core.h:71 (defined at
 * sources/src/core.cu:1282-1297, which forwards to v8::cudaCallback,
 * core.cu:856-958).  Plain pointers and sizes only; no HIP, torch or C++ types.
 *
 * Results are bit-identical to the reference's serial v0 path
 * (core.cu:27-62): squared distance accumulated in fp32 in dimension order,
 * one rounding per operation (no FMA), and the lowest index among equal
 * minima.
 *
 * There is NO CPU fallback in this library.  Where the reference silently
 * computes on the CPU when no GPU is present (core.cu:869-870), this library
 * reports the error and exits like the reference's CHECK macro does for any
 * other runtime error (core.h:77-87).
 */
#ifndef KNN_MI355X_H
#define KNN_MI355X_H

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * 1. The drop-in entry point.  Replaces: core.h:71 / core.cu:1282-1297.
 *
 *   k, m, n            dimensions, #queries, #references (all >= 1)
 *   searchPoints       host, fp32, row-major [m][k]   (read-only, not freed)
 *   referencePoints    host, fp32, row-major [n][k]   (read-only, not freed)
 *   *results           set to a malloc()'d int[m]; caller free()s it
 *                      (core.cu:35,59,935; main.cu:98,175)
 *
 * results[j] = 0-based index of the reference nearest to query j.
 * Synchronous: all device work has finished on return.  The reference set is
 * split over every visible GPU in contiguous index ranges (the scheme of
 * core.cu:873-883) and the per-GPU winners are min-reduced as packed
 * (distance, global index) keys.  On a runtime error prints
 * "Error: <file>:<line>, code:<c>, reason: <text>" and exit(1)s (core.h:77-87).
 * ---------------------------------------------------------------------- */
void cudaCallback(int k, int m, int n, float *searchPoints, float *referencePoints,
                  int **results);

/* The host-input entry points (cudaCallback, knn_index_query_host, knn_index_create from host
 * rows) keep their device staging buffers in a small per-device pool between calls — hipMalloc +
 * hipFree cost more than the scan at the reference's test sizes.  At most 64 buffers / 4 GiB per
 * device; knn_trim() gives them all back to the runtime (returns the number of bytes released). */
long long knn_trim(void);

/* ------------------------------------------------------------------------
 * 2. Device-resident index API (not in the reference; cudaCallback is
 *    create + query + destroy over all GPUs).  Lets a caller keep the
 *    reference set in HBM across calls and time the kernels without PCIe.
 *    All functions return 0 on success, a negative KNN_E* code on failure;
 *    knn_last_error() gives the message for the calling thread.
 * ---------------------------------------------------------------------- */
typedef struct knn_index knn_index;

enum {
    KNN_OK = 0,
    KNN_EINVAL = -1,   /* bad argument */
    KNN_ENODEV = -2,   /* no usable GPU */
    KNN_EHIP = -3,     /* HIP runtime error */
    KNN_ENOMEM = -4
};

/* Packed result key: (float_bits(dist2) << 32) | global_index.  dist2 >= +0 so
 * unsigned order == lexicographic (distance, index) order == v0's first strict
 * minimum.  KNN_KEY_INIT = (+INF, index 0): what v0 returns when nothing
 * beats +INF (core.cu:39-40,50). */
#define KNN_KEY_INIT 0x7F80000000000000ull

int knn_device_count(void);
const char *knn_last_error(void);
const char *knn_version(void);

/* Build an index over one contiguous shard of the reference set on `device`.
 *   refs           fp32 row-major [n_local][k]; host pointer if
 *                  refs_on_device == 0 (copied to the GPU), else a device
 *                  pointer on `device` that must stay valid until destroy
 *                  (borrowed, not copied)
 *   base_index     global index of refs[0] (the shard offset that
 *                  core.cu:932-933 adds on the host; here it is folded into the
 *                  keys on the GPU)
 *   stream         hipStream_t as void* (NULL = default stream) used for the
 *                  layout-preparation kernels
 * n_local may be 0 (an empty shard: queries leave the keys untouched). */
int knn_index_create(knn_index **out, int device, int k, long long n_local, const float *refs,
                     int refs_on_device, long long base_index, void *stream);
void knn_index_destroy(knn_index *idx);

/* ------------------------------------------------------------------------
 * 2b. Cell-range shards (round 4): how a caller with several GPUs (one process per GPU, or one index per GPU in one process)
 *     splits the reference set so that the GPUs' scans ADD UP to the scan of one GPU holding everything.
 *     The reference splits by index range (core.cu:875-883) and so does cudaCallback here — rows arrive in the caller's
 *     order.  For a resident set that costs work: each range is gridded by itself at 1 / N of the resolution, and the ranks
 *     together do 3.8x the tile steps of one GPU at N = 8 (profiles/r04_shard_sim.txt).  Instead:
 *       1. every rank takes a strided sample of its rows; the samples are gathered (a few hundred KB) and
 *          knn_geom_create builds ONE grid from them — identical input, identical grid on every rank;
 *       2. knn_geom_assign says which rank's cell range each row falls into; the caller moves the rows there (one
 *          all-to-all at build time, not on the query path) together with their global numbers, ascending per rank;
 *       3. knn_index_create_sharded sorts a rank's rows into ITS cells of the global grid;
 *       4. knn_index_seed_export writes the first few tiles of each of the rank's cells into its part of a buffer of
 *          knn_geom_info()[5] bytes; the caller all-gathers the parts and hands the whole layer to knn_index_seed_attach
 *          (replicated: 151 MB for 2^16 cells).  A query bounds its answer from the 4 seed cells around it (16 measured slower, profiles/r04_seed_sweep.txt) — this rank's
 *          whole, the others' through the layer — so a rank prunes almost as if it saw everybody's rows.
 *     Queries, keys and the exchange step (min over the ranks' keys) are the same calls as for index-range shards: the
 *     keys carry global row numbers (gids) when the batch's last kernel has run.
 * ---------------------------------------------------------------------- */
typedef struct knn_geom knn_geom;
/* sample_host: samples x k floats, rows of the GLOBAL set (>= 64; a few thousand is plenty); seed_tiles: tiles of every cell
 * in the replicated layer (0 = 2).  KNN_EINVAL when the set does not suit (k > 16, too few rows per rank, degenerate sample). */
int knn_geom_create(knn_geom **out, int k, long long n_global, int nranks, const float *sample_host, long long samples,
                    int seed_tiles);
void knn_geom_destroy(knn_geom *g);
/* out = {bits of the global grid, its cells, cells per rank, seed tiles per cell, bytes of one rank's part of the seed layer,
 * bytes of the whole layer, bits of the low pruning table, ranks} */
int knn_geom_info(const knn_geom *g, long long out[8]);
/* First cell code of `rank`'s range (rank = the number of ranks: the number of cells); ranges start at multiples of 2^sa. */
long long knn_geom_first_cell(const knn_geom *g, int rank);
/* owner_dev[i] = rank whose cell range holds rows_dev[i] (device arrays on `device`; synchronous on return). */
int knn_geom_assign(const knn_geom *g, int device, const float *rows_dev, long long n, int *owner_dev, void *stream);
/* refs_dev: the rank's rows (device, borrowed); gids_dev[i]: global row number of refs_dev[i], STRICTLY ASCENDING, < 2^31
 * (device, borrowed) — v0's lowest-index tie-break is decided by local row order.
 * LIFETIME: refs_dev, gids_dev and the layer given to knn_index_seed_attach are BORROWED for the index's whole life: the prep,
 * scan and finalise kernels of every later query read them.  They must stay allocated and unchanged until knn_index_destroy
 * returns (a caller that lets them go gets use-after-free reads inside those kernels).  KNN_EINVAL when a row lies outside the
 * rank's cell range of the geometry.  The index must be given the seed layer (export on every rank, gather, attach) before
 * it is queried by more than one rank's worth of queries: without it the bound comes from the rank's own cells only —
 * still exact, only slower. */
int knn_index_create_sharded(knn_index **out, int device, const knn_geom *g, int rank, long long n_local, const float *refs_dev,
                             const unsigned *gids_dev, void *stream);
int knn_index_seed_export(knn_index *idx, void *layer_dev, void *stream);   /* this rank's part, in place in the whole-layer buffer */
int knn_index_seed_attach(knn_index *idx, const void *layer_dev);           /* the gathered layer (borrowed until destroy) */

/* Fill keys_dev[0..m) with KNN_KEY_INIT (async on stream). */
int knn_keys_init(int device, unsigned long long *keys_dev, int m, void *stream);

/* keys_dev[j] = min(keys_dev[j], key of the nearest reference of this shard to
 * query j).  queries_dev: device fp32 [m][k].  Asynchronous on `stream`.
 * Several shards (or GPUs, after an all-reduce MIN) may fold into one key
 * array; the minimum is the global answer. */
int knn_index_query_keys(knn_index *idx, int m, const float *queries_dev,
                         unsigned long long *keys_dev, void *stream);

/* Same, using query workspace `slot` (0 .. 7) of the index.  The index owns eight independent
 * workspaces, so up to eight batches may be in flight at once on their own streams (e.g. batch
 * i+1's small preparation kernels beside batch i's scan); calls that share a slot must be
 * stream-ordered by the caller.  Calls on one index from several host threads are serialised by the
 * index (a lock around the ~20 us of host work of a call; the GPU work of different slots still
 * overlaps); knn_index_last_stats then describes whichever call was enqueued last.  A slot outside
 * 0 .. 7 is KNN_EINVAL.
 * knn_index_query_keys == slot 0. */
int knn_index_query_keys_slot(knn_index *idx, int slot, int m, const float *queries_dev,
                              unsigned long long *keys_dev, void *stream);

/* Same, with flags.  KNN_QUERY_INIT_KEYS: the call WRITES the keys — (+INF, 0) min-folded with this shard's
 * answer — instead of folding into what keys_dev holds: the caller needs no knn_keys_init launch in front (the
 * cell-pruned path sets the keys inside its first kernel; the other paths issue the fill themselves). */
#define KNN_QUERY_INIT_KEYS 1u
int knn_index_query_keys_ex(knn_index *idx, int slot, int m, const float *queries_dev,
                            unsigned long long *keys_dev, void *stream, unsigned flags);

/* Same, and ALSO the int32 indices of the batch: indices_dev[j] = (int)(keys_dev[j] & 0xFFFFFFFF) once the shard's answer has
 * been folded in (indices_dev may be NULL: then exactly knn_index_query_keys_ex).  For a caller whose answer is this one
 * shard's (one GPU holds the whole set): on the cell-pruned path the indices are written by the last block of the batch's
 * last kernel, so the batch costs no knn_keys_to_indices launch; the other paths issue that launch themselves.  Callers that
 * merge several shards' keys first (min over shards / GPUs) pass NULL and unpack after the merge. */
int knn_index_query(knn_index *idx, int slot, int m, const float *queries_dev, unsigned long long *keys_dev,
                    int *indices_dev, void *stream, unsigned flags);

/* The path's one exchange step, for callers that keep one index per GPU in ONE process: min-reduce the
 * GPUs' key arrays with RCCL — ncclAllReduce(ncclUint64, ncclMin) per device inside
 * ncclGroupStart/End over xGMI, communicators from ncclCommInitAll created ONCE per process: the first call
 * fixes the device list, a later call with another list returns KNN_EHIP (merge those keys on the host).
 * Replaces the reference's host gather + CPU re-rank (core.cu:925-957).
 *   devices[g]    HIP device of key array g (each device at most once)
 *   keys_dev[g]   m packed keys on devices[g]; on completion every array holds the elementwise
 *                 unsigned minimum (= lexicographic (distance, index) minimum) of all of them
 *   streams[g]    hipStream_t as void* the reduction of array g is enqueued on (NULL array or NULL
 *                 entries = default stream); stream-ordered after the queries that wrote the keys
 * One process per GPU (bench.py) uses torch.distributed's all_reduce(MIN) on the same keys instead.
 * librccl is opened at first use; KNN_EHIP with the reason if it cannot be. */
int knn_keys_allreduce_min(int ndev, const int *devices, unsigned long long *const *keys_dev, int m,
                           void *const *streams);

/* out_dev[j] = (int)(keys_dev[j] & 0xFFFFFFFF) (async on stream). */
int knn_keys_to_indices(int device, const unsigned long long *keys_dev, int m, int *out_dev,
                        void *stream);

/* Convenience: host queries in, host indices out, synchronous. */
int knn_index_query_host(knn_index *idx, int m, const float *queries_host, int *out_host);

/* ------------------------------------------------------------------------
 * 2c. k-nearest neighbours (top-K), 1 <= K <= 64.
 *
 * For query j, keys_dev[j*K + t], t = 0 .. K-1, holds the K smallest packed keys of the shard's rows whose v0 distance is
 * finite (v0's strict `<` against +INF admits only these), in ascending order: distance first, then the lowest global
 * number.  A query with fewer than K such rows gets KNN_KEY_INIT (+INF, index 0) in the remaining slots.  Column 0 is the
 * 1-NN key for every input (NaN and overflowing rows included), and K = 1 equals knn_index_query bit for bit.  The keys
 * carry the same global numbers as the 1-NN keys: base_index + row for index-range shards, gids for cell-range shards.
 *
 * Folding shards: without KNN_QUERY_INIT_KEYS the call folds into what keys_dev holds (K sorted keys per query, e.g. the
 * answer of another shard): the result is the K smallest of (those keys and this shard's).  With the flag it writes the
 * keys fresh.  Global numbers are distinct across shards, so a fold never holds a row twice.  Cell-range shards fold too.
 * knn_keys_init and knn_keys_to_indices work on top-K keys as they are: pass m*K as their count.
 *
 * Paths (knn_index_last_stats [0]; options "path" and "cells" as for 1-NN): 2 = the MFMA filter, for the dense filter layouts
 * and for cell-sorted layouts in the shard's frame (scanned in full) — the threshold comes from the K-th smallest per-block
 * sample minimum, the survivors are evaluated with v0's arithmetic and the K smallest kept; a batch the filter cannot serve
 * (a query nothing bounds, fewer than K sampled blocks with a real row, more candidates than the buffers hold) raises [2] = 1
 * and is answered by the exact top-K scan; [1] = records re-ranked.  1 = the exact top-K scan (v0 arithmetic over every
 * row): per-cell frames (centred or 8-bit rows), grid indexes, cell-range shards, shards or batches below the filter's sizes.
 * 3 = the grid index, only for calls that carry KNN_QUERY_TOPK_GRID (below).  4 = the cell-pruned top-K (option "topk_cells");
 * on per-cell frames only for calls that carry KNN_QUERY_TOPK_FRAMES (below).
 * Results are bit-exact either way.
 * Any K outside 1 .. 64, or m < 1, is KNN_EINVAL (knn_last_error says why) and launches nothing.
 *
 * KNN_QUERY_TOPK_PARTIAL (knn_index_query_topk only; the 1-NN entry points reject it): the caller will MERGE this shard's lists
 * with those of every other shard of the set (knn_keys_topk_merge, or a fold), so a shard need only report the rows that can
 * belong to the GLOBAL top-K.  With the flag the call guarantees, for query j:
 *   - every row of the shard whose packed key is <= the K-th smallest key over ALL ranks' rows — the global set the geometry
 *     and the attached seed layer describe — is in the list (ties at the K-th distance included);
 *   - every other entry that is not padding is a real row of this shard with its bit-exact v0 key;
 *   - the list is strictly ascending, padding is KNN_KEY_INIT.
 * It does NOT guarantee a prefix of the shard's own top-K: a row between the global bound and the path's distance gate may be
 * present while a nearer one is absent (both are then beyond the global K-th key, so no merge can tell).  Merging every
 * rank's list gives the global top-K bit for bit, and so does folding (no KNN_QUERY_INIT_KEYS) one rank after the other: the
 * keys carry gids from the moment they are candidates.  What the flag buys: a cell-range shard (knn_index_create_sharded) with
 * option "topk_cells" = 1 takes the cell-pruned top-K ([0] = 4), its bound the K-th smallest seed score over K distinct rows
 * of the global set, those of other ranks scored from the seed layer.  Without a layer attached the bound comes from the rank's
 * own rows and the list is the shard's complete top-K.  On any other index, or under "topk_cells" 0 or 2, the flag is accepted
 * and changes nothing: full lists satisfy the contract.
 * ---------------------------------------------------------------------- */
#define KNN_QUERY_TOPK_PARTIAL 2u
/* KNN_QUERY_TOPK_GRID (knn_index_query_topk only; the 1-NN entry points reject it): the grid index may answer this top-K call.
 * With the flag, a call on an index that has a grid index, under option "path" 0 or 3, is served by it (knn_index_last_stats
 * [0] = 3): one wave per query walks the grid's rings as the 1-NN query does, keeps the K smallest keys seen — one per lane — and
 * stops once no unseen row can reach the K-th; a few hundred rows per query where the exact top-K scan reads the shard.  A
 * batch with a query the rings cannot finish (far outside the rows' box, an empty region) is answered by the exact top-K scan
 * instead ([2] = 1); [1] and [3] are 0.  On any other index or path the flag is accepted and changes nothing, and without it
 * every call goes exactly where it went before.  Results are bit-identical either way.  The library will take this path on its
 * own once it is measured against the exact top-K scan: the policy sends a call to a path only where it is measured faster than
 * the one it replaces (tools/grid_topk_timing.py takes those measurements). */
#define KNN_QUERY_TOPK_GRID 4u
/* KNN_QUERY_TOPK_FRAMES (knn_index_query_topk only; the 1-NN entry points reject it): a cell-sorted layout in per-cell frames may
 * answer this top-K call with the cell-pruned scan.  With the flag AND option "topk_cells" = 1, a call on a resident, non-sharded
 * index whose cell-sorted layout has per-cell frames — fp16 rows centred per cell ("cells_centre"), or 8-bit rows in each cell's
 * own frame ("cells_rows" 2 with "cells_u8_frame" 1); k <= 16 — takes the cell-pruned top-K (knn_index_last_stats [0] = 4) under
 * that path's call conditions: m >= 5, room for >= 64 candidate keys per query, out-of-box rows at most half that room, option
 * "path" 0 or 2.  Its bound is the K-th smallest of the FRAME-FREE distance bounds the seed cells' K smallest scores imply, each
 * through its own cell's constants ("Per-cell frames").  [1], [2] and [3] mean what they mean on the pruned top-K of
 * the one-frame layouts; folding, passes of 1024 queries, slots and indices_dev are unchanged.  On any other index, option or
 * path the flag is accepted and changes nothing, and without it every call goes exactly where it went before: per-cell frames
 * then take the exact top-K scan whatever "topk_cells" says.  Results are bit-identical either way.  On request: it has
 * not been measured against the exact top-K scan yet. */
#define KNN_QUERY_TOPK_FRAMES 8u
/* keys_dev [m][K]; indices_dev [m][K] or NULL: the int32 indices, unpacked after the fold.  Slot rules as knn_index_query:
 * eight workspaces, calls sharing one must be stream-ordered; asynchronous on `stream`. */
int knn_index_query_topk(knn_index *idx, int slot, int m, int K, const float *queries_dev, unsigned long long *keys_dev,
                         int *indices_dev, void *stream, unsigned flags);
/* b_dev[j] <- the K smallest of a_dev[j] and b_dev[j], sorted; both hold m sorted lists of K keys (device arrays on
 * `device`).  Merges shards, or GPUs after the caller has gathered their keys.  Asynchronous on `stream`. */
int knn_keys_topk_merge(int device, int m, int K, const unsigned long long *a_dev, unsigned long long *b_dev, void *stream);
/* Synchronous: host queries [m][k] in, indices_host [m][K] out; dist2_host [m][K] (may be NULL) receives the float of each
 * key's high word (+INF in padding slots). */
int knn_index_query_topk_host(knn_index *idx, int m, int K, const float *queries_host, int *indices_host, float *dist2_host);

/* Radius-bounded top-K: the K nearest rows WITHIN a distance.  Everything knn_index_query_topk says holds, with one change: a row
 * of the shard is a candidate when its v0 distance E is finite and E <= max_dist2 — an fp32 compare on the value in the key's high
 * word, equality inside.  keys_dev[j*K + t] holds the K smallest such keys, ascending, padded with KNN_KEY_INIT.
 * max_dist2 = +INF gives knn_index_query_topk's keys bit for bit; max_dist2 = 0 (-0 counts as 0) exact duplicates of the query
 * only; max_dist2 < 0 or NaN, and the plain call's bad arguments, are KNN_EINVAL and launch nothing.
 * The same four flags with the same meaning; under KNN_QUERY_TOPK_PARTIAL the list guarantee reads "every row with key <= the
 * global K-th key AND E <= max_dist2".  Without KNN_QUERY_INIT_KEYS the result is the K smallest of what keys_dev held and this
 * shard's candidates: the keys already there are the caller's and are NOT clipped.  Slots, passes of 1024, indices_dev and
 * knn_index_last_stats are as for the plain call, and the path is the plain call's for the same flags and options: the radius
 * changes no route.  The cap holds on every way out, a batch that falls back included.
 * What the radius buys ("Within a radius"): the grid index stops a query's ring walk as soon as the face bound passes
 * the radius — a query in an empty region or outside the rows' box ends with a short or empty list instead of sending its batch
 * to the exact top-K —; the cell-pruned scan of a one-frame layout caps its distance bound with the radius (fewer cells and
 * records, and a query with fewer than K rows in its seed cells is bounded and does not fall back); in the exact top-K scan a
 * row beyond the radius never enters a list.  The dense filter and per-cell frames (KNN_QUERY_TOPK_FRAMES) answer as for the
 * plain call and clip their lists in one more launch. */
int knn_index_query_topk_within(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                                unsigned long long *keys_dev, int *indices_dev, void *stream, unsigned flags);
/* Synchronous, as knn_index_query_topk_host; counts_host [m] (may be NULL) receives the number of entries of each list that are
 * not padding. */
int knn_index_query_topk_within_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                     int *indices_host, float *dist2_host, int *counts_host /* may be NULL */);

/* ------------------------------------------------------------------------
 * 2d. Counts within a radius: how many rows of the shard lie within a distance of each query.
 *
 * counts_dev[j] receives the number of rows of this shard whose v0 distance E to query j is finite and E <= max_dist2: fp32,
 * accumulated in dimension order, no FMA, an fp32 compare with equality inside — exactly the candidate rule of
 * knn_index_query_topk_within, whose lists hold at most 64 entries and cannot tell a complete list from one cut at K.
 * max_dist2 = +INF counts the rows with a finite distance; 0 (and -0) exact duplicates of the query; a query with a non-finite
 * coordinate has count 0.  max_dist2 < 0 or NaN, m < 1, a slot outside 0 .. 7, a null pointer or any flag other than the three
 * below are KNN_EINVAL with a knn_last_error text, and nothing is launched.
 * Folding: without KNN_QUERY_INIT_KEYS counts_dev[j] += this shard's count, with it counts_dev[j] = the count.  Counts of
 * disjoint shards add: index-range shards, cell-range shards (knn_index_create_sharded: as they are — no seed layer and no
 * KNN_QUERY_TOPK_PARTIAL contract is needed), GPUs after the caller has summed.  Counts are unsigned 32-bit: one shard's count is
 * at most n_local < 2^32, a fold wraps modulo 2^32.  An empty shard adds nothing (writes zeros under the init flag).
 * Asynchronous on `stream`; slots as for every other query (eight workspaces, calls that share one are stream-ordered by the
 * caller); 1-NN, top-K and count calls may follow one another on a slot in any order.
 * Ways (knn_index_last_stats [0]): 1 = the exact count scan, the default and what every call without a flag takes.  3 = the grid
 * index, when the index has one, the call carries KNN_QUERY_COUNT_GRID and option "path" is 0 or 3: a query's ring walk ends when
 * the face bound passes the radius.  4 = the cell-pruned scan, when the call carries KNN_QUERY_COUNT_CELLS, max_dist2 is finite,
 * the index has a cell-sorted layout in the shard's one frame (fp16 rows without per-cell frames, or 8-bit rows in bin frames),
 * k <= 32, m >= 5, "path" is 0 or 2 and "cells" is not 2; passes of 1024 queries.  On every other index a flag is accepted and
 * changes nothing.  Both fast ways are on request until they are measured against the exact count ("Counts within a
 * radius").  knn_index_last_stats: [1] records re-ranked (way 4; the last pass), [2] = 1 when the grid gave up or a cell pass
 * fell back and the exact count answered, [3] rows outside the robust box (way 4).  The count is exact on every way out. */
#define KNN_QUERY_COUNT_GRID  16u
#define KNN_QUERY_COUNT_CELLS 32u
int knn_index_count_within(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                           unsigned *counts_dev, void *stream, unsigned flags);
/* Synchronous: host queries [m][k] in, counts_host [m] out (this shard alone, written from scratch, the default way). */
int knn_index_count_within_host(knn_index *idx, int m, const float *queries_host, float max_dist2, unsigned *counts_host);

/* ------------------------------------------------------------------------
 * 2e. Lists within a radius (range queries): WHICH rows of the shard lie within a distance of each query — the second pass of the
 * classic count -> offsets -> fill scheme; 2d is its first.
 *
 *   knn_index_count_within (every shard, folding)  ->  knn_counts_to_offsets  ->  knn_index_list_within (every shard, appending)
 *   ->  knn_keys_sort_segments (when an order is wanted)
 *
 * Segment j of keys_dev is [offsets_dev[j], offsets_dev[j + 1]); its room is the difference, capped at 2^32 - 1 (descending
 * offsets: no room).  A row of the shard is a hit under exactly knn_index_count_within's rule: its v0 distance E is finite and
 * E <= max_dist2 — fp32, accumulated in dimension order, no FMA, an fp32 compare with equality inside, -0 counts as 0.  A hit's
 * packed key has E's bits in the high word and in the low word the global number the top-K keys carry (base_index + row, or the
 * gid on a cell-range shard).  It is stored at keys_dev[offsets_dev[j] + p], p being the value fill_dev[j] had when the hit
 * reserved its place; fill_dev[j] ends as its entry value plus this shard's number of hits, whether or not a hit was stored: a hit
 * whose p is not below the room is NOT stored, nothing is ever stored outside a query's segment, and fill_dev[j] > room is how the
 * caller sees an overflow — on the device, without a synchronisation.  With KNN_QUERY_INIT_KEYS the call zeroes fill_dev first;
 * without it the call appends, so disjoint shards fold by calling one after the other on a stream: index-range shards and
 * cell-range shards as they are (no seed layer, no KNN_QUERY_TOPK_PARTIAL contract), exactly as for counts.  fill_dev is unsigned
 * 32-bit, as the counts are.  Within a segment the order of the keys is unspecified, and so is what lies beyond fill_dev[j];
 * knn_keys_sort_segments gives the ascending (distance, global number) order.  An empty shard appends nothing.
 * max_dist2 < 0 or NaN, m < 1, a slot outside 0 .. 7, a null pointer or any flag other than KNN_QUERY_INIT_KEYS,
 * KNN_QUERY_COUNT_GRID and KNN_QUERY_COUNT_CELLS are KNN_EINVAL, each with its own knn_last_error text, checked before the index,
 * and nothing is launched.  Asynchronous on `stream`; slots as for every other query; 1-NN, top-K, count and list calls may follow
 * one another on a slot in any order.
 * Ways: chosen exactly as for a count call (2d; knn_debug_count_plan describes a list call too).  1 = the exact list scan, the
 * default.  3 = the grid index and 4 = the cell-pruned scan, by the same two flags under the same conditions; both reserve in the
 * slot's scratch cursor — a copy of fill_dev — and store behind it, and the cursor becomes fill_dev only when no query gave up and
 * no pass fell back; otherwise the exact list answers from the untouched fill_dev over the same places.  knn_index_last_stats: [0]
 * the way, [1], [2], [3] as for the count.  The lists are exact on every way out. */
/* offsets_dev[0] = 0, offsets_dev[j + 1] = offsets_dev[j] + counts_dev[j] (64-bit: totals pass 2^32).  Asynchronous. */
int knn_counts_to_offsets(int device, const unsigned *counts_dev, int m, unsigned long long *offsets_dev /*[m+1]*/, void *stream);
int knn_index_list_within(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                          const unsigned long long *offsets_dev /*[m+1]*/, unsigned *fill_dev /*[m]*/,
                          unsigned long long *keys_dev, void *stream, unsigned flags);
/* Sorts the first min(fill_dev[j], room of segment j) keys of every segment ascending; the entries beyond keep their bytes.
 * Asynchronous. */
int knn_keys_sort_segments(int device, int m, const unsigned long long *offsets_dev, const unsigned *fill_dev,
                           unsigned long long *keys_dev, void *stream);
/* Synchronous: count, offsets, list, sort on this shard alone (the default way).  offsets_host [m + 1]; *indices_out and
 * *dist2_out (dist2_out may be NULL) receive malloc()'d arrays of offsets_host[m] entries — a 1-entry allocation when the total
 * is 0 — that the caller free()s: query j's rows, nearest first, are entries offsets_host[j] .. offsets_host[j + 1] - 1. */
int knn_index_list_within_host(knn_index *idx, int m, const float *queries_host, float max_dist2,
                               long long *offsets_host, int **indices_out, float **dist2_out);

/* ------------------------------------------------------------------------
 * 2f. Top-K beyond 64: the exact K nearest rows for 1 <= K <= 4096.
 *
 * The contract of knn_index_query_topk_within (2c) holds word for word with 1 <= K <= KNN_TOPK_LARGE_MAX: a row of the shard is a
 * candidate when its v0 distance E is finite and E <= max_dist2 — fp32, accumulated in dimension order, no FMA, an fp32 compare
 * with equality inside, -0 counts as 0; max_dist2 = +INF is the plain top-K.  keys_dev[j*K + t] holds the K smallest candidate
 * keys ascending — distance first, then the lowest global number (base_index + row, or the gid on a cell-range shard) —, the
 * remaining slots KNN_KEY_INIT.  For K <= 64 the keys equal those of the radius-bounded call of 2c bit for bit on every input,
 * NaN and overflowing rows and non-finite queries included.
 * Flags: KNN_QUERY_INIT_KEYS alone.  With it the call writes the lists; without it the result is the K smallest of what keys_dev
 * held (K sorted keys per query, the caller's, NOT clipped) and this shard's candidates, so index-range shards or cell-range
 * shards (as they are: no seed layer) fold into the global list by calling one after the other on a stream.  Every other flag —
 * KNN_QUERY_TOPK_PARTIAL, KNN_QUERY_TOPK_GRID, KNN_QUERY_TOPK_FRAMES, both KNN_QUERY_COUNT_* — is KNN_EINVAL.
 * K outside 1 .. 4096, m < 1, m*K > INT_MAX, a slot outside 0 .. 7, max_dist2 < 0 or NaN and a null pointer are KNN_EINVAL, each
 * with its own knn_last_error text, checked in that order (a flag after the radius) — the sizes first, unlike 2g .. 2i, which look
 * at radius, flags and slot first; the host call below likewise — and before the index, and nothing is launched.
 * An empty shard leaves the keys alone (writes padding under the init flag).  Asynchronous on `stream`; slots as for every other query; 1-NN, top-K, count, list and
 * large calls may follow one another on a slot in any order.  indices_dev (may be NULL) receives the keys' low words.
 * One way on every index (knn_index_last_stats [0] = 1; DESIGN §4.6 "Top-K beyond 64"): a radix select over the packed keys finds
 * each query's K-th smallest candidate key in four scans of the shard — eight when some query's cut falls inside a class of equal
 * distances —, one more scan fills the lists, one launch sorts them.  knn_index_last_stats: [1] = 0, [2] = 1 when the index
 * word's passes ran (the last chunk of 65536 queries), [3] = 0.  The call it leaves alone has its limit of 64 as before. */
#define KNN_TOPK_LARGE_MAX 4096
int knn_index_query_topk_large(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                               unsigned long long *keys_dev /*[m][K]*/, int *indices_dev /*[m][K] or NULL*/,
                               void *stream, unsigned flags);
/* b_dev[j] <- the K smallest of a_dev[j] and b_dev[j], both sorted lists of K keys, 1 <= K <= 4096, in place: the any-K sibling
 * of the 64-key merge of 2c, for callers that gather GPUs' lists.  Asynchronous. */
int knn_keys_topk_merge_large(int device, int m, int K, const unsigned long long *a_dev, unsigned long long *b_dev, void *stream);
/* Synchronous, this shard alone: host queries [m][k] in, indices_host [m][K] out; dist2_host [m][K] (may be NULL) the float of each
 * key's high word (+INF in padding); counts_host [m] (may be NULL) the entries of each list that are not padding. */
int knn_index_query_topk_large_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                    int *indices_host, float *dist2_host /*NULL ok*/, int *counts_host /*NULL ok*/);
/* Test hooks, host arithmetic only.  knn_debug_topk_large_plan: in = {k, m, K, rows, CUs, 1 if init}; out = {chunks, slices of a
 * pass, distance passes, index passes at most, LDS bytes of the select kernel, scratch bytes of the slot, launches of a call whose
 * index passes stay gated off, launches with ties}.  knn_debug_radix_kth: the whole select over n given keys through the pick
 * kernel's own lines — *kth = the threshold T the fill uses: the K-th smallest key down to the last digit a pass had to fix, ones
 * below it (of distinct keys exactly K are <= T, and T is below the next one), or 0x7F7FFFFFFFFFFFFF when n < K; *passes_run =
 * the passes not gated off (above 4: the index word's passes ran). */
int knn_debug_topk_large_plan(const long long in[6], long long out[8]);
int knn_debug_radix_kth(const unsigned long long *keys, long long n, int K, unsigned long long *kth, int *passes_run);

/* ------------------------------------------------------------------------
 * 2g. Queries over a subset of the rows: the top-K and the count within a radius, asked of the rows a bit mask admits — the rows
 * of one tenant or label, the rows not deleted, everything but the rows already returned — without a second index and without
 * over-fetching.
 *
 * The mask: mask_dev is a device array of (n_local + 31) / 32 unsigned words on the index's device, borrowed for the call.  Bit
 * i % 32 of word i / 32 admits LOCAL row i: row i of the refs given to knn_index_create, row i of the refs_dev given to
 * knn_index_create_sharded — the order the exact scans read the rows in and number them base_index + row / gids[row].  Bits at and
 * beyond n_local in the last word are ignored, whatever they hold.
 * The contract is that of knn_index_query_topk_within (2c) and knn_index_count_within (2d) with one change: a row is a candidate
 * only when its mask bit is set AND its v0 distance E is finite and E <= max_dist2 — fp32, accumulated in dimension order, no FMA,
 * an fp32 compare with equality inside, -0 counts as 0; max_dist2 = +INF is the plain filtered top-K.  Keys carry the ORIGINAL
 * global numbers (base_index + row, or the gid), lists are ascending and padded with KNN_KEY_INIT, 1 <= K <= 64.  An all-ones mask
 * gives knn_index_query_topk_within's keys and knn_index_count_within's counts bit for bit on every input, NaN and overflowing rows
 * and non-finite queries included; an all-zero mask gives padding and zero counts.
 * Flags: KNN_QUERY_INIT_KEYS alone.  Without it the call folds into the K sorted keys held (the caller's, NOT clipped) or adds to
 * the counts, so disjoint shards, each with its own mask, fold by calling one after the other on a stream; with it the call writes
 * (an empty shard writes padding or zeros under it and otherwise leaves things alone).  Every other flag is KNN_EINVAL.
 * Argument errors are KNN_EINVAL, each with its own knn_last_error text, checked in this order — the first that fails speaks —:
 * max_dist2 < 0 or NaN, an unknown flag, a slot outside 0 .. 7, m < 1, K outside 1 .. 64, m * K > INT_MAX, a null queries, mask,
 * keys or counts pointer, a null index; nothing is launched.  Asynchronous on `stream`; slots as for every other query; masked
 * calls may follow or precede any other call on a slot.
 * One way on every index (knn_index_last_stats: [0] = 1, [1] = [2] = [3] = 0; DESIGN §4.6 "Over a subset of the rows"): the exact
 * masked scan.  No layout is consulted, so grid, cell-sorted, per-cell-framed and sharded indexes all answer.  The scan walks the
 * mask words — a zero word skips 32 rows without touching them, an admitted row costs what a row costs the exact scan — and cuts
 * the shard into slices of equal numbers of ADMITTED rows, so a mask that admits one contiguous range is spread over the whole
 * device like any other.  The mask may change between calls: every call counts it anew.
 * Lists within a radius and top-K beyond 64 over a mask: 2h. */
int knn_index_query_topk_masked(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                                const unsigned *mask_dev, unsigned long long *keys_dev /*[m][K]*/,
                                int *indices_dev /*[m][K] or NULL*/, void *stream, unsigned flags);
int knn_index_count_within_masked(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                                  const unsigned *mask_dev, unsigned *counts_dev, void *stream, unsigned flags);
/* mask_dev bits of the listed local rows <- value (1 set, 0 clear); rows outside 0 .. n_local-1 are ignored; async.
 * Serves allow-lists (memset 0, then set) and tombstones (memset 0xFF, then clear). */
int knn_mask_set_rows(int device, long long n_local, const unsigned *rows_dev, long long count, int value,
                      unsigned *mask_dev, void *stream);
/* Synchronous, this shard alone; mask_host: the words on the host.  dist2_host / counts_host may be NULL. */
int knn_index_query_topk_masked_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                     const unsigned *mask_host, int *indices_host, float *dist2_host, int *counts_host);
/* Test hooks, host arithmetic only.  knn_debug_masked_plan: in = {k, m, K (0 = a count call), rows, CUs, 1 if init}; out =
 * {granules of 1024 rows, slices of the first chunk of queries (the unmasked exact scan's number), chunks of 65536 queries, LDS
 * bytes of the scan, bytes of the slot's mask scratch, bytes of the slot's per-slice lists, kernel launches of an init call
 * (granule counts, prefix, per chunk the scan and — top-K — the select), queries of the first chunk}.  knn_debug_mask_split: the
 * cut the scan's blocks make, through their own lines (knn_mask_split.h), at its first step: first_granule[b], b = 0 .. slices, is
 * the least g with P[g] * slices >= b * T, P the exclusive prefix of granule_counts and T its total.  knn_debug_mask_split_rows:
 * the whole cut for a mask on the host: first_row[b] is the least row r with A(r) * slices >= b * T, A(r) the admitted rows before
 * row r — found inside granule first_granule[b] - 1 —; slice b is the rows [first_row[b], first_row[b + 1]). */
int knn_debug_masked_plan(const long long in[6], long long out[8]);
int knn_debug_mask_split(const unsigned *granule_counts, long long granules, int slices, long long *first_granule /*[slices+1]*/);
int knn_debug_mask_split_rows(const unsigned *mask_host, long long n_local, int slices, long long *first_row /*[slices+1]*/);

/* ------------------------------------------------------------------------
 * 2h. Lists within a radius and top-K beyond 64 over a subset of the rows: with 2g, every query kind the index answers — top-K up
 * to 64, top-K up to 4096, count, list — respects a mask.
 *
 * The mask is 2g's, layout and lifetime: (n_local + 31) / 32 words, bit i % 32 of word i / 32 admits LOCAL row i, bits at and
 * beyond n_local are ignored, borrowed for the call and counted anew on every call.  A row is a candidate only when its mask bit
 * is set AND its v0 distance E is finite and E <= max_dist2 (fp32, dimension order, no FMA, equality inside, -0 counts as 0).
 *
 * knn_index_list_within_masked: the contract of knn_index_list_within (2e) with that candidate rule — the third step of
 * knn_index_count_within_masked -> knn_counts_to_offsets -> this call -> knn_keys_sort_segments.  Keys carry the ORIGINAL global
 * numbers (base_index + row, or the gid).  A hit reserves p = fill_dev[j]++ and is stored at keys_dev[offsets_dev[j] + p] only
 * when p is below the segment's room; fill_dev[j] ends as its entry value plus this shard's admitted hits, stored or not; nothing
 * is ever stored outside a segment; the order inside a segment is unspecified.  KNN_QUERY_INIT_KEYS zeroes fill_dev first;
 * without it the call appends, so disjoint shards, each with its own mask, fold by calling one after the other.  An all-ones
 * mask gives exactly the set of keys the unmasked call gives; an all-zero mask stores nothing and leaves fill_dev at its entry
 * value.
 *
 * knn_index_query_topk_large_masked: the contract of knn_index_query_topk_large (2f) with that candidate rule.  1 <= K <=
 * KNN_TOPK_LARGE_MAX, lists ascending and padded with KNN_KEY_INIT; without KNN_QUERY_INIT_KEYS the call folds into the K sorted
 * keys held (the caller's, NOT clipped).  An all-ones mask gives knn_index_query_topk_large's keys bit for bit; for K <= 64 the
 * keys equal knn_index_query_topk_masked's bit for bit on every input, NaN and overflowing rows and non-finite queries included.
 * knn_index_last_stats reads [1, 0, t, 0], t = 1 when the index word's passes ran — some query's cut fell inside a class of
 * equal distances among the ADMITTED rows.
 *
 * Flags: KNN_QUERY_INIT_KEYS alone.  Argument errors are KNN_EINVAL, each with its own knn_last_error text, checked in this order
 * — the first that fails speaks, nothing is launched —: max_dist2 < 0 or NaN, an unknown flag, a slot outside 0 .. 7, m < 1,
 * (large) K outside 1 .. 4096, (large) m * K > INT_MAX, a null queries pointer, a null mask pointer, a null offsets, fill or keys
 * pointer, a null index.  Asynchronous on `stream`; slots as for every other query; these calls may follow or precede any other
 * call on a slot.  One way on every index (DESIGN §4.6 "Lists and large K over a subset of the rows"): no layout is consulted, so
 * grid, cell-sorted, per-cell-framed and sharded indexes all answer.  An empty shard appends nothing, or leaves the keys alone
 * (writes padding under the init flag). */
int knn_index_list_within_masked(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                                 const unsigned *mask_dev, const unsigned long long *offsets_dev /*[m+1]*/,
                                 unsigned *fill_dev /*[m]*/, unsigned long long *keys_dev, void *stream, unsigned flags);
int knn_index_query_topk_large_masked(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2,
                                      const unsigned *mask_dev, unsigned long long *keys_dev /*[m][K]*/,
                                      int *indices_dev /*[m][K] or NULL*/, void *stream, unsigned flags);
/* Synchronous, this shard alone; mask_host: the words on the host.  The list call runs masked count -> offsets -> masked list ->
 * sort and returns malloc'd arrays as knn_index_list_within_host does (a 1-entry allocation when the total is 0; the caller
 * frees them); the large call mirrors knn_index_query_topk_large_host.  dist2 / counts outputs may be NULL. */
int knn_index_list_within_masked_host(knn_index *idx, int m, const float *queries_host, float max_dist2,
                                      const unsigned *mask_host, long long *offsets_host /*[m+1]*/,
                                      int **indices_out, float **dist2_out /*NULL ok*/);
int knn_index_query_topk_large_masked_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2,
                                           const unsigned *mask_host, int *indices_host, float *dist2_host /*NULL ok*/,
                                           int *counts_host /*NULL ok*/);
/* Test hook, host arithmetic only.  in = {k, m, K (0 = a list call), rows, CUs, 1 if init}; out = {granules of 1024 rows, blocks
 * along the rows of the first chunk's scan (a list call: the masked count's slices; a large call: the select's), waves per block
 * that each take their own admitted-row slice (1; KNN_SELECT_WAVES = 8 for the select passes), chunks of 65536 queries, LDS bytes
 * of the scan, bytes of the slot's mask scratch, bytes of the slot's select scratch (0 for a list call), launches of an init call
 * whose index passes stay gated off: granule counts, prefix, then per chunk the list scan — or what knn_debug_topk_large_plan
 * counts for a call without ties, the state's memset included}.  A list call's [0], [1], [3], [5] are knn_debug_masked_plan's
 * [0], [1], [2], [4] for a count call on the same inputs: the count pass and the list pass cut the shard identically. */
int knn_debug_masked_lists_plan(const long long in[6], long long out[8]);

/* ------------------------------------------------------------------------
 * 2i. Queries about the shard's own rows: the K nearest OTHER rows of every row (the kNN graph), the number of other rows within a
 * radius (the degree of the radius graph) and the list of them (its adjacency).
 *
 * Query j of a call is LOCAL row row_first + j of the index: row row_first + j of the refs given to knn_index_create, or of the
 * refs_dev given to knn_index_create_sharded.  0 <= row_first, rows >= 1, row_first + rows <= n_local.  There is no queries
 * pointer: the coordinates are read from the resident rows, nothing is uploaded or gathered.
 *
 * Row i is a candidate for query j when i != row_first + j — identity by LOCAL ROW NUMBER: other copies of the row stay candidates,
 * at distance 0 —, its v0 distance E is finite, and E <= max_dist2 (fp32, dimension order, no FMA, equality inside, -0 counts as 0;
 * +INF: no radius).  Keys carry the global numbers every other call carries (base_index + row, or the gid).  A query row with a
 * non-finite coordinate has no candidate (every E is NaN or +INF): a padding list, count 0, nothing listed.
 *
 * knn_index_self_topk: 1 <= K <= 64; lists ascending, padded with KNN_KEY_INIT.  KNN_QUERY_INIT_KEYS writes; without it the call
 * folds into the K sorted keys held, which are the caller's and are NOT clipped.  indices_dev may be NULL.
 * knn_index_self_count_within, knn_index_self_list_within: 2d and 2e word for word with the candidate rule above — counts ADD; a
 * hit reserves p = fill_dev[j]++ and is stored at keys_dev[offsets_dev[j] + p] only when p is below the segment's room, so an
 * overflow shows in the cursor and nothing is ever stored outside a segment; the order inside a segment is unspecified;
 * KNN_QUERY_INIT_KEYS zeroes counts_dev / fill_dev first.
 *
 * Flags.  Count and list: KNN_QUERY_INIT_KEYS alone — one way on every index, the exact self-scan (DESIGN §4.6 "About the shard's
 * own rows"), as for the masked calls; knn_index_last_stats reads [1, 0, 0, 0].  Top-K also admits KNN_QUERY_TOPK_GRID and
 * KNN_QUERY_TOPK_FRAMES with their 2c meaning; KNN_QUERY_TOPK_PARTIAL and the KNN_QUERY_COUNT_* flags are KNN_EINVAL.  The top-K's
 * way is the one the plain top-K call of K + 1 neighbours (self is among ITS candidates) would take for `rows` queries under the
 * same flags and options: where that is the exact scan, always for K = 64, and where rows * (K + 1) would exceed INT_MAX (the plain
 * call's own limit), the exact self-scan answers with K; otherwise the
 * plain call runs as it is for K + 1 into slot scratch and one more launch removes self (the last entry when self is not among
 * the K + 1: then K + 1 other rows precede it) — so the grid index (with its flag), the MFMA filter and the cell-pruned scan
 * (option "topk_cells" 1, and KNN_QUERY_TOPK_FRAMES on per-cell frames) all serve the kNN graph, bit-exact, with the plain call's
 * own fallbacks inside, and knn_index_last_stats reports what the plain call reports.  A cell-range shard takes the self-scan.
 *
 * The graph of a set split over shards needs nothing new, because a row lives in one shard: make the self call on the row's own
 * shard, then the plain knn_index_query_topk_within, knn_index_count_within or knn_index_list_within call on every other shard
 * with the row block as queries_dev, folding (or the other way round: the self call folds too).
 *
 * Argument errors are KNN_EINVAL, each with its own knn_last_error text prefixed by the function's name, checked in this order —
 * the first that fails speaks, nothing is launched —: max_dist2 < 0 or NaN, an unknown flag, a slot outside 0 .. 7, rows < 1,
 * row_first < 0, (top-K) K outside 1 .. 64, (top-K) rows * K > INT_MAX, a null keys, counts, offsets or fill pointer, a null
 * index, row_first + rows > n_local (which needs the index: any call on an empty shard fails here).  Asynchronous on `stream`;
 * slots as for every other query; these calls may follow or precede any other call on a slot. */
int knn_index_self_topk(knn_index *idx, int slot, long long row_first, int rows, int K, float max_dist2,
                        unsigned long long *keys_dev /*[rows][K]*/, int *indices_dev /*[rows][K] or NULL*/, void *stream,
                        unsigned flags);
int knn_index_self_count_within(knn_index *idx, int slot, long long row_first, int rows, float max_dist2,
                                unsigned *counts_dev /*[rows]*/, void *stream, unsigned flags);
int knn_index_self_list_within(knn_index *idx, int slot, long long row_first, int rows, float max_dist2,
                               const unsigned long long *offsets_dev /*[rows+1]*/, unsigned *fill_dev /*[rows]*/,
                               unsigned long long *keys_dev, void *stream, unsigned flags);
/* Synchronous, the WHOLE shard, in blocks of 65536 rows on the default way (no flag but the init flag).  The top-K call fills
 * indices_host [n_local][K] (dist2_host: +INF in padding; counts_host: the entries of each list that are not padding; both may be
 * NULL).  The list call runs self count -> knn_counts_to_offsets -> self list -> knn_keys_sort_segments and returns the CSR
 * adjacency: offsets_host [n_local + 1] and malloc'd arrays as knn_index_list_within_host does (nearest first within a row; a
 * 1-entry allocation when the total is 0; the caller frees them); n_local <= INT_MAX there. */
int knn_index_self_topk_host(knn_index *idx, int K, float max_dist2, int *indices_host /*[n_local][K]*/,
                             float *dist2_host /*NULL ok*/, int *counts_host /*NULL ok*/);
int knn_index_self_list_within_host(knn_index *idx, float max_dist2, long long *offsets_host /*[n_local+1]*/,
                                    int **indices_out, float **dist2_out /*NULL ok*/);
/* Test hooks, host arithmetic only.  knn_debug_self_plan: in = {k, rows, K (0 = a count call, -1 = a list call), the shard's rows,
 * CUs, 1 if init}; out = {chunks of 65536 rows, slices of the first chunk (the plain exact scan's number for `rows` queries),
 * query groups of 64 of the first chunk, LDS bytes of the scan, bytes of the slot's per-slice lists, kernel launches of an init
 * call on the self-scan (per chunk the scan and — top-K — the select), rows of the first chunk, bytes of the through way's scratch
 * for this call: [rows][K + 1] keys, and [rows][K] more when the call folds; 0 for K = 64, count and list}.
 * knn_debug_self_ranges: the cut a block of the self-scans makes of its slice [i0, i1) around its window of own rows [w0, w1),
 * through the kernels' own lines (knn_self_window.h): out = {b0, b1, w0', w1', a0, a1} — the rows before the window, inside it
 * and after it: three disjoint ranges, ascending, whose union is [i0, i1). */
int knn_debug_self_plan(const long long in[6], long long out[8]);
int knn_debug_self_ranges(long long i0, long long i1, long long w0, long long w1, long long out[6]);
/* knn_debug_slice_chunks: the chunks every exact slice scan (2b-2m: top-K, count, list, select, masked, self, cluster sweep) walks
 * its queries in, and each chunk's cut of the shard's rows.  in = {queries, the shard's rows, CUs, K, rule}; rule 0: the count
 * scan's slices (K ignored), 1: the top-K scan's for 1 <= K <= 64, 2: a select pass's (K ignored).  out[i] = {first query, queries
 * (<= 65536), slices, rows of a slice, grid.x, grid.y} for chunk i < *chunks; cap: the rows of out, EINVAL when too few. */
int knn_debug_slice_chunks(const long long in[5], int cap, long long (*out)[6], int *chunks);

/* ------------------------------------------------------------------------
 * 2j. A radius per query: the counts and lists of 2d, 2e and 2i with ONE RADIUS FOR EVERY QUERY, read from a device array — ball
 * queries at each point's own scale, and "everything within the K-th neighbour's distance" (k-distance neighbourhoods with their
 * ties, core distances, locally scaled kernels) without a copy to the host or a synchronisation in between:
 *
 *   a top-K call  ->  knn_keys_column_dist2 (column K - 1)  ->  knn_index_count_within_each  ->  knn_counts_to_offsets
 *   ->  knn_index_list_within_each  ->  knn_keys_sort_segments
 *
 * max_dist2_dev is a device array of m (self forms: rows) floats on the index's device, borrowed for the call and read by its
 * kernels; no value in it is ever checked on the host.  cap is a host float, >= 0 or +INF, not NaN: an upper bound the caller
 * states for the radii; pass +INF when there is none.
 * Candidate rule: a row is a hit for query j when its v0 distance E is finite AND E <= max_dist2_dev[j] AND E <= cap — E in fp32,
 * accumulated in dimension order, no FMA; both tests plain fp32 compares with equality inside.  So a NaN or negative radius gives
 * query j no hit (never an error, never a fallback), -0 counts as 0, +INF is every row with a finite distance (under cap), and a
 * query with a non-finite coordinate has no hit, as in 2d.  Where a kernel prunes or stops by the radius it uses the query's bound,
 * max_dist2_dev[j] <= cap ? max_dist2_dev[j] : cap, and a query without candidates (max_dist2_dev[j] >= 0 fails) does no work.
 * cap is what lets the host plan: the way is chosen exactly as for the scalar call at max_dist2 = cap — the grid's ring limit from
 * cap, the cell-pruned way only at a finite cap — so knn_debug_count_plan describes these calls too.
 *
 * knn_index_count_within_each, knn_index_list_within_each: 2d and 2e word for word with the rule above — folding and
 * KNN_QUERY_INIT_KEYS, slots, the fill_dev / room / overflow contract, the global numbers in the keys (base_index + row, or the
 * gid), knn_index_last_stats; flags KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS with their 2d meaning.  On the
 * grid way a query without candidates never makes the batch give up.
 * knn_index_self_count_within_each, knn_index_self_list_within_each: 2i's count and list with the rule above (and i != row_first +
 * j); max_dist2_dev[j] belongs to LOCAL row row_first + j; KNN_QUERY_INIT_KEYS is the only flag, the exact self-scan the only way.
 * knn_keys_column_dist2: dist2_dev[j] = the float in the high word of keys_dev[j * K + column], 0 <= column < K, m >= 1; a
 * padding key gives +INF.  Asynchronous on `stream`; m < 1, K < 1, a column outside 0 .. K - 1 or a null pointer are KNN_EINVAL.
 *
 * Argument errors of the four device calls are KNN_EINVAL, each with its own knn_last_error text prefixed by the function's name,
 * checked in this order — the first that fails speaks, nothing is launched —: cap < 0 or NaN, an unknown flag, a slot outside
 * 0 .. 7, m < 1 (self: rows < 1, then row_first < 0), a null queries pointer (not the self forms), a null radii pointer, a null
 * counts pointer or a null offsets, fill or keys pointer, a null index, (self) row_first + rows > n_local. */
int knn_index_count_within_each(knn_index *idx, int slot, int m, const float *queries_dev, const float *max_dist2_dev, float cap,
                                unsigned *counts_dev, void *stream, unsigned flags);
int knn_index_list_within_each(knn_index *idx, int slot, int m, const float *queries_dev, const float *max_dist2_dev, float cap,
                               const unsigned long long *offsets_dev /*[m+1]*/, unsigned *fill_dev /*[m]*/,
                               unsigned long long *keys_dev, void *stream, unsigned flags);
int knn_index_self_count_within_each(knn_index *idx, int slot, long long row_first, int rows, const float *max_dist2_dev /*[rows]*/,
                                     float cap, unsigned *counts_dev /*[rows]*/, void *stream, unsigned flags);
int knn_index_self_list_within_each(knn_index *idx, int slot, long long row_first, int rows, const float *max_dist2_dev /*[rows]*/,
                                    float cap, const unsigned long long *offsets_dev /*[rows+1]*/, unsigned *fill_dev /*[rows]*/,
                                    unsigned long long *keys_dev, void *stream, unsigned flags);
int knn_keys_column_dist2(int device, const unsigned long long *keys_dev, int m, int K, int column, float *dist2_dev, void *stream);
/* Synchronous, host arrays in and out, this shard alone on the default way: knn_index_count_within_host and
 * knn_index_list_within_host (its malloc'd arrays and their 1-entry rule included) with max_dist2_host [m] and cap. */
int knn_index_count_within_each_host(knn_index *idx, int m, const float *queries_host, const float *max_dist2_host, float cap,
                                     unsigned *counts_host);
int knn_index_list_within_each_host(knn_index *idx, int m, const float *queries_host, const float *max_dist2_host, float cap,
                                    long long *offsets_host, int **indices_out, float **dist2_out /*NULL ok*/);
/* Test hook, host arithmetic only, through the kernels' own lines (knn_each_radius.h): out = {1 if a query of this radius has
 * candidates else 0, its bound under cap (0 when it has none)}.  cap < 0 or NaN is KNN_EINVAL. */
int knn_debug_each_radius(float radius, float cap, float out[2]);

/* ------------------------------------------------------------------------
 * 2k. The radius graph on the grid and cell-pruned ways: 2i's count and list (and their 2j forms) with the two pruned ways the
 * plain calls of 2d and 2e have on request.  The self calls of 2i and 2j know the exact self-scan alone and refuse every flag but
 * the init flag; these entry points admit KNN_QUERY_COUNT_GRID and KNN_QUERY_COUNT_CELLS as well.
 *
 * Candidate rule: exactly 2i's with 2j's radius rule.  Row i is a hit for query j — LOCAL row row_first + j — when
 * i != row_first + j (identity by local row number: other copies of the row stay hits, at distance 0), its v0 distance E is finite,
 * E <= the query's radius and E <= cap.  max_dist2_dev == NULL is the scalar form: every query's radius is cap, which may then be
 * +INF.  Otherwise max_dist2_dev [rows] is 2j's array word for word: a NaN or negative radius gives no hit and never an error, the
 * bound a kernel prunes or stops by is the smaller of the radius and cap.  Keys carry base_index + row, or the gid on a cell-range
 * shard.  Folding, KNN_QUERY_INIT_KEYS, the fill_dev / room / overflow contract, slots and asynchrony are 2i's.  For every input the
 * counts equal what the calls of 2i and 2j give, and every segment holds the same set of keys.
 *
 * Flags: KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS; anything else is KNN_EINVAL.  The way is the one
 * knn_index_count_within would take for `rows` queries at max_dist2 = cap under the same flags and options (knn_debug_count_plan
 * describes it), with the exact self-scan in the exact count's place: without a flag the call launches exactly what the call of 2i
 * or 2j launches.  On the grid way (k <= 4) a row's own position is dropped behind the distance; on the cell-pruned way (a finite
 * cap, a one-frame cell-sorted layout, rows >= 5) the pass's preparation, match and scan are the plain count's, launched on the
 * resident rows, and the kernels that turn its records into hits drop the query's own row.  Nothing is uploaded or gathered.  A
 * grid batch that gives up, and a cell-pruned pass that falls back, are answered by the exact self-scan, gated on the device.
 * knn_index_last_stats reports [0] = 1 / 3 / 4; [1], [2] and [3] mean what 2d says.
 *
 * Argument errors are KNN_EINVAL, each with its own knn_last_error text prefixed by the function's name, checked in this order —
 * the first that fails speaks, nothing is launched —: cap < 0 or NaN, an unknown flag, a slot outside 0 .. 7, rows < 1,
 * row_first < 0, a null counts pointer or a null offsets, fill or keys pointer, a null index, row_first + rows > n_local. */
int knn_index_self_count_within_routed(knn_index *idx, int slot, long long row_first, int rows,
                                       const float *max_dist2_dev /*[rows] or NULL*/, float cap, unsigned *counts_dev /*[rows]*/,
                                       void *stream, unsigned flags);
int knn_index_self_list_within_routed(knn_index *idx, int slot, long long row_first, int rows,
                                      const float *max_dist2_dev /*[rows] or NULL*/, float cap,
                                      const unsigned long long *offsets_dev /*[rows+1]*/, unsigned *fill_dev /*[rows]*/,
                                      unsigned long long *keys_dev, void *stream, unsigned flags);
/* Synchronous, the WHOLE shard in blocks of 65536 rows: routed self count -> knn_counts_to_offsets -> routed self list ->
 * knn_keys_sort_segments under `flags` (the init flag is implied); the CSR adjacency comes out as knn_index_self_list_within_host
 * returns it (malloc'd arrays, the 1-entry rule; n_local <= INT_MAX).  max_dist2_host [n_local] or NULL (the scalar form).  cap < 0
 * or NaN, an unknown flag, a null offsets or indices pointer and a null index are KNN_EINVAL, in this order. */
int knn_index_self_list_within_routed_host(knn_index *idx, const float *max_dist2_host, float cap, unsigned flags,
                                           long long *offsets_host /*[n_local+1]*/, int **indices_out, float **dist2_out /*NULL ok*/);
/* Test hook, host arithmetic only: knn_debug_count_plan's sixteen inputs with m = the call's rows (1 <= rows <= the shard's rows
 * <= 2^32) and its eight outputs; out[6] is the slices of the exact self-scan (knn_debug_self_plan's for a count call). */
int knn_debug_self_routed_plan(const long long in[16], long long out[8]);

/* ------------------------------------------------------------------------
 * 2l. Counts and lists within a radius over a subset of the rows, on the grid and cell-pruned ways: the masked count of 2g and the
 * masked list of 2h with the two pruned ways the plain calls of 2d and 2e have on request.  The masked calls of 2g and 2h know the
 * exact masked scan alone and refuse every flag but the init flag; these entry points admit KNN_QUERY_COUNT_GRID and
 * KNN_QUERY_COUNT_CELLS as well.  A tenant filter or a tombstone mask no longer takes a range query off the pruned ways.
 *
 * The contract is 2g's (count) and 2h's (list) word for word.  The mask: mask_dev is a device array of (n_local + 31) / 32
 * unsigned words on the index's device, borrowed for the call; bit i % 32 of word i / 32 admits LOCAL row i — the order of the refs
 * the index was created from, whatever order a layout keeps them in —; bits at and beyond n_local in the last word are ignored,
 * whatever they hold; the mask may change between calls.  A row is a candidate only when its mask bit is set AND its v0 distance E
 * is finite and E <= max_dist2 (fp32, accumulated in dimension order, no FMA, an fp32 compare with equality inside, -0 counts as
 * 0).  Keys carry the ORIGINAL global numbers: base_index + row, or the gid on a cell-range shard.  Without KNN_QUERY_INIT_KEYS the
 * call adds to the counts / appends behind fill_dev, so disjoint shards, each with its own mask, fold by calling one after the
 * other on a stream; with it counts_dev / fill_dev are zeroed first.  A hit reserves p = fill_dev[j]++ and is stored at
 * keys_dev[offsets_dev[j] + p] only when p is below the segment's room; fill_dev[j] ends as its entry value plus this shard's
 * admitted hits, stored or not; nothing is ever stored outside a segment; the order inside a segment is unspecified.  Asynchronous
 * on `stream`; slots as for every other query; these calls may follow or precede any other call on a slot.
 * For every input the counts equal knn_index_count_within_masked's and every segment holds the same set of keys as
 * knn_index_list_within_masked's; an all-ones mask gives what knn_index_count_within / knn_index_list_within give under the same
 * flags.
 *
 * Flags: KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS; anything else is KNN_EINVAL.  The way is the one
 * knn_index_count_within would take for m queries at max_dist2 under the same flags and options (knn_debug_count_plan describes
 * these calls too), with the exact masked scan in the exact scan's place: without a routing flag the call launches exactly what
 * the call of 2g / 2h launches.  On the grid way (k <= 4) a row inside the radius is a hit only when its bit is set; on the
 * cell-pruned way (a finite radius, a one-frame cell-sorted layout, m >= 5) the pass's preparation, match and scan are the plain
 * count's — they know no mask, their records name masked-out rows too — and the kernels that turn records into hits drop a row
 * whose bit is clear.  Either way the mask is read by LOCAL row number, for the rows inside the radius alone.  A grid batch that
 * gives up, and a cell-pruned pass that falls back, are answered by the exact masked scan, gated on the device.
 * knn_index_last_stats reports [0] = 1 / 3 / 4; [1], [2] and [3] mean what 2d says.
 *
 * Argument errors are KNN_EINVAL, each with its own knn_last_error text prefixed by the function's name, checked in this order —
 * the first that fails speaks, nothing is launched —: max_dist2 < 0 or NaN, an unknown flag, a slot outside 0 .. 7, m < 1, a null
 * queries pointer, a null mask pointer, a null counts pointer or a null offsets, fill or keys pointer, a null index.
 *
 * Not built: a radius per query under a mask (that needs an each-form of the exact masked scans); masked self calls; the masked
 * top-K on the pruned ways; a default policy — both pruned ways stay on request, as for the unmasked calls; using the mask to skip
 * whole cells (the walk and the scan visit what the unmasked call visits). */
int knn_index_count_within_masked_routed(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                                         const unsigned *mask_dev, unsigned *counts_dev, void *stream, unsigned flags);
int knn_index_list_within_masked_routed(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2,
                                        const unsigned *mask_dev, const unsigned long long *offsets_dev /*[m+1]*/,
                                        unsigned *fill_dev /*[m]*/, unsigned long long *keys_dev, void *stream, unsigned flags);

/* ------------------------------------------------------------------------
 * 2m. Clusters of the radius graph: density clustering (DBSCAN), friends-of-friends groups, the connected components of "closer
 * than r" — of the shard's own rows, straight from the index.  2i .. 2k give the radius graph's degrees and adjacency; this call
 * gives what they are for, without the adjacency ever being stored: one degree per row, then one idempotent unite per pair of core
 * rows within the radius, in the scans' hit path (a lock-free union-find in the labels array itself).  The device call always
 * answers about the WHOLE shard — clusters are a property of the set — so it takes no row_first / rows window.
 *
 * The definition; the answer depends neither on the way nor on thread timing.
 *   Degree.  deg(i) = the number of rows j != i (by LOCAL row number: another copy of the row counts) whose v0 distance E(i, j)
 *     is finite and <= max_dist2 — 2i's candidate rule word for word: fp32, accumulated in dimension order, no FMA, an fp32
 *     compare with equality inside, -0 counts as 0, +INF means no radius.
 *   Symmetry.  E is a sum of squares of differences; (a - b) and (b - a) differ in sign alone, their squares are the same
 *     float, and the sum runs over the dimensions in the same order: E(i, j) == E(j, i) bit for bit.  So "within the radius" is a
 *     symmetric relation, and everything below rests on it: a pair is seen from both rows alike, by every way.
 *   Core.  Row i is core when deg(i) + 1 >= min_pts: the row counts itself, as scikit-learn's min_samples does.
 *   Core labels.  Two core rows within the radius of each other belong to one cluster; a cluster is a connected component of the
 *     core rows under that relation.  labels_dev[i] of a core row = the SMALLEST local row number of a core row in its component.
 *   Border rows.  A row that is not core but has at least one core row within the radius takes the label of the core row with
 *     the smallest packed key (E's bits, local row number) among those: the nearest core row, the lower row number on a tie.
 *     (A border row joins no two clusters: only core rows link.)
 *   Noise.  Every other row gets KNN_CLUSTER_NOISE.  A row with a non-finite coordinate has deg 0: noise, or — min_pts == 1 — a
 *     cluster of its own.
 *   Label space.  Labels are LOCAL row numbers on every index: base_index and gids do not enter.  n_local <= INT_MAX.
 *   core_dev, when not NULL, receives the core rows as a bit mask in 2g's format ((n_local + 31) / 32 words, bit i % 32 of word
 *     i / 32), bits at and beyond n_local written 0: it can be handed straight to the masked calls ("query the core rows only").
 *   min_pts == 1 makes every row core: the labels are the connected components of the radius graph.
 * labels_dev is also the call's working memory (the degrees, then the union-find forest): its contents are the answer only once
 * the call's work on `stream` is done.
 *
 * Flags: KNN_QUERY_COUNT_GRID alone.  KNN_QUERY_INIT_KEYS has no meaning (the call always writes); every other flag,
 * KNN_QUERY_COUNT_CELLS included, is KNN_EINVAL.  The way is the one knn_index_self_count_within_routed takes for the shard's rows
 * at cap = max_dist2 under the same flag and options: the grid way on a grid index (k <= 4) with the flag and option "path" 0 or
 * 3, the exact self-scan everywhere else (a cell-range shard included).  Both the degree step and the link sweep take it.  A grid
 * batch that gives up is answered by the gated exact twins: the degrees through the routed count's commit, the links by a whole
 * exact sweep over whatever the grid walk left — unite and the border key's minimum are idempotent.  knn_index_last_stats
 * reports [0] = 1 or 3, [2] = 1 when a grid batch gave up.  Asynchronous on `stream`; slots as for every other query; the scratch
 * (8 bytes per row, and the mask's words when core_dev is NULL; on the grid way the routed count's 4 bytes per row as well) is the
 * slot's, grown on demand.
 *
 * Argument errors are KNN_EINVAL, each with its own knn_last_error text prefixed by the function's name, checked in this order —
 * the first that fails speaks, nothing is launched —: max_dist2 < 0 or NaN, an unknown flag, a slot outside 0 .. 7, min_pts < 1,
 * a null labels pointer, a null index, n_local > INT_MAX.  An empty shard succeeds and writes nothing.
 *
 * knn_index_self_cluster_within_host: synchronous, the device call on the default stream, copied back and RENUMBERED — clusters
 * 0 .. C - 1 in ascending order of their representative (smallest core) row, which for core rows is scikit-learn's numbering;
 * noise stays -1.  core_host [n_local] (NULL ok): 1 for a core row.  info (NULL ok) = {clusters, core rows, border rows, noise
 * rows}.  Errors, in this order: max_dist2, an unknown flag, min_pts < 1, a null labels pointer, a null index, n_local > INT_MAX.
 *
 * Test hooks, host arithmetic only.  knn_debug_cluster_plan: in = {k, the shard's rows, CUs, 1 if core_dev is given, 1 if the grid
 * way answers (k <= 4)}; out = {chunks of 65536 rows of the exact link sweep, slices of its first chunk, kernel launches of the
 * whole call on the exact way (per chunk the self count and the link sweep; core; flatten), the same on the grid way (grid count,
 * commit, the gated self count per chunk; core; grid link, the gated link sweep per chunk; flatten), bytes of the slot's cluster
 * scratch, bytes of the slot's count scratch on this way, the way (1 / 3), the launches on this way}.
 * knn_debug_cluster_unite: the kernels' own find / unite lines (knn_cluster_uf.h) with the host's atomics, one unite per pair, in
 * order, on parent [n] (on entry parent[x] <= x, e.g. parent[x] = x; pairs of rows 0 .. n - 1).
 *
 * Not built: clusters across shards (merging the ranks' components); a radius per row; compact numbering on the device; a mask of
 * admitted rows; evaluating a pair once for both rows (each sweep still meets a pair from either side).  (The cell-pruned way:
 * 2n.) */
#define KNN_CLUSTER_NOISE (-1)
int knn_index_self_cluster_within(knn_index *idx, int slot, float max_dist2, int min_pts, int *labels_dev /*[n_local]*/,
                                  unsigned *core_dev /*[(n_local+31)/32] or NULL*/, void *stream, unsigned flags);
int knn_index_self_cluster_within_host(knn_index *idx, float max_dist2, int min_pts, unsigned flags, int *labels_host /*[n_local]*/,
                                       unsigned char *core_host /*[n_local] or NULL*/, long long info[4] /*NULL ok*/);
int knn_debug_cluster_plan(const long long in[], long long out[]);   /* host arithmetic only */
int knn_debug_cluster_unite(int *parent, long long n, const int *pairs /*[npairs][2]*/, long long npairs);

/* ------------------------------------------------------------------------
 * 2n. Clusters on the routed ways: 2m's call with the cell-pruned scan as a third way, on request.  2m's two ways leave a k = 8 .. 32
 * shard in a cell-sorted layout with an O(n^2) clustering call; here its degree step and its link sweep both run in passes of 1024
 * own rows on the cell-pruned scan (KNN_QUERY_COUNT_CELLS), as 2k's routed count does.  2m's call stays as it is.
 *
 * The answer is 2m's, word for word: degree, symmetry, core, core labels (the smallest core local row of the component), border
 * rows (the label of the core row with the smallest packed key: E's bits, local row), noise, labels as LOCAL rows on every index,
 * core_dev in 2g's format, min_pts == 1 the connected components.  It depends neither on the way nor on thread timing: for every
 * input the labels and the core mask equal 2m's bit for bit.
 *
 * Flags: KNN_QUERY_COUNT_GRID and KNN_QUERY_COUNT_CELLS; anything else, KNN_QUERY_INIT_KEYS included, is KNN_EINVAL.  The way is the
 * one knn_index_self_count_within_routed takes for the shard's rows at cap = max_dist2 under the same flags and options
 * (knn_count_route, its precedence for a call that carries both flags included; knn_debug_count_plan describes it), and both the
 * degree step and the link sweep take it.  Without a flag, or with the grid flag alone, the call launches exactly what 2m's call
 * launches.  The cell-pruned way (4) needs all of: a finite max_dist2, a one-frame cell-sorted layout (fp16 rows without per-cell
 * frames, or 8-bit rows in bin frames), k <= 32, at least 5 rows, "path" 0 or 2, "cells" not 2.  A cell-range shard takes it as the
 * routed count does; its labels stay local rows.
 *
 * The link sweep on way 4, per pass of <= 1024 own rows first .. first + m - 1: the count pass's front unchanged (prep, match,
 * record-only scan, Q = R + first * k), then the link re-rank of the records and the link kernel of the layout's out-of-box rows.
 * A hit is a pair (own = first + query, row) with E finite, E <= max_dist2 and row != own; both core and row < own: unite(row,
 * own); own not core and row core: (E's bits, row) is folded into own's border key.  A pass unites exactly the pairs whose LARGER
 * row it owns and sets exactly its own rows' border keys, so it is self-contained: a pass that raises FALLBACK (a row nothing
 * bounds — far outside the box, or with a non-finite coordinate —, an over-full record list) is swept whole by the gated exact
 * link kernel over its own window, over whatever the record kernels left (unite and the key's minimum are idempotent: nothing is
 * committed), and touches no other pass.  knn_index_last_stats: [0] = 1 / 3 / 4; on way 4 [1], [2], [3] are 2d's for the LAST pass
 * that ran (the link sweep's last).  Scratch: 2m's (8 bytes per row, and the mask's words when core_dev is NULL) and the routed
 * count's 4 bytes per row, the slot's, grown on demand.
 *
 * Argument errors: 2m's rules in 2m's order, each text prefixed by the function's name — max_dist2 < 0 or NaN, an unknown flag
 * ("unknown flag (KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS)"), a slot outside 0 .. 7, min_pts < 1, a null labels pointer, a null
 * index, n_local > INT_MAX; the host form (2m's renumbering and info) skips the slot rule.  An empty shard succeeds and writes
 * nothing.
 *
 * Measured (MI355X, uniform rows, min_pts 5, the radius the median 10th-neighbour distance; profiles/cluster_cells_timing.txt):
 * medians of 5 calls, the whole call (degree step + link sweep with core and flatten), way 4 against way 1 of the same index —
 *   k 16, n 2^18:   55.048 ms (27.048 + 28.000) against  158.259 ms (  68.390 +   89.869)
 *   k 16, n 2^20:  182.707 ms (89.209 + 93.498) against 2746.771 ms (1140.563 + 1606.208)
 *   k  8, n 2^20:  104.167 ms (50.174 + 53.993) against 3230.807 ms (1275.537 + 1955.270)
 * way 4 was faster at every shape (2.87 x, 15.03 x, 31.02 x); labels and core masks equal; no pass fell back.  The link sweep keeps
 * the degree step's ratio (link 3.21 x, 17.18 x, 36.21 x against degree 2.53 x, 12.79 x, 25.42 x).  Dense blobs were not measured.
 *
 * Test hooks, host arithmetic only.  knn_debug_cluster_routed_plan: in = knn_debug_count_plan's sixteen inputs with m = the shard's
 * rows (<= INT_MAX), then 1 if core_dev is given; out = {the way (1 / 3 / 4), passes and the first pass's rows (way 4), kernel
 * launches of the whole call on that way — ways 1 and 3: knn_debug_cluster_plan's; way 4: per pass of the degree step prep, match,
 * scan, the count re-rank of the slices and of the overflow area, commit, the gated self-scan (7), core, per pass of the link sweep
 * the same front, the link re-rank of the slices and of the overflow area, the gated twin (6), flatten —, the same when the layout
 * has out-of-box rows (one more launch per pass in each sweep), bytes of the slot's cluster scratch, bytes of its count scratch on
 * this way, chunks of the exact link sweep}.  knn_debug_cluster_pair: the link kernels' own decision lines (knn_cluster_pair.h)
 * for one hit — *action = 0 nothing, 1 unite, 2 border key — from (own core, row core, row, own).
 *
 * Not built: a default policy (way 4 stays on request until someone decides from profiles/cluster_cells_timing.txt); skipping the
 * degree step when min_pts is 1; one pass front for both sweeps (the core bits need every degree first); clusters across shards, a
 * radius per row, a mask of admitted rows, per-cell-framed layouts, compact numbering on the device, evaluating a pair once. */
int knn_index_self_cluster_within_routed(knn_index *idx, int slot, float max_dist2, int min_pts, int *labels_dev /*[n_local]*/,
                                         unsigned *core_dev /*[(n_local+31)/32] or NULL*/, void *stream, unsigned flags);
int knn_index_self_cluster_within_routed_host(knn_index *idx, float max_dist2, int min_pts, unsigned flags, int *labels_host /*[n_local]*/,
                                              unsigned char *core_host /*[n_local] or NULL*/, long long info[4] /*NULL ok*/);
int knn_debug_cluster_routed_plan(const long long in[], long long out[]);   /* host arithmetic only */
int knn_debug_cluster_pair(int own_core, int row_core, long long row, long long own, int *action);

/* ------------------------------------------------------------------------
 * 2o. Minimum spanning forest of the shard's own rows (single linkage).  2m and 2n answer for ONE radius, fixed before the call;
 * the minimum spanning tree holds all radii at once: the single-linkage dendrogram, the friends-of-friends groups at every linking
 * length from one run, the backbone of HDBSCAN, the usual Euclidean-MST uses on point clouds.  The adjacency is never stored:
 * Borůvka rounds on the index, each a scan whose hit path is "the nearest row of ANOTHER component", a pick per component and a
 * hook (a lock-free union-find in the labels array itself, 2m's).
 *
 * The definition; the answer depends neither on the way nor on thread timing.
 *   Graph.  Vertices are the shard's LOCAL rows.  Rows i < j are joined when their v0 distance E(i, j) is finite and <= max_dist2
 *     — 2i's candidate rule word for word: fp32, accumulated in dimension order, no FMA, an fp32 compare with equality inside, -0
 *     counts as 0, +INF means no radius (the complete graph of the rows with finite coordinates).  E(i, j) == E(j, i) bit for bit
 *     (2m, "Symmetry").  A row with a non-finite coordinate has no edge.
 *   Edge order.  Edges are ordered by the triple (E's bits as unsigned, i, j), i < j, lexicographically: a strict total order, so
 *     the minimum spanning forest of the graph is UNIQUE — the set Kruskal accepts when it takes the edges in that order.  The call
 *     returns exactly that set: n_local - C edges, C the connected components of the graph.
 *   Labels.  labels_dev[i] = the smallest local row of i's component; for a finite radius, bit for bit, the labels of
 *     knn_index_self_cluster_within at min_pts 1.
 *   Labels and edge ends are LOCAL rows on every index, as in 2m.  n_local <= INT_MAX.
 *
 * The device call is asynchronous on `stream`, with no host round trip inside it.  Edge e, e < count_dev[0], is edge_keys_dev[e] =
 * (E's bits << 32 | i) and edge_hi_dev[e] = j, i < j; the order of the edges is unspecified.  count_dev[0] = the number of edges,
 * count_dev[1] = the number of rounds that added at least one.  Nothing is ever stored at or beyond entry n_local (a forest has at
 * most n_local - 1 edges: the reserve-and-test is a guard, not an overflow contract).  labels_dev is also the call's working
 * memory, as in 2m: its contents are the answer only once the call's work on `stream` is done.
 *
 * The rounds.  ROUNDS(n) = max(1, ceil(log2 n)); the call queues all of them, and every kernel of round t > 0 is gated on a device
 * word that round t - 1 raises when it adds an edge, so a run that finishes early costs empty launches only.  One round: flatten
 * (labels[i] = root(i), frozen until the hook); scan (per row the smallest key (E's bits, row) of a row of another component within
 * the radius — for a fixed row that is also its smallest edge —; a row that finds none is done for good, components only grow);
 * pick (per component the smallest offered edge: an atomic min of (E's bits << 32 | lo) on the root's slot, then of hi among the
 * rows that match it); hook (every root with a pick appends its edge through one cursor and unites its ends; when the component at
 * the other end picked the SAME edge only the one that holds `lo` appends, so every forest edge is stored exactly once).  Behind
 * the last round one more flatten, gated on the word that round raised: a hook re-parents only the larger root, and when even the
 * LAST queued round added an edge (rows paired at every level) no later round would bring the labels back to depth 1.
 *
 * Flags: KNN_QUERY_COUNT_GRID alone; every other flag, KNN_QUERY_INIT_KEYS and KNN_QUERY_COUNT_CELLS included, is KNN_EINVAL.  The way
 * is the one knn_index_self_count_within_routed takes for the shard's rows at cap = max_dist2 under the flag and options: the grid
 * way on a grid index (k <= 4) with the flag and option "path" 0 or 3, the exact self-scan everywhere else.  On the grid way a
 * row's walk ends by the radius clause or by the 1-NN walk's clause on the best key so far; a row that passes the ring limit raises
 * the round's give-up word, and that round's exact scan then runs over the whole shard (the candidate's atomic min is idempotent:
 * nothing is committed).  An infinite radius with the flag is legal and simply ends on the exact scan.  knn_index_last_stats
 * reports [0] = 1 or 3, [1] = 0, [2] = 1 when a grid round gave up (the last round that ran), [3] = 0.  Scratch, the slot's, grown
 * on demand: 20 bytes and one bit per row, and 2 ROUNDS(n) + 2 words.
 *
 * Argument errors are KNN_EINVAL, each with its own knn_last_error text prefixed by the function's name, checked in this order —
 * the first that fails speaks, nothing is launched —: max_dist2 < 0 or NaN, an unknown flag, a slot outside 0 .. 7, a null labels,
 * edge-keys, edge-hi or count pointer, a null index, n_local > INT_MAX.  An empty shard succeeds and writes count_dev = {0, 0}.
 *
 * knn_index_self_forest_within_host: synchronous, the device call on the default stream, copied back, the edges SORTED ascending
 * by (E, i, j) — the order single linkage merges in — into lo_host, hi_host and dist2_host (NULL ok), n_local entries each of which
 * the first info[0] are written; labels_host [n_local] (NULL ok).  info (NULL ok) = {edges, components, rounds run, 1 if a grid
 * round gave up}.  Errors, in this order: max_dist2, an unknown flag, a null lo or hi pointer, a null index, n_local > INT_MAX.
 *
 * Measured (MI355X, uniform rows, the radius the median 10th-neighbour distance; profiles/forest_timing.txt): medians of 5 calls, the
 * whole call, against what a caller did before it — knn_index_self_list_within_routed_host under the same flag plus Kruskal over
 * the CSR on the host (a numpy sort and a Python union-find in tools/forest_timing.py; in brackets scipy's minimum_spanning_tree
 * in its place) —
 *   k  3, n 2^20, the grid way:    14.433 ms against 3375.6 ms (list 67.8 + Kruskal 3307.7; scipy 946.9); 10 of 20 rounds added
 *                                  edges; 21.1 MB of scratch and 16.8 MB of outputs beside an 89.7 MB CSR
 *   k 16, n 2^16, the exact way:   30.640 ms against  163.5 ms (list 14.8 + Kruskal  148.8; scipy 128.9); 6 of 16 rounds
 *   k 16, n 2^16, exact, +INF:     35.940 ms; no route before (a list call needs a radius)
 * the sorted edge weights equal both routes' bit for bit.  The exact way at n 2^20, clustered rows, k 3 at +INF: not measured.
 *
 * Test hooks, host code only.  knn_debug_forest_plan: in = {k, the shard's rows, CUs, 1 if the grid way answers (k <= 4)}; out =
 * {ROUNDS, chunks of 65536 rows of one round's exact scan, slices of its first chunk, kernel launches of the whole call on the exact
 * way (per round: flatten, the scan's chunks, two offers, emit, hook; then the last flatten), the same on the grid way (one more per
 * round: the grid scan; the exact scan's chunks are then gated on its give-up word), bytes of the slot's scratch, the way (1 / 3), the launches on this
 * way}.  knn_debug_forest_round: ONE round's flatten, pick and hook by the kernels' own lines (knn_forest_pick.h,
 * knn_cluster_uf.h) with the host's atomics, on parent [n] (on entry parent[x] <= x, e.g. parent[x] = x) and a candidate array
 * cand [n] the caller made from the roots of `parent` (KNN_KEY_INIT: none); edges are appended at count[0], count[1] is raised when
 * the round added one, *added = the edges this round added.  On ENTRY *added = the number of host threads that share every step's
 * rows (below 2: the calling thread alone; at most 16), a join between two steps.  A call whose candidates are all KNN_KEY_INIT
 * is the flatten alone — the device call's last step: parent[x] = root(x) for every x.
 *
 * Not built: the cell-pruned way (way 4) for k = 8 .. 32; forests across shards; mutual-reachability weights (HDBSCAN's core
 * distances); the dendrogram or a cut of it on the device; a mask of admitted rows; a radius per row. */
int knn_index_self_forest_within(knn_index *idx, int slot, float max_dist2, int *labels_dev /*[n_local]*/,
                                 unsigned long long *edge_keys_dev /*[n_local]*/, unsigned *edge_hi_dev /*[n_local]*/,
                                 unsigned *count_dev /*[2]*/, void *stream, unsigned flags);
int knn_index_self_forest_within_host(knn_index *idx, float max_dist2, unsigned flags, int *labels_host /*[n_local] or NULL*/,
                                      int *lo_host, int *hi_host /*[n_local] each*/, float *dist2_host /*[n_local] or NULL*/,
                                      long long info[4] /*NULL ok*/);
int knn_debug_forest_plan(const long long in[], long long out[]);   /* host arithmetic only */
int knn_debug_forest_round(long long n, int *parent, const unsigned long long *cand, unsigned long long *edge_keys, unsigned *edge_hi,
                           unsigned *count, int *added);

/* Tuning / test hooks.  Known names:
 *   "path"    0 = auto, 1 = exact VALU kernels only, 2 = force the MFMA filter
 *             (+ exact re-rank) where its preconditions hold, 3 = the uniform-grid spatial index
 *             where k <= 4 and the data allows it (else the exact kernels).  Auto: resident shards
 *             with k <= 4 and >= 16384 rows get the grid index at creation and are served by it
 *   "shards"  cudaCallback only: split the reference set into this many
 *             shards.  0 = the library's rule: ONE GPU when n <= min(2^18, m << 10) (the reference's rule,
 *             core.cu:871-872: every case of the TA harness), else as many of the visible GPUs as the cost
 *             model says repay their fan-out (knn_debug_shard_policy; knn_get_option("last_shards") tells what the
 *             most recent call used).  Shards beyond the GPU count wrap around the devices — exercises the
 *             partition + merge logic on a single GPU.
 *   "filter_qt" tuning: query tiles (of 32) each filter wave keeps in registers: 8, 16 or 32
 *             (0 = chosen from m)
 *   "stream"  cudaCallback only: scan each shard chunk by chunk under its host-to-device copy
 *             with the exact kernels: 0 = when the cost model says so, 1 = never, 2 = always
 *             (shards of at least 64 MiB)
 *   "ingest"  indexes created from HOST rows (knn_index_create with refs_on_device = 0, and the
 *             staged-filter case of cudaCallback): 0 = the rows go over in chunks and every chunk's
 *             MFMA layouts are built as soon as it has landed (robust box from a strided host
 *             sample), 1 = copy everything, then build (the box from full-range statistics)
 *   "rccl"    cudaCallback only: how the shards' keys are merged: 0 = RCCL all-reduce when the set
 *             is split over ALL visible GPUs (one shard each), host merge otherwise (a process holds ONE
 *             communicator set, for all its GPUs: knn_get_option("rccl_comm_sets") is 0 or 1); 1 = RCCL
 *             whenever the shards are one per visible GPU (also with one GPU: a 1-rank communicator);
 *             2 = host merge always.
 *             knn_get_option("rccl_reductions") counts the merges RCCL has done,
 *             knn_get_option("rccl_version") is the loaded library's NCCL_VERSION_CODE (0: none)
 *   "cells"   the MFMA filter's cell-pruned form (k <= 32): the index sorts the shard into 2^B cells (every
 *             dimension — the first 16 when k > 16 — cut at sample quantiles), and a batch scores only the cells each query
 *             could not rule out by its distance to the cell's box.  0 = library policy: indexes created with
 *             knn_index_create of >= 2^19 rows (k <= 12), >= 2^20 rows (k = 13 .. 16), >= 2^22 rows (k = 17 .. 21), >= 2^23 rows
 *             (k = 22, 23) or >= 2^24 rows (k = 24, 25; beyond that too few cells are ruled out for the pruned scan to win); for the one-shot
 *             cudaCallback on shards of that size when the cost model says the batch repays the sort (the bucket pass of
 *             the sort runs under the host-to-device copy, ~1 ms per 2^24 rows stays behind the last byte: from about
 *             2500 queries on at n = 2^24; knn_get_option("last_cells") counts the shards of the most recent call
 *             that the pruned scan served).  1 = every index of >= 2^17 rows (k <= 32),
 *             cudaCallback's shards included; 2 = never.  Read when an index is created; 2 also makes
 *             existing indexes use the full scan.  Any distribution keeps its cells: a cell of many rows
 *             (clustered, low-rank data) is cut into several work items, empty cells cost nothing.  A batch
 *             the pruned path cannot bound (non-finite or far-away queries, no reference row found to bound a
 *             query with) is answered by the exact scan of the shard; a batch whose candidates overflow the
 *             record buffers (rows of a cluster tighter than the fp16 step) by the exact arithmetic over its
 *             listed (cell, query) pairs only; the next batch is back on the pruned path.  Results are
 *             bit-exact either way
 *   "scan_blocks" the pruned scan's blocks per CU: 0 = auto (two; one for shards of up to 2^15 cells while the index's last
 *             eight calls named more than one workspace slot — batches in flight side by side: the scan alone gets 10-20 %
 *             longer and the next batch's preparation kernels find room beside it, 5-7 % per step), 1, 2
 *   "run_thresholds" the LDS-tiled filter scan at 64 < k <= 512 (at k <= 128 for batches of at least 16 query tiles, m > 480;
 *             smaller batches there take the register scan): 0 / 1 = every score below a query's threshold lowers that
 *             threshold for the rest of the launch (threshold' = max(floor, score + margin), shared between blocks through an
 *             atomic minimum per query; the sample pass then only visits every 32nd tile), 2 = thresholds stay what the sample
 *             pass made them.  1-NN queries only: top-K runs with 2
 *   "sample_stride" the LDS-tiled filter scan (32 < k <= 512; at k <= 128 for batches of at least 16 query tiles): tiles the
 *             sample pass skips between two it scores (0 = library policy).  1-NN queries only; the other scans keep the policy
 *   "cells_centre" per-cell frames of the cell-sorted layout (k <= 16, not for cell-range shards): the fp16 fragments of a cell are
 *             taken about the middle of the cell's own box and scaled (by up to 2^8 more) to fill the fp16 range the rows of the
 *             whole shard share otherwise — the filter's rounding error shrinks from 2^-12 of the shard's box to 2^-12 of the
 *             cell's, what a set of tight clusters needs for its thresholds to separate anything.  0 = library policy: when the
 *             build's sample of the rows looks clustered (median nearest-neighbour distance inside the sample below 1/16 of the
 *             box); 1 = every cell-sorted layout; 2 = never.  Read when an index is built.  Costs one more pass over the rows at
 *             build time and ~100 instructions per (cell, 32 queries) at query time; results are identical either way.
 *             knn_get_option("cells_centred_builds") counts the layouts built so (read-only).
 *   "cells_rows" the rows the cell-pruned scan reads (k <= 16, not for cell-range shards): 1 = the fp16 fragments (32 bytes
 *             per row + a 4-byte norm); 2 = 8-bit codes in per-cell frames (8 bytes per half row: 16 bytes + the 4-byte norm),
 *             which brings per-cell frames with it; 0 = library policy (8-bit rows for shards of >= 2^24 rows whose build
 *             sample is uniform-like and not clustered).  Read when an index is built; results are identical either way.
 *             knn_get_option("cells_u8_builds") counts the layouts built with 8-bit rows (read-only).
 *   "cells_u8_frame" the frame of the 8-bit rows: 2 = per-dimension bins (one shard-wide scale, an offset per bin of every
 *             dimension: the layout stays in the shard's one frame and the scan takes a per-query operand), 1 = each cell's own
 *             frame, 0 = auto (bins where they fit the cells — uniform-like rows —, per-cell frames on clustered data).  Read when
 *             an index is built; results are identical either way.  knn_get_option("cells_u8_bin_builds") counts the layouts built
 *             with bin frames (read-only).  Top-K queries: bin frames can take the cell-pruned scan ("topk_cells"), per-cell
 *             frames take the exact top-K scan unless the call carries KNN_QUERY_TOPK_FRAMES (2c).
 *   "topk_cells" top-K queries (knn_index_query_topk) on the cell-pruned scan, for cell-sorted layouts in the shard's one frame
 *             (fp16 rows without per-cell frames, 8-bit rows in bin frames; k <= 32, m >= 5; a cell-range shard only for calls
 *             that carry KNN_QUERY_TOPK_PARTIAL, and only under 1; a layout in per-cell frames, k <= 16, only for calls that carry
 *             KNN_QUERY_TOPK_FRAMES, and only under 1 — without the flag per-cell frames take the exact top-K scan):
 *             0 = library policy: for now the same as 2 — the policy sends a call to this path only where it is measured faster
 *             than the path it replaces, and those measurements are not taken yet (it will start at the row count from which the
 *             library builds the cell-sorted layout on its own for that k);
 *             1 = wherever the layout allows it; 2 = never (the MFMA filter's full scan or the exact top-K scan, as before).
 *             Read at every call; results are identical either way.
 *   "cells_lists" who makes a cell's list of queries (those of the batch that cannot rule the cell out) on the pruned path:
 *             1 = knn_cells_match_kernel in a launch of its own between the preparation and the scan (lists in memory),
 *             2 = the scan's waves for the items they take (same test, same arithmetic, lists in LDS: one launch and one
 *             dependent round trip per item fewer), 0 = auto: 2 for shards of up to 2^13 cells queried one batch at a time
 *   "scan_deal" how the pruned scan's waves get their work items (runs of tiles of one cell): 1 = fixed (wave w takes items
 *             w, w + W, ...), 2 = a block owns a contiguous run and its waves take items from a counter in LDS (the launch
 *             is 6-8 % shorter: no wave is left with twice the average), 0 = auto: 2 for callers that query one batch at a
 *             time on shards with at least two items per wave, and for shards of more than 2^15 cells always; 1 below two items
 *             per wave, and on the smaller shards while the last eight calls on the index named more than one workspace slot
 *             (batches in flight fill each other's gaps; the fixed deal's cheaper prologue then gives the shorter step).  The automatic choices follow the caller's recent behaviour: a
 *             caller that goes back to one batch at a time gets the one-batch shapes again after eight calls
 *   "cells_build" how the cell-sorted layout is built: 0 = two passes (rows grouped into 256 buckets of consecutive cells, then
 *             placed bucket by bucket out of one XCD's L2; needs n x 72 bytes of scratch + 1/8: used for shards of up to 2^25 rows,
 *             and falls back when the scratch does not fit) in their FAST form — buckets of fixed room, no counting pass over the
 *             rows, tile ranges and work items from a device prefix, one synchronisation for the whole build; a bucket that
 *             outgrows its room (rows the cuts do not spread) makes the build start over in the counted form; 1 = the one-pass
 *             placement; 2 = the counted two-pass build (rounds 3-4: a pass for the bucket counts, two host round trips).
 *             Read when an index is created
 *   "filter_rounds" tuning: filter workgroups per resident slot (0/1 = one: persistent waves)
 *   "filter_chain" filter scans issued on different workspace slots / streams: 1 = run one
 *             after the other (event-chained), 2 = free to overlap, 0 = auto (chained when the
 *             shard is >= 16M references: a launch's duration then stays that of the kernel alone)
 * Returns KNN_EINVAL for an unknown name or value. */
int knn_set_option(const char *name, long long value);
long long knn_get_option(const char *name);

/* Statistics of the most recent knn_index_query_keys or knn_index_query_topk on this index (filled
 * when the stream has completed; call after synchronising):
 *   [0] path taken (1 exact, 2 filter, 3 grid index, 4 filter in its cell-pruned form)
 *   [1] candidates re-ranked exactly
 *   [2] how the device answered a batch the filter could not: 0 = it could; 1 = exact scan of the whole shard (a query
 *       nothing bounds: not finite, far outside the references' box); 2 = cell-pruned path only: more candidates than the
 *       record buffers hold (rows of a cluster tighter than the fp16 step), the batch's listed (cell, query) pairs were
 *       evaluated with the exact arithmetic — the cells the geometry ruled out stay ruled out
 *   [3] reference rows outside the filter's robust box (scanned exactly on every query)
 * A call of more than 1024 queries on the cell-pruned paths runs in passes of 1024: [1] and [2] are those of the LAST pass. */
int knn_index_last_stats(knn_index *idx, long long stats[4]);

/* Test / development hook: counters of the most recent batch on the cell-pruned path (call after synchronising; all 0
 * on other paths): [0] queries whose seed cells held no reference row (their bound came from a strided sample of the
 * layout), [1] cells whose query list outgrew its on-chip room (scored against the whole batch instead),
 * [2] cells of the index, [3] rows of its largest cell. */
int knn_index_debug_counters(knn_index *idx, long long out[4]);

/* Test hook: what the match launch of the most recent cell-pruned batch on workspace `slot` read and wrote, copied to the host
 * (waits for the device first).  what = 0 nothing (dims only), 1 the cells' list lengths (unsigned [ncells]; above cap: the list
 * is cut short), 2 the lists (unsigned short [ncells][cap]: the first min(length, cap) entries of a row are the cell's queries,
 * in the order of the block's queue), 3 the low pruning table (float [m_padded][low entries]), 4 the high one (float [high entries][m_padded]), 5 the
 * smallest of every 64 consecutive low entries (float [low entries / 64][m_padded]), 6 Dup (float [m_padded]); m_padded = the
 * batch's queries rounded up to 32.  At most `bytes` bytes are copied.  dims = {ncells, cap, low entries, high entries, queries
 * the tables have room for, first cell code of the index}. */
int knn_debug_cells_fetch(knn_index *idx, int slot, int what, void *out, long long bytes, long long dims[6]);
/* Test hook (host arithmetic only, no GPU needed): the match kernel's two tests, by the kernel's own lines, on n cases of one
 * high entry hi[i], one Dup dup[i] and 64 low entries lo[64 i .. 64 i + 63]: queued[i] = 1 if a block of those 64 cells takes the
 * query into its queue (the test on the smallest low entry), listed[i] = how many of the 64 cells keep it on their list. */
int knn_debug_match_tests(long long n, const float *lo, const float *hi, const float *dup, unsigned char *queued, unsigned char *listed);

/* Test hook (host arithmetic only, no GPU needed): the number of GPUs a cudaCallback(k, m, n, ...) is split over on a
 * node with ndev visible devices — the reference's rule (core.cu:865-872) plus the library's cost model. */
int knn_debug_shard_policy(int k, int m, long long n, int ndev);
/* Test hook (host arithmetic only): how ONE shard of `rows` rows of a one-shot cudaCallback(k, m, ...) would be served under the
 * current options: out = {filter layouts (0 none: exact kernels, 1 plain, 2 cell-sorted: the pruned scan), 1 if the exact scan
 * runs chunk by chunk under the copy, 1 if the grid index (k <= 4) serves it, copy calls of the streamed form}. */
int knn_debug_plan_shard(int k, int m, long long rows, long long out[4]);
/* Test hook (host arithmetic only, no GPU needed): everything a cudaCallback(k, m, n, ...) decides before it runs, under the
 * current options: in = {k, m, n, visible devices (faked), 1 if RCCL could be used (the answer its probe would give)};
 * out = {shards, rows per shard, host threads, exchange step (0 keys merged on the host, 1 RCCL all-reduce), refusal (0 none;
 * option rccl = 1 but 1: the shards are not the visible devices, 2: RCCL cannot be used), empty shards, rows of the last
 * non-empty shard, 1 if the RCCL probe was asked at all, [8..11] the way the plan gives shard 0 and [12..15] the way it gives the
 * last non-empty shard, each as knn_debug_plan_shard's four outputs}.  KNN_EINVAL unless k, m, n and the devices are >= 1. */
int knn_debug_call_plan(const long long in[5], long long out[16]);
/* Test hook (host arithmetic, no GPU): one row of k <= 16 coordinates through the 8-bit rows' quantiser (option "cells_rows"),
 * v = (row - centre) x scale in fp32: codes[k] = its bytes, out[0] = the largest per-coordinate error bound, out[1] = eta for a
 * query of largest |coordinate| amax.  0 on success. */
int knn_debug_u8_row(int k, const float *row, const float *centre, float scale, double amax, unsigned char *codes, double out[2]);
/* Test hooks (host arithmetic, no GPU) for the 8-bit rows in bin frames (option "cells_u8_frame"): knn_debug_u8_bin_row codes
 * one row, u = (row - centre) x scale, v = u - w in fp32 -> codes[k], *err = the largest per-coordinate error bound;
 * knn_debug_u8_bin_threshold -> *thr, the scan's threshold for a query whose fp16 B operand in the bins' units has the bits
 * b_bits[16], with Dup dup (shard units), 2^e ratio and the shard's largest err, N'' and sum |w|.  0 on success. */
int knn_debug_u8_bin_row(int k, const float *row, const float *centre, float scale, const float *w, unsigned char *codes, double *err);
int knn_debug_u8_bin_threshold(int k, const unsigned short *b_bits, float dup, float ratio, float er, float nmax, float w1, float *thr);

/* Test hook (host arithmetic only, no GPU needed): every size one scan launch of the cell-pruned path and the re-rank behind
 * it index with, for an index of `nitems` work items on a device of num_cu CUs and a batch of m <= 1024 queries:
 * out = {scan blocks, record lists (= scan waves), records per list, first record of the shared overflow area, its
 * capacity, dynamic LDS bytes of the scan, records a workspace holds, list counters a workspace holds}. */
int knn_debug_scan_plan(int num_cu, int blocks_per_cu, unsigned nitems, int m, long long out[8]);
/* The same with the list maker named: self_lists != 0 = the scan's waves list their own items (option "cells_lists" 2): the
 * dynamic LDS then also holds the batch's Dup values and one list room per wave. */
int knn_debug_scan_plan_ex(int num_cu, int blocks_per_cu, unsigned nitems, int m, int self_lists, long long out[8]);
/* Test hook (host arithmetic only, no GPU needed): every choice and size one batch of the cell-pruned query launches with.
 * in = {k, kt, centred, rows_u8, ncells, nitems, cap, several_slots, scan_blocks, scan_deal, cells_lists, m, num_cu, rec_cap};
 * out = {prep: PW, KT, CTR; self_lists; match: waves (0 none), stage, dynamic LDS; the scan's form: DYN, K, SELF, KT, CTR,
 * NIF, U8; its grid: blocks, waves, record lists, records per list, overflow base, overflow capacity, dynamic LDS; list_cap;
 * tail: K, KT, blocks; 1 if the gated exact scan is a launch of its own; the LDS limits of the scan and the match kernel
 * (0: the default)}. */
int knn_debug_cells_query_plan(const long long in[14], long long out[28]);
/* Test hook (host arithmetic only, no GPU needed): whether a top-K call takes the cell-pruned scan and what one of its passes
 * launches with.  in = {k, K, m (the call's queries), rows of the shard, option topk_cells, 1 if a cell-sorted layout exists,
 * centred (1: per-cell frames; 2: per-cell frames and the call carries KNN_QUERY_TOPK_FRAMES — with 8-bit rows in bin frames, which
 * are never centred, 2 means the flag alone), rows_u8, 1 if the 8-bit rows are in bin frames, 1 for a cell-range shard (2: and the call carries
 * KNN_QUERY_TOPK_PARTIAL), out-of-box rows, ncells, nitems, cap,
 * several_slots, scan_blocks, scan_deal, num_cu, rec_cap, option cells};
 * out = {1 if pruned; prep: PW, KT, CTR; match: waves, stage; the record-only scan's form: DYN, KT, NIF, U8, SELF, CTR; its grid:
 * blocks, waves, record lists, records per list, overflow base, overflow capacity, dynamic LDS; list_cap; candidate keys per
 * query; passes; the LDS limits of the scan and the match kernel; queries of the first pass}.  Everything after out[0] but the
 * candidate keys is 0 when the call is not pruned. */
int knn_debug_cells_topk_plan(const long long in[20], long long out[25]);
/* Test hook (host arithmetic, no GPU): the value the top-K form of the cell-pruned path's preparation kernel hands to the
 * threshold — the K-th smallest finite score among nseed seed scores as a block of pw (2 or 4) waves selects it, the nwide
 * scores of the strided sample merged in when fewer than K are finite; +INF when still fewer.  0 on success. */
int knn_debug_seed_kth(const float *seed, int nseed, const float *wide, int nwide, int K, int pw, float *out);
/* Test hook (host arithmetic, no GPU): the threshold of a query of the cell-pruned path from a seed score u (filter units), for a
 * shard of scale sigma, largest |fp16 query coordinate| amax, |fp16 row coordinate| bmax, row norm nmax, and the query's computed
 * norm mq: out = {the score threshold, Dup (the largest scaled squared distance a candidate can have, fp32 rounded up), the
 * distance gate of the top-K re-rank: the largest v0 distance (rows' own units) a row of the top-K can have}.  0 on success. */
int knn_debug_topk_gate(int k, float sigma, double amax, double bmax, double nmax, double u, double mq, double out[3]);
/* The same three for a call of knn_index_query_topk_within with radius max_dist2 (>= 0, +INF allowed): Dup is capped at
 * sigma^2 (max_dist2 (1 + g2) + tau), u = +INF (fewer than K finite seed scores) leaves that cap alone, and the gate then lies
 * slightly above max_dist2 (the exact cut is made behind).  max_dist2 = +INF gives knn_debug_topk_gate's values exactly. */
int knn_debug_within_bound(int k, float sigma, double amax, double bmax, double nmax, double u, double mq, float max_dist2,
                           double out[3]);
/* Test hook (host arithmetic, no GPU): what the per-cell-frame top-K form of the preparation kernel makes of one seed score
 * (knn_frame_dup.h: the kernel runs the same lines).  frame = {the cell's centre [16], scale, ratio = scale / sigma (a power of
 * two), largest |fp16 row coordinate|, largest row norm} (KNN_CELL_FRAME_WORDS = 20 floats), query_row = k floats, u = a finite
 * seed score of that cell (the far branch takes any finite value): out = {Dup — the bound on that row's real squared distance in
 * the SHARD's scaled units, fp32 rounded up, +INF when nothing bounds it; 1 if the query does not fit the frame (far branch)}. */
int knn_debug_frame_dup(int k, const float frame[20], const float *query_row, float u, float out[2]);
/* Test hook (host arithmetic only, no GPU needed): every choice and size one batch of the dense filter query launches with.
 * in = {kt, ntiles, m, num_cu, rec_cap, K (0 = 1-NN), and the options filter_qt, filter_rounds, filter_chain, run_thresholds,
 * sample_stride};
 * out = {ok, form (0 register pieces, 1 LDS-tiled, 2 chunked-K), KT, pieces, record lists, records per list, sample stride,
 * sample blocks, sample minima (floats), K of the K-th-minimum launch (0 none), sample rows of the thresholds kernel, 1 if it
 * writes running thresholds, 1 if the scan reads them, 1 if the scan is in the slots' chain, 1 if it waits and records there,
 * 1 if records carry row masks; per piece (four) {QT, first tile, tiles, grid x, grid y, first list}; the re-rank's pieces,
 * first lists [4] and first query rows [4]}. */
int knn_debug_filter_query_plan(const long long in[11], long long out[49]);
/* Test hook (host arithmetic only, no GPU needed): which path answers a call on a shard of n > 0 rows (the value
 * knn_index_last_stats reports in [0]), under the options given as inputs.  in = {the twenty inputs of
 * knn_debug_cells_topk_plan — K = 0: a 1-NN call; "1 if a cell-sorted layout exists": filter layouts exist and are cell-sorted —,
 * option path, 1 if the index has filter layouts, 1 if it has a grid index (never together with a cell-range shard), 1 if the
 * creator asked for the filter layouts, 1 if the call carries KNN_QUERY_INIT_KEYS};
 * out = {the way: 1 exact, 2 filter, 3 grid index, 4 cell-pruned; 1 if the keys are set to (+INF, 0) by a launch of their own
 * first (1-NN); top-K: candidate keys per query, 1 if knn_debug_cells_topk_plan takes the call, its passes and the first pass's
 * queries}. */
int knn_debug_query_route(const long long in[25], long long out[6]);
/* Test hook (host arithmetic only, no GPU needed): what a top-K call that carries KNN_QUERY_TOPK_GRID launches with.
 * in = {k (1 .. 4), K, m, 1 if the index has a grid index, option path, 1 if the call carries the flag};
 * out = {1 if the grid index answers the call; rings a query walks before it gives up; blocks; waves per block (one query each);
 * bytes of the slot's list scratch for a folding call ([m][K] keys); launches of a folding call: the grid kernel, the gated exact
 * top-K (a scan and a select per 65536 queries), the fold}.  Everything after out[0] is 0 when the grid does not answer. */
int knn_debug_grid_topk_plan(const long long in[6], long long out[6]);
/* The same for knn_index_query_topk_within: in = {the six inputs of knn_debug_grid_topk_plan, the rings the radius spans on the
 * grid (the library computes them from the cell widths, a degenerate axis ignored; 0 = none)}; out = the same six.  The rings
 * raise out[1] to themselves while a walk of that many rings stays within 2^15 cells, (2 rings + 1)^k; beyond that the plain
 * value and the give-up rule stand. */
int knn_debug_grid_within_plan(const long long in[7], long long out[6]);
/* Which way answers a knn_index_count_within call and what it launches with (host arithmetic, no GPU).  in = {k, m, rows, 1 if
 * the radius is finite, KNN_QUERY_COUNT_GRID given, KNN_QUERY_COUNT_CELLS given, has a grid index, has a cell-sorted layout,
 * per-cell frames, 8-bit rows, bin frames, cell-range shard, option "path", option "cells", CUs, the rings the radius spans on the
 * grid}; out = {way (1, 3, 4), passes and the first pass's queries (way 4), the grid's rmax, blocks and waves per block (way 3),
 * slices of the exact count scan, bytes of the slot's count scratch}.  Bad inputs are KNN_EINVAL.  A knn_index_list_within call
 * with the same arguments takes the same way, slices and passes, and the bytes also cover it: the count scratch [m] serves as its
 * scratch cursor. */
int knn_debug_count_plan(const long long in[16], long long out[8]);
/* Test hook (host arithmetic only, no GPU needed): the bytes a workspace slot's three top-K buffers must hold for a call.
 * in = {the way that answers it (knn_index_last_stats' [0]: 1 exact, 2 filter, 3 grid, 4 cell-pruned), m, K, the shard's rows,
 * the device's compute units, 1 if the call carries KNN_QUERY_INIT_KEYS, 1 if it has a finite radius, the queries of a pass of
 * the cell-pruned way (0 on the others), out[4] of knn_debug_grid_topk_plan on the grid way (0 on the others)};
 * out = {the exact top-K scan's per-slice lists; the filter ways' candidate lists and counters, or a folding grid call's lists;
 * the unclipped lists of a radius call on the filter ways}. */
int knn_debug_topk_scratch(const long long in[9], long long out[3]);
/* Test hook (host arithmetic only, no GPU needed): what an index is built with.  in = {k, n_local, 1 if the rows are on the
 * device, build_filter (-1 library policy: knn_index_create; 0 none, 1 the MFMA filter layouts, 2 cell-sorted), build_grid (-1
 * library policy, 0, 1), and the options path, cells, ingest, cells_build};
 * out = {1 if the creator asked for the layouts below the size rule, 1 if the layouts are cell-sorted, the resolved build_filter,
 * 1 if the grid index is tried first, 1 if the layouts are built (unless the grid index serves the shard), how host rows reach
 * the device: 0 copy then build, 1 layouts under the copy, 2 cell sort under the copy}. */
int knn_debug_index_build_plan(const long long in[9], long long out[6]);
/* Test hook (host arithmetic only, no GPU needed): how an index created from host rows splits the copy of its shard.
 * in = {k, n_local (0 .. 2^40), the granule in rows (a multiple of 32 up to 2^20: 1024 for the plain layouts under the copy,
 * 4096 for the cell sort under the copy)};
 * out = {rows of the first copy: everything but the last 64 MiB, rounded down to the granule, when the shard is larger than
 * 128 MiB — or n_local, one copy, for smaller shards and where that would leave less than one granule; the second copy is
 * the rest}. */
int knn_debug_ingest_head_rows(const long long in[3], long long out[1]);

/* Test hook for the filter's error bound: raw MFMA filter scores S[m][n_local] (row-major,
 * device) for a query batch, the fp32 squared norms M[m] of the fp16 query rows (device), and
 * consts = {sigma, eta, rho, Amax, Bmax, g2, gamma, #non-finite fp16 query coordinates}.  A pair's
 * score obeys |S + M - sigma^2 d^2| <= 2 eta sigma d + eta^2 + rho (+ gamma M), d = real distance.
 * Synchronous; needs an index that has filter layouts in row order (else KNN_EINVAL / KNN_EHIP: a cell-sorted
 * index — option "cells" — has no [m][n_local] score matrix). */
int knn_debug_filter_scores(knn_index *idx, int m, const float *queries_dev, float *scores_dev,
                            float *qnorm_dev, double consts[8]);

/* Bench support: time the index's dominant kernel (the one the roofline is quoted for) with a
 * HIP event pair recorded on the caller's stream around the launch.  enable = N > 0 brackets every
 * N-th later knn_index_query_keys (1 = all; an event record costs the stream ~5 us, which shows
 * in sub-100-us steps), 0 stops and drops the record. */
int knn_index_timing(knn_index *idx, int enable);
/* Waits for the recorded events, returns how many launches were timed and their summed
 * duration in milliseconds, and clears the record. */
int knn_index_timing_read(knn_index *idx, int *launches, double *total_ms);

/* Bench support: x[i] = (float)((splitmix64-style hash of (seed, first + i)) >> 40) * 2^-24,
 * uniform in [0,1), written on the device (same values as the oracle's
 * knn_synth_fill for the same seed/first). */
int knn_synth_fill_device(int device, float *dst_dev, long long count, unsigned long long seed,
                          long long first, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KNN_MI355X_H */
