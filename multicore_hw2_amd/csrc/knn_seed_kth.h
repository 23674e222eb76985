// knn_seed_kth.h — the K-th smallest seed score of a top-K batch on the cell-pruned path (knn_cells_prep_kernel<.., TK = true>),
// and its host restatement (knn_debug_seed_kth; tests/test_cells_topk_logic.py).
//
// The rule.  The prep kernel scores real layout positions of the query's seed cells; for top-K it hands
// knn_threshold the K-th smallest FINITE score u_(K) among scores of DISTINCT positions instead of the smallest.  Why that is
// valid: a padding position and a row outside the robust box carry a +INF norm, so K finite scores of K distinct positions are
// K distinct real rows, each scoring <= u_(K).  knn_threshold(u) bounds the score of every row whose v0 distance is <= that of
// the row scoring u, and it is non-decreasing in u; the K-th smallest true distance D_(K) is <= the largest distance among those
// K rows, so every true top-K row (ties at D_(K) included) scores <= thr(u_(K)), has a real distance <= Dup(u_(K)), and lies in
// a cell with LB <= Dup.  Leaving a position OUT of the selection can only raise u_(K): every omission below is safe.
//
// Per-row scores, not per-(tile, half) group minima.  Both are valid inputs (groups are disjoint); a group minimum stands for 16
// rows with one score, so the K-th smallest of ~64 group minima is about the 16 K-th smallest row score — at K 64 that is every
// seed row, and the threshold admits ~16 times the rows.  Per-row costs a 64-lane sorting network per tile in a kernel whose
// top-K call is worth milliseconds.
//
// Mechanism.  Every column of the seed MFMA is the same query: lane c (c < 16) of either half holds, in accumulator c, the score
// of one of the tile's 32 rows — lanes 0..15 and 32..47 pick accumulator (lane & 15), the other lanes hold "none".  A wave keeps
// the 64 smallest keys it has seen, sorted ascending over its lanes (K <= 64): a tile's 64 lane values are sorted by a bitonic
// network and merged in (min against the reversed list leaves the 64 smallest as a bitonic sequence; six more stages sort it).
// A tile none of whose scores is below the wave's current K-th is skipped.  The block merges its waves' lists the same way.
// Keys are order-preserving 32-bit images of the scores; a score that is not finite (padding, out-of-box rows) is "none" = ~0.
// Fewer than K finite scores: the strided sample of 64 tiles over the whole layout is merged in, MINUS the tiles that lie in a
// seed cell (their positions may have been counted already); still fewer: +INF, and the batch raises KNN_CTL_FALLBACK.
#pragma once

#include <math.h>
#include <string.h>

#define KNN_SEED_NONE 0xFFFFFFFFu

__host__ __device__ inline unsigned knn_seed_key(float s)
{
    if (!(fabsf(s) < INFINITY))   // +-INF, NaN: not a real row's score
        return KNN_SEED_NONE;
    unsigned b;
    memcpy(&b, &s, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float knn_seed_score(unsigned key)
{
    if (key == KNN_SEED_NONE)
        return INFINITY;
    const unsigned b = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
    float f;
    memcpy(&f, &b, 4);
    return f;
}
// One compare-exchange of the bitonic network: what `lane` keeps of (its value, its partner's — lane ^ j) in the stage (kk, j).
__host__ __device__ inline unsigned knn_seed_cx(unsigned mine, unsigned other, int lane, int kk, int j)
{
    const bool up = (lane & kk) == 0, lower = (lane & j) == 0;
    const unsigned lo = other < mine ? other : mine, hi = other < mine ? mine : other;
    return lower == up ? lo : hi;
}
// The lane of a tile's 64 that holds a row score: accumulator (lane & 15) of lanes 0..15 (half 0) and 32..47 (half 1).
__host__ __device__ inline bool knn_seed_lane_holds_row(int lane)
{
    return (lane & 16) == 0;
}

#ifdef __HIPCC__
__device__ __forceinline__ unsigned seed_sort64(unsigned v, int lane)
{
#pragma unroll
    for (int kk = 2; kk <= 64; kk <<= 1) {
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1)
            v = knn_seed_cx(v, (unsigned)__shfl_xor((int)v, j, 64), lane, kk, j);
    }
    return v;
}
// a, b: sorted ascending over the lanes -> the 64 smallest of both, sorted ascending
__device__ __forceinline__ unsigned seed_merge64(unsigned a, unsigned b, int lane)
{
    const unsigned br = (unsigned)__shfl((int)b, 63 - lane, 64);
    unsigned v = br < a ? br : a;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1)
        v = knn_seed_cx(v, (unsigned)__shfl_xor((int)v, j, 64), lane, 64, j);
    return v;
}
#endif

// ---- host restatement: the same network and the same rule, lanes as array elements ----------------------------------------
static inline void knn_seed_host_sort64(unsigned v[64])
{
    for (int kk = 2; kk <= 64; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            unsigned o[64];
            for (int l = 0; l < 64; ++l)
                o[l] = v[l ^ j];
            for (int l = 0; l < 64; ++l)
                v[l] = knn_seed_cx(v[l], o[l], l, kk, j);
        }
}
static inline void knn_seed_host_merge64(unsigned a[64], const unsigned b[64])
{
    for (int l = 0; l < 64; ++l)
        a[l] = b[63 - l] < a[l] ? b[63 - l] : a[l];
    for (int j = 32; j > 0; j >>= 1) {
        unsigned o[64];
        for (int l = 0; l < 64; ++l)
            o[l] = a[l ^ j];
        for (int l = 0; l < 64; ++l)
            a[l] = knn_seed_cx(a[l], o[l], l, 64, j);
    }
}
// One wave's collector over tiles [t0, t1) of `scores` (32 per tile; score (half h, accumulator c) = scores[32 t + 16 h + c]).
static inline void knn_seed_host_collect(const float *scores, int t0, int t1, int K, unsigned cur[64])
{
    for (int l = 0; l < 64; ++l)
        cur[l] = KNN_SEED_NONE;
    for (int t = t0; t < t1; ++t) {
        unsigned v[64];
        bool any = false;
        for (int l = 0; l < 64; ++l) {
            v[l] = knn_seed_lane_holds_row(l) ? knn_seed_key(scores[32 * t + 16 * (l >> 5) + (l & 15)]) : KNN_SEED_NONE;
            any = any || v[l] < cur[K - 1];
        }
        if (!any)
            continue;
        knn_seed_host_sort64(v);
        knn_seed_host_merge64(cur, v);
    }
}
// The block's value for knn_threshold: seed[32 nseed_tiles] scored by `pw` waves (wave w: tiles w, w + pw, ... — any deal gives
// the same multiset), then, with fewer than K finite, wide[32 nwide_tiles] (the strided sample, tiles inside seed cells already
// taken out by the caller) merged in.  +INF: fewer than K finite scores in all.
static inline float knn_seed_kth_host(const float *seed, int nseed_tiles, const float *wide, int nwide_tiles, int K, int pw)
{
    unsigned all[64], cur[64];
    for (int l = 0; l < 64; ++l)
        all[l] = KNN_SEED_NONE;
    for (int w = 0; w < pw; ++w) {
        const int per = (nseed_tiles + pw - 1) / pw;
        const int t0 = w * per < nseed_tiles ? w * per : nseed_tiles, t1 = (w + 1) * per < nseed_tiles ? (w + 1) * per : nseed_tiles;
        knn_seed_host_collect(seed, t0, t1, K, cur);
        knn_seed_host_merge64(all, cur);
    }
    if (all[K - 1] == KNN_SEED_NONE && nwide_tiles > 0)
        for (int w = 0; w < pw; ++w) {
            const int per = (nwide_tiles + pw - 1) / pw;
            const int t0 = w * per < nwide_tiles ? w * per : nwide_tiles, t1 = (w + 1) * per < nwide_tiles ? (w + 1) * per : nwide_tiles;
            knn_seed_host_collect(wide, t0, t1, K, cur);
            knn_seed_host_merge64(all, cur);
        }
    return knn_seed_score(all[K - 1]);
}
