// knn_masked_dev.h — device code the scans over a subset of the rows share (knn_masked.hip: masked top-K and count;
// knn_masked_lists.hip: masked lists and masked top-K beyond 64; DESIGN §4.6 "Over a subset of the rows"): the block's (or the
// wave's) slice by admitted rows, and the walk over the set bits of a slice's mask words (v0's distance of an admitted row is the
// exact scans' own: lane_row_dist2, knn_exact_dev.h).
// The mask words, the bit positions and the row addresses are wave-uniform everywhere here: scalar loads, scalar arithmetic.
#pragma once

#include "knn_exact_dev.h"
#include "knn_mask_split.h"

#include <math.h>

// A wave-uniform 64-bit value made scalar by name.
__device__ __forceinline__ long long masked_uniform(long long v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// The block's rows [r0, r1): slice blockIdx.x of gridDim.x by admitted rows (knn_mask_split.h).  Every lane runs the same search
// over the same prefix and the same words; the results are made scalar by name so that everything derived from them — mask words,
// rows, addresses — stays scalar.
__device__ __forceinline__ void masked_slice(const unsigned *__restrict__ mask, long long n, const u64 *__restrict__ P, int G,
                                             long long &r0, long long &r1)
{
    const u64 S = gridDim.x, b = blockIdx.x;
    r0 = masked_uniform(knn_mask_split_row(mask, n, P, G, S, b));
    r1 = masked_uniform(knn_mask_split_row(mask, n, P, G, S, b + 1ull));
}

// The rows [r0, r1) of wave `wave` of a block of W waves that each take their own slice: slice blockIdx.x * W + wave of
// gridDim.x * W, through the same cut.  wave: wave-uniform (readfirstlane'd by the caller).  The products of the cut stay below
// 2^64: gridDim.x * W < 2^20 and P <= 2^32.
__device__ __forceinline__ void masked_wave_slice(const unsigned *__restrict__ mask, long long n, const u64 *__restrict__ P, int G,
                                                  int W, int wave, long long &r0, long long &r1)
{
    const u64 S = (u64)gridDim.x * (u64)W, b = (u64)blockIdx.x * (u64)W + (u64)wave;
    r0 = masked_uniform(knn_mask_split_row(mask, n, P, G, S, b));
    r1 = masked_uniform(knn_mask_split_row(mask, n, P, G, S, b + 1ull));
}

// Mask word wi with the bits of rows outside [r0, r1) dropped.
__device__ __forceinline__ unsigned masked_clip(unsigned m, long long wi, long long r0, long long r1)
{
    const long long lo = r0 - wi * 32, hi = r1 - wi * 32;   // the word's bits [lo, hi) are rows of the slice
    if (lo > 0)
        m &= ~knn_mask_below(lo < 32 ? (int)lo : 32);
    if (hi < 32)
        m &= knn_mask_below(hi > 0 ? (int)hi : 0);
    return m;
}

// row(i) for every admitted row i of [r0, r1), r1 <= n, ascending: the mask words that hold those rows, four at a time (groups
// aligned to four words), the first and the last cut to the slice.  Where the walk enters a granule that admits nothing — the
// prefix says so — it jumps behind the last of the empty granules that follow, found by a binary search over the prefix: a slice
// that begins in front of a long empty stretch (slice 0 of a mask whose first admitted row is far into the shard) would otherwise
// read that stretch word by word, and the whole launch would wait for it (measured: 0.75 ms for 340 empty granules).  Nothing
// beyond the word of row r1 - 1 is read, no row outside the slice is visited.
template <class F>
__device__ __forceinline__ void masked_walk(const unsigned *__restrict__ mask, const u64 *__restrict__ P, int G, long long r0,
                                            long long r1, F &&row)
{
    const long long wbeg = (r0 >> 5) & ~3ll, wend = (r1 + 31) >> 5;
    for (long long w = wbeg; w < wend; w += 4) {
        if ((w & (KNN_MASK_GRANULE_WORDS - 1)) == 0) {
            const long long g = w / KNN_MASK_GRANULE_WORDS;   // below G: w is a word of the mask
            const u64 here = P[g];
            if (P[g + 1] == here) {
                long long lo = g + 1, hi = G;   // the last granule number whose prefix is still `here` lies in [lo, hi]
                while (lo < hi) {
                    const long long mid = (lo + hi + 1) >> 1;
                    if (P[mid] == here)
                        lo = mid;
                    else
                        hi = mid - 1;
                }
                w = lo * KNN_MASK_GRANULE_WORDS - 4;   // granules g .. lo - 1 admit nothing
                continue;
            }
        }
        unsigned m0, m1, m2, m3;
        if (w + 4 <= wend) {   // wave-uniform addresses -> scalar loads
            m0 = mask[w];
            m1 = mask[w + 1];
            m2 = mask[w + 2];
            m3 = mask[w + 3];
        } else {
            m0 = mask[w];
            m1 = w + 1 < wend ? mask[w + 1] : 0u;
            m2 = w + 2 < wend ? mask[w + 2] : 0u;
            m3 = 0u;
        }
        if (w == wbeg || w + 4 >= wend) {   // the group holds the slice's first or last word
            m0 = masked_clip(m0, w, r0, r1);
            m1 = masked_clip(m1, w + 1, r0, r1);
            m2 = masked_clip(m2, w + 2, r0, r1);
            m3 = masked_clip(m3, w + 3, r0, r1);
        }
        if ((m0 | m1 | m2 | m3) == 0u)
            continue;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            unsigned word = j == 0 ? m0 : j == 1 ? m1 : j == 2 ? m2 : m3;
            const long long row0 = (w + j) << 5;
            while (word) {
                const int bit = __builtin_ctz(word);   // find-first-set, then clear the lowest
                word &= word - 1u;
                row(row0 + bit);
            }
        }
    }
}
