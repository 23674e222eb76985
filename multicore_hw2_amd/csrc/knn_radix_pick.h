// knn_radix_pick.h — one pass's pick of the MSB-first radix select behind knn_index_query_topk_large (DESIGN §4.6 "Top-K beyond
// 64"): the bin walk the pick kernel (knn_select_pick_kernel, knn_select.hip) runs per query, and the host restatement
// (knn_debug_radix_kth; tests/test_topk_large_logic.py) — the kernel runs these same lines.
//
// The select finds, per query, the need-th smallest 64-bit packed key among the candidates, eight bits a pass from the top.
// Before pass p the query holds `prefix` — the digits fixed so far in their places, zero below — and `need` >= 1: the rank of
// the wanted key among the candidates whose bits above the pass's digit equal the prefix's.  The pass's histogram counts those
// candidates by their digit.  The walk finds the digit whose bin holds the need-th of them, fixes it, and lowers need by the
// bins below it.
//
// A query is RESOLVED (need = 0, prefix = its final threshold T: a candidate is in the list exactly when key <= T) when
//   - fewer candidates exist than it needs (pass 0 only): T = KNN_RADIX_ALL, every candidate passes;
//   - the digit's bin holds exactly the `need` left: every key that shares the prefix up to this digit passes, T = the prefix
//     with ones below;
//   - the last pass fixed the last digit: T = the key itself.
// A query left open after the distance word's last pass has its cut inside a class of equal distances — the rows at the K-th
// distance outnumber the places left —, and only then do the index word's passes run.
#pragma once

#define KNN_RADIX_BITS 8
#define KNN_RADIX_BINS 256
#define KNN_RADIX_PASSES 8                       // 64 / KNN_RADIX_BITS
#define KNN_RADIX_DIST_PASSES 4                  // the key's high word: the distance
#define KNN_RADIX_ALL 0x7F7FFFFFFFFFFFFFull      // (largest finite float, largest index): no candidate is above it

__host__ __device__ inline int knn_radix_shift(int pass) { return 64 - KNN_RADIX_BITS * (pass + 1); }

// Does `key` take part in pass `pass` of a query with this prefix: its bits above the pass's digit are the prefix's.
__host__ __device__ inline bool knn_radix_match(unsigned long long key, unsigned long long prefix, int pass)
{
    return pass == 0 || ((key ^ prefix) >> (knn_radix_shift(pass) + KNN_RADIX_BITS)) == 0ull;
}
__host__ __device__ inline unsigned knn_radix_digit(unsigned long long key, int pass)
{
    return (unsigned)(key >> knn_radix_shift(pass)) & (KNN_RADIX_BINS - 1u);
}

// The walk: hist[b * stride] = candidates of the query with digit b.  need >= 1 on entry.  Returns true when the query stays
// open (need >= 1, prefix extended by the digit), false when it is resolved (need = 0, prefix = T).
__host__ __device__ inline bool knn_radix_pick(const unsigned *hist, unsigned long long stride, int pass, unsigned long long &prefix,
                                               unsigned &need)
{
    unsigned long long below = 0ull;   // candidates in the bins under the digit
    unsigned digit = KNN_RADIX_BINS, at = 0u;
    for (unsigned b = 0; b < KNN_RADIX_BINS; ++b) {
        const unsigned c = hist[b * stride];
        if (digit == KNN_RADIX_BINS) {
            if (below + c >= need) {
                digit = b;
                at = c;
            } else {
                below += c;
            }
        }
    }
    if (digit == KNN_RADIX_BINS) {   // fewer candidates than places: all of them
        prefix = KNN_RADIX_ALL;
        need = 0u;
        return false;
    }
    const int shift = knn_radix_shift(pass);
    prefix |= (unsigned long long)digit << shift;
    need -= (unsigned)below;
    if (at == need) {                // the bin fills the places exactly: everything under this prefix
        prefix |= shift ? (1ull << shift) - 1ull : 0ull;
        need = 0u;
        return false;
    }
    if (pass == KNN_RADIX_PASSES - 1) {   // the whole key is fixed
        need = 0u;
        return false;
    }
    return true;
}
