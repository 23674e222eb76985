// knn_mask_split.h — how the masked scans (knn_masked.hip; knn_index_query_topk_masked, knn_index_count_within_masked; DESIGN §4.6
// "Over a subset of the rows") cut a shard into slices: by ADMITTED rows, not by rows.  The scan kernels run these lines per block,
// knn_debug_mask_split and knn_debug_mask_split_rows (tests/test_masked_logic.py) run the same lines on the host.
//
// A granule is KNN_MASK_GRANULE_ROWS = 1024 rows = 32 mask words.  P[0 .. G] is the exclusive prefix of the granules' admitted rows
// (P[0] = 0, P[G] = T, non-decreasing).  Slice b of S begins where need_b = ceil(b T / S) admitted rows lie behind — for whole
// numbers A, A * S >= b * T exactly when A >= need_b.  The cut is made in two steps.
//
// 1. Granules (knn_mask_split_first).  g_b = min{ g in 0 .. G : P[g] * S >= b * T }   (b = 0 .. S; the set holds G because
//    P[G] = T), found by a binary search over the non-decreasing P.  From the definition:
//      - g_0 = 0 and g_b <= g_{b+1} (the condition only gets harder with b);
//      - g_S = the first granule with P[g] = T: no admitted row lies at or behind it, so every admitted row is in exactly one of
//        the ranges [g_b, g_{b+1});
//      - P[g_{b+1} - 1] * S < (b + 1) T and P[g_b] * S >= b T: a range holds fewer than T / S admitted rows plus those of its
//        last granule;
//      - T = 0: every g_b = 0, every range is empty.
// 2. Rows (knn_mask_split_row).  Cutting at granules alone leaves a slice no smaller than a granule, and a mask that admits one
//    contiguous range of T rows would keep T / 1024 blocks busy whatever S is (measured so: profiles/masked_timing.txt).  So the
//    cut is refined inside the one granule it falls into, g_b - 1: with A(r) the admitted rows before row r,
//    r_b = min{ r in 0 .. n : A(r) >= need_b } lies in ((g_b - 1) * 1024, g_b * 1024]; the granule's 32 words find the word, the
//    word's 32 bits the row.  Slice b is the rows [r_b, r_{b+1}): r_0 = 0, the r_b do not decrease, every admitted row lies in
//    exactly one slice, a slice holds need_{b+1} - need_b admitted rows — floor(T / S) or one more — and all are empty when T = 0.
// Bits of the last word at and beyond the shard's rows are dropped wherever a word is read (knn_mask_word).
// The products stay below 2^64: P <= rows <= 2^32 and S < 2^16 (the host refuses more before anything is launched).
#pragma once

#define KNN_MASK_GRANULE_ROWS 1024
#define KNN_MASK_GRANULE_WORDS 32   // KNN_MASK_GRANULE_ROWS / 32

// Word w of the mask over n rows with the bits at and beyond n dropped; 0 beyond the mask's (n + 31) / 32 words.
__host__ __device__ inline unsigned knn_mask_word(const unsigned *mask, long long n, long long w)
{
    const long long nwords = (n + 31) >> 5;
    if (w >= nwords)
        return 0u;
    const unsigned tail = (unsigned)(n & 31);
    const unsigned v = mask[w];
    return tail && w == nwords - 1 ? v & ((1u << tail) - 1u) : v;
}

// The bits of a word below position p (0 .. 32).
__host__ __device__ inline unsigned knn_mask_below(int p) { return p >= 32 ? 0xFFFFFFFFu : (1u << p) - 1u; }

__host__ __device__ inline long long knn_mask_split_first(const unsigned long long *P, long long G, unsigned long long S,
                                                          unsigned long long b)
{
    const unsigned long long want = b * P[G];
    long long lo = 0, hi = G;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (P[mid] * S >= want)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// The first row of slice b (b = 0 .. S).  A only grows along the words of granule g_b - 1 and along the bits of a word, so the
// words (bits) that still lie before the cut are the leading ones: they are counted, without a branch on what a word holds — and
// with products, not the quotient need_b: a 64-bit division on the device goes through floating point.
__host__ __device__ inline long long knn_mask_split_row(const unsigned *mask, long long n, const unsigned long long *P, long long G,
                                                        unsigned long long S, unsigned long long b)
{
    const long long g = knn_mask_split_first(P, G, S, b);
    if (g == 0)
        return 0;
    const unsigned long long want = b * P[G];
    const long long w0 = (g - 1) * KNN_MASK_GRANULE_WORDS;
    unsigned long long before = P[g - 1];   // A at word w0: before * S < want, g being the least
    unsigned long long cut_before = before;
    unsigned cut_word = 0u;
    long long ahead = 0;   // words of the granule that begin before the cut: the last of them holds it
    for (int j = 0; j < KNN_MASK_GRANULE_WORDS; ++j) {
        const unsigned word = knn_mask_word(mask, n, w0 + j);
        const bool open = before * S < want;
        ahead += open ? 1 : 0;
        cut_before = open ? before : cut_before;
        cut_word = open ? word : cut_word;
        before += (unsigned)__builtin_popcount(word);
    }
    int p = 0;             // the least bit position of that word with enough admitted rows behind it: 1 .. 32
    for (int j = 0; j < 32; ++j)
        p += (cut_before + (unsigned)__builtin_popcount(cut_word & knn_mask_below(j))) * S < want ? 1 : 0;
    const long long r = (w0 + ahead - 1) * 32 + p;
    return r < n ? r : n;
}
