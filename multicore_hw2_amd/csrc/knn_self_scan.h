// knn_self_scan.h — the row loops of the exact self-scans (knn_self.hip: top-K, count, list and their forms; knn_cluster.hip: the
// link sweep of knn_index_self_cluster_within).  One wave per block, lanes = queries that are rows of the shard, rows as
// wave-uniform scalar loads, v0's arithmetic (lane_row_dist2, knn_exact_dev.h); the block cuts its slice around the only rows that
// can be some lane's own (knn_self_window.h).  knn_self.hip's head describes the kernels built on them.
#pragma once

#include "knn_exact_dev.h"
#include "knn_self_window.h"

// hit(acc, row) for the next `count` rows but — WIN — the lane's own: the one row-loop body of the three scans.  r: the first of
// them, row: its local number's low word (what a key carries and what `own` is compared with); both are left behind the last.
// The counter is 32-bit: the loop's test is scalar arithmetic.
template <int KC, bool WIN, class Hit>
__device__ __forceinline__ void self_rows(const float (&qv)[KC > 0 ? 16 * KC : 1], const float *__restrict__ qp,
                                          const float *__restrict__ &r, int k, unsigned &row, unsigned count, unsigned own, Hit &&hit)
{
    for (unsigned c = 0; c < count; ++c, ++row, r += k) {
        const float acc = lane_row_dist2<KC>(qv, qp, r, k);
        if (!WIN || row != own)
            hit(acc, row);
    }
}

// The block's slice [i0, i1) around its window [w0, w1) (a slice is shorter than 2^32 rows: the launchers see to it): the rows
// before the window, inside it and after it, in that order, through two copies of the loop — the plain one and the window's.
template <int KC, class Hit>
__device__ __forceinline__ void self_scan(const float (&qv)[KC > 0 ? 16 * KC : 1], const float *__restrict__ qp,
                                          const float *__restrict__ R, int k, long long i0, long long i1, long long w0, long long w1,
                                          unsigned own, Hit &&hit)
{
    long long rg[6];
    knn_self_ranges(i0, i1, w0, w1, rg);
    const unsigned n0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rg[1] - rg[0]));
    const unsigned n1 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rg[3] - rg[2]));
    const unsigned n2 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rg[5] - rg[4]));
    const float *__restrict__ r = R + (size_t)i0 * k;
    unsigned row = (unsigned)i0;
#pragma clang loop unroll(disable)
    for (int t = 0; t < 3; ++t) {
        if (t == 1)
            self_rows<KC, true>(qv, qp, r, k, row, n1, own, hit);
        else
            self_rows<KC, false>(qv, qp, r, k, row, t ? n2 : n0, own, hit);
    }
}

// The same cut through ONE copy of the loop: `win` — the range is the window's — is wave-uniform, so outside the window the own-row
// compare is skipped by a scalar branch.  For a scan whose hit path is long (the list's reserve-and-store, the link sweep's
// unite): two copies of it cost registers (17-19 VGPRs in the list form, a wave of occupancy at KC 6), one does not.
template <int KC, class Hit>
__device__ __forceinline__ void self_scan_one(const float (&qv)[KC > 0 ? 16 * KC : 1], const float *__restrict__ qp,
                                              const float *__restrict__ R, int k, long long i0, long long i1, long long w0, long long w1,
                                              unsigned own, Hit &&hit)
{
    long long rg[6];
    knn_self_ranges(i0, i1, w0, w1, rg);
    const unsigned n0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rg[1] - rg[0]));
    const unsigned n1 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rg[3] - rg[2]));
    const unsigned n2 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rg[5] - rg[4]));
    const float *__restrict__ r = R + (size_t)i0 * k;
    unsigned row = (unsigned)i0;
#pragma clang loop unroll(disable)
    for (int t = 0; t < 3; ++t) {
        const bool win = t == 1;
        const unsigned count = t == 0 ? n0 : t == 1 ? n1 : n2;
        for (unsigned c = 0; c < count; ++c, ++row, r += k) {
            const float acc = lane_row_dist2<KC>(qv, qp, r, k);
            hit(acc, row, !(win && row == own));
        }
    }
}
