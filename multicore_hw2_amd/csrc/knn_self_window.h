// knn_self_window.h — how a block of the self-scans (knn_self.hip; knn_index_self_topk, knn_index_self_count_within,
// knn_index_self_list_within; DESIGN §4.6 "About the shard's own rows") cuts its slice of the shard around the rows that can be some
// lane's OWN row.  The scan kernels run these lines per block, knn_debug_self_ranges (tests/test_self_logic.py) runs them on the host.
//
// A block's 64 lanes hold the queries of local rows [w0, w1), w1 <= w0 + 64: only those rows can be the row a lane must not meet.
// The slice [i0, i1) is cut at the window's two ends, each clamped into the slice:
//     before = [i0, c0),   inside = [c0, c1),   after = [c1, i1),      c0 = clamp(w0, i0, i1),  c1 = clamp(w1, c0, i1).
// From the clamps: i0 <= c0 <= c1 <= i1, so the three ranges are disjoint, ascending and their union is exactly the slice; every
// row of the slice that lies in the window is in `inside` and no other row is (c0 >= w0 or c0 = i1; c1 <= w1 or c1 = c0); a window
// that misses the slice, or an empty one (w1 <= w0), leaves `inside` empty; an empty slice (i1 <= i0) gives three empty ranges at i0.
#pragma once

// out = {before's first and end, inside's first and end, after's first and end}
__host__ __device__ inline void knn_self_ranges(long long i0, long long i1, long long w0, long long w1, long long out[6])
{
    if (i1 < i0)
        i1 = i0;
    const long long c0 = w0 < i0 ? i0 : (w0 > i1 ? i1 : w0);
    const long long c1 = w1 < c0 ? c0 : (w1 > i1 ? i1 : w1);
    out[0] = i0;
    out[1] = c0;
    out[2] = c0;
    out[3] = c1;
    out[4] = c1;
    out[5] = i1;
}
