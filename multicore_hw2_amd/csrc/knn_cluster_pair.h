// knn_cluster_pair.h — what a link kernel of the cell-pruned way does with one hit (knn_cluster_routed.hip; include/knn_mi355x.h
// 2n; DESIGN §4.6 "Clusters on the cell-pruned way").  A hit is a pair (own, row): `own` the pass's query, a local row of the
// shard, `row` another local row with a finite E <= max_dist2.  The decision is written ONCE: the two kernels include these
// lines, and the test hook knn_debug_cluster_pair compiles the same lines with the host compiler, so what the tests check without
// a GPU is what the lanes run.
//   both core, row < own     UNITE  — E(row, own) == E(own, row) bit for bit: the pair is a hit of the pass that owns `row` too,
//                                     and the owner of the larger row alone unites;
//   own not core, row core   BORDER — pack_key(E, row) is folded into own's smallest key;
//   everything else          NOTHING (row == own is no hit: the kernels drop it before they come here, and these lines say
//                                     NOTHING for it all the same).
#pragma once

enum { KNN_PAIR_NOTHING = 0, KNN_PAIR_UNITE = 1, KNN_PAIR_BORDER = 2 };

#define KNN_PAIR_FN __host__ __device__ inline   // (as knn_cluster_uf.h: the HIP headers give the two words to host code too)

KNN_PAIR_FN int knn_cluster_pair(bool own_core, bool row_core, long long row, long long own)
{
    if (!row_core || row == own)
        return KNN_PAIR_NOTHING;
    if (own_core)
        return row < own ? KNN_PAIR_UNITE : KNN_PAIR_NOTHING;
    return KNN_PAIR_BORDER;
}
