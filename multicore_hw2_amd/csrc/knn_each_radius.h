// knn_each_radius.h — the radius of ONE query of a call that carries a radius per query (include/knn_mi355x.h 2j; DESIGN §4.6
// "A radius per query"): knn_index_count_within_each, knn_index_list_within_each and their self forms.  The kernels that prune or
// stop by the radius — the grid walks' stop clause, the cell-pruned way's preparation — run these lines per query,
// knn_debug_each_radius (tests/test_each_logic.py) runs them on the host.
//
// A row is a hit for query j when its v0 distance E is finite, E <= r_j and E <= cap: two plain fp32 compares, equality inside.
// E >= 0 always, so a query whose radius is negative or NaN has no hit whatever the rows are — it "has no candidates" — and every
// other query's hits are exactly the rows with E <= min(r_j, cap), its bound.  -0 >= 0 holds: -0 has candidates, and its bound
// compares as 0 everywhere a bound is used.  cap >= 0 and not NaN (the entry points refuse anything else).
#pragma once

// r_j >= 0 (NaN fails): the query can have a hit
__host__ __device__ inline bool knn_each_has(float radius)
{
    return radius >= 0.0f;
}

// The radius the query's hits all lie within: what pruning and stop rules use in the scalar calls' max_dist2's place.  Only
// meaningful when knn_each_has(radius).
__host__ __device__ inline float knn_each_bound(float radius, float cap)
{
    return radius <= cap ? radius : cap;
}
