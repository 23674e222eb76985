// knn_forest_pick.h — the pick and the hook of one Borůvka round of knn_index_self_forest_within (include/knn_mi355x.h 2o;
// knn_forest.hip; DESIGN §4.6 "Minimum spanning forest").  The decision lines are written ONCE, over a policy A that names the
// memory operations they use, as knn_cluster_uf.h's are: the kernels compile them with device atomics (KnnPickDevice), the test
// hook knn_debug_forest_round compiles the same lines with the host compiler's atomics (KnnPickHost), so what the tests check
// without a GPU is what the lanes run.
//
// A round stands on FROZEN labels: labels[i] = the root of row i's component (a depth-1 forest), which nothing writes from the
// flatten to the last emit.  cand[i] = the packed key (E's bits << 32 | row) of the nearest row of ANOTHER component within the
// radius, KNN_KEY_INIT when there is none.  The edge it stands for is (E, lo, hi), lo = min(i, row), hi = max(i, row); edges are
// ordered by that triple, a strict total order, so every component has ONE smallest outgoing edge and the picks of a round can
// close no cycle.
//   offer 1   every row with a candidate: atomic min of (E << 32 | lo) on pick1[labels[i]];
//   offer 2   every row whose (E, lo) is the one its root kept: atomic min of hi on pick2[labels[i]].  Only a root's slots ever
//             receive an offer, so "pick1[x] is not KNN_KEY_INIT" says "x is a root with a pick".
//   emit      every root with a pick appends its edge through the one cursor — unless the component at the OTHER end picked
//             the SAME edge and this one holds `hi`: of the two only the component that holds `lo` appends.  Every forest edge
//             is so stored exactly once.  Reads labels and picks alone.
//   hook      every root with a pick: knn_uf_unite(lo, hi).  This is the first step that writes labels, so it is a launch of its
//             own behind the emit (on the host: behind a join): the emit's "which component is at the other end" needs the frozen
//             labels of both ends.
// The atomic minima and unite are idempotent and commute: the picks, the set of edges and the components after the round depend
// neither on the order of the rows nor on how many lanes or host threads share them.  The ORDER of the stored edges does.
#pragma once

#include "knn_cluster_uf.h"

#define KNN_FOREST_NONE 0x7F80000000000000ull   // KNN_KEY_INIT: no candidate, no pick
#define KNN_FOREST_NO_HI 0xFFFFFFFFu

#if defined(__HIP__)   // (a translation unit compiled as HIP: the kernels')
struct KnnPickDevice {
    typedef KnnUfDevice Uf;
    static __device__ __forceinline__ void min64(unsigned long long *p, unsigned long long v)
    {
        __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void min32(unsigned *p, unsigned v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ unsigned add32(unsigned *p, unsigned v)
    {
        return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ unsigned swap32(unsigned *p, unsigned v)
    {
        return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ unsigned load32(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
#endif

// The host's: the compiler's atomic builtins, so several host threads may share a round's rows as the lanes do.
struct KnnPickHost {
    typedef KnnUfHost Uf;
    static __host__ __device__ inline void min64(unsigned long long *p, unsigned long long v)
    {
        unsigned long long seen = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (v < seen && !__atomic_compare_exchange_n(p, &seen, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
        }
    }
    static __host__ __device__ inline void min32(unsigned *p, unsigned v)
    {
        unsigned seen = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (v < seen && !__atomic_compare_exchange_n(p, &seen, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
        }
    }
    static __host__ __device__ inline unsigned add32(unsigned *p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
    static __host__ __device__ inline unsigned swap32(unsigned *p, unsigned v) { return __atomic_exchange_n(p, v, __ATOMIC_RELAXED); }
    static __host__ __device__ inline unsigned load32(const unsigned *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
};

#define KNN_FOREST_FN __host__ __device__ inline   // (as knn_cluster_uf.h)

// Row i's candidate as the edge it stands for.
struct KnnForestEdge {
    unsigned long long elo;   // E's bits << 32 | lo
    unsigned hi;
};
KNN_FOREST_FN KnnForestEdge knn_forest_edge(unsigned i, unsigned long long cand)
{
    const unsigned row = (unsigned)cand;
    KnnForestEdge e;
    e.elo = (cand & 0xFFFFFFFF00000000ull) | (unsigned long long)(row < i ? row : i);
    e.hi = row < i ? i : row;
    return e;
}

// labels[i] = root(i), in place, by the walk that writes nothing else: every store is "replace a parent by an ancestor", so every
// walk that passes through i afterwards still ends at the same root (knn_cluster_flatten_kernel).  The first step of every round
// and, once more, the LAST step of the call: a hook re-parents only the larger root, so behind the last round that added an edge
// the other rows of that component still carry the old root.
template <class A>
KNN_FOREST_FN void knn_forest_flatten(int *labels, long long i)
{
    const int p = A::Uf::load(&labels[i]);
    if (p != (int)i)
        A::Uf::store(&labels[i], knn_uf_root<typename A::Uf>(labels, p));
}

// The slots of the round start empty.  (The flatten's second half: every row, root or not.)
KNN_FOREST_FN void knn_forest_clear(unsigned long long *pick1, unsigned *pick2, long long i)
{
    pick1[i] = KNN_FOREST_NONE;
    pick2[i] = KNN_FOREST_NO_HI;
}

template <class A>
KNN_FOREST_FN void knn_forest_offer1(const int *labels, const unsigned long long *cand, unsigned long long *pick1, long long i)
{
    const unsigned long long c = cand[i];
    if (c != KNN_FOREST_NONE)
        A::min64(&pick1[labels[i]], knn_forest_edge((unsigned)i, c).elo);
}

template <class A>
KNN_FOREST_FN void knn_forest_offer2(const int *labels, const unsigned long long *cand, const unsigned long long *pick1,
                                     unsigned *pick2, long long i)
{
    const unsigned long long c = cand[i];
    if (c == KNN_FOREST_NONE)
        return;
    const KnnForestEdge e = knn_forest_edge((unsigned)i, c);
    const int root = labels[i];
    if (pick1[root] == e.elo)
        A::min32(&pick2[root], e.hi);
}

// Root i's pick goes to the list when it is this component's to store; true: it did.  count[0]: the cursor (nothing is stored at
// or beyond entry n: a forest has fewer edges, the test is a guard); count[1]: the rounds that added an edge, raised by the lane
// that finds *raised still 0 — the word that also opens the next round's gate.
template <class A>
KNN_FOREST_FN bool knn_forest_emit(const int *labels, const unsigned long long *pick1, const unsigned *pick2, long long i, long long n,
                                   unsigned long long *edge_keys, unsigned *edge_hi, unsigned *count, unsigned *raised)
{
    const unsigned long long elo = pick1[i];
    if (elo == KNN_FOREST_NONE)
        return false;
    const unsigned lo = (unsigned)elo, hi = pick2[i];
    const bool holds_lo = labels[lo] == (int)i;
    const int other = holds_lo ? labels[hi] : labels[lo];
    if (!holds_lo && pick1[other] == elo && pick2[other] == hi)   // the same edge from both ends: the other end stores it
        return false;
    const unsigned e = A::add32(&count[0], 1u);
    if ((long long)e < n) {
        edge_keys[e] = elo;
        edge_hi[e] = hi;
    }
    if (A::load32(raised) == 0u && A::swap32(raised, 1u) == 0u)
        (void)A::add32(&count[1], 1u);
    return true;
}

template <class A>
KNN_FOREST_FN void knn_forest_hook(int *parent, const unsigned long long *pick1, const unsigned *pick2, long long i)
{
    const unsigned long long elo = pick1[i];
    if (elo != KNN_FOREST_NONE)
        (void)knn_uf_unite<typename A::Uf>(parent, (int)(unsigned)elo, (int)pick2[i]);
}
