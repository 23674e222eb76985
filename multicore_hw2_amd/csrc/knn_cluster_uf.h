// knn_cluster_uf.h — the lock-free union-find of knn_index_self_cluster_within (include/knn_mi355x.h 2m; knn_cluster.hip, the grid
// link kernel in knn_grid.hip; DESIGN §4.6 "Clusters of the radius graph").  find and unite are written ONCE, over a policy A that
// names the three memory operations they use: the kernels compile them with device atomics (KnnUfDevice below), the test hook
// knn_debug_cluster_unite compiles the same lines with the host compiler's atomics (KnnUfHost: what std::atomic<int> is made of), so what the tests
// check without a GPU is what the lanes run.
//
// The forest: parent[x] for every member x (a core row), in an int array that also holds other values (-1) for non-members, which
// nobody ever starts from or reaches.  INVARIANT: parent[x] <= x, always, for every member; x is a root iff parent[x] == x.  Every
// value ever stored into parent[x] is x itself (at the start) or a member of x's set that is smaller than x: an ancestor of x at
// the time of the store, and ancestors stay ancestors — a root is only ever hooked under another root, a non-root's parent is only
// ever replaced by one of its own ancestors.  So the root of a finished forest is the smallest member of its set.
//
// Memory operations: every read of parent is an atomic relaxed load (the compiler must not keep one in a register across a loop;
// on the device it is served by the coherent level, never by a lane's stale line), the path-halving write is an atomic relaxed
// store, and the hook is ONE compare-and-swap on the larger root's own slot.  Nothing orders anything else: the only state is the
// forest, and every intermediate forest is a valid one.
//
// NO LANE EVER WAITS FOR ANOTHER.  There is no lock and no flag to spin on; termination needs no forward-progress guarantee
// between lanes, only that a lane's own instructions retire:
//   find:   every turn either returns or moves x to parent[parent[x]] < parent[x] < x — x descends strictly, at most x turns.
//           (The halving store replaces a NON-root's parent — parent[x] != x was just read, and a non-root never becomes a root
//           again — with that grandparent: an ancestor.  It cannot collide with a hook, which swaps a slot that holds its own
//           number.)
//   unite:  finds both roots, hooks the LARGER under the smaller with the compare-and-swap "parent[hi]: hi -> lo".  It fails only
//           when parent[hi] was no longer hi — some other lane's hook of hi succeeded — and then returns the value it saw there,
//           an ancestor of hi below hi.  The retry starts from (lo, that ancestor): the larger of the two roots it finds next is
//           below hi.  So hi descends strictly from try to try, whatever the other lanes do or do not do, and the loop ends
//           after at most hi tries — without ever reading a slot again to see whether "it has changed yet".
// unite is idempotent and commutes with every other unite: the sets after any interleaving of a multiset of unites are the
// connected components of its pairs, and the roots their smallest members.  The forest's SHAPE depends on the timing; the
// answer read from it (find of every member) does not.
#pragma once

// The device's operations: agent scope — every lane of the launch, whichever CU it runs on.
#if defined(__HIP__)   // (a translation unit compiled as HIP: the kernels')
struct KnnUfDevice {
    static __device__ __forceinline__ int load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    // parent[*p]: expect -> want; returns what the slot held (== expect: the swap happened)
    static __device__ __forceinline__ int cas(int *p, int expect, int want)
    {
        (void)__hip_atomic_compare_exchange_strong(p, &expect, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
};
#endif

// The host's: the same three through the compiler's atomic builtins (what std::atomic<int> compiles to), so several host threads
// may run knn_uf_unite on one array as the lanes do.
struct KnnUfHost {
    static __host__ __device__ inline int load(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static __host__ __device__ inline void store(int *p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
    static __host__ __device__ inline int cas(int *p, int expect, int want)
    {
        (void)__atomic_compare_exchange_n(p, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expect;
    }
};

#define KNN_UF_FN __host__ __device__ inline   // (as knn_self_window.h: the HIP headers give the two words to host code too)

// The root of member x, with path halving.
template <class A>
KNN_UF_FN int knn_uf_find(int *parent, int x)
{
    for (;;) {
        const int p = A::load(&parent[x]);
        if (p == x)
            return x;
        const int g = A::load(&parent[p]);
        if (g == p)
            return p;
        A::store(&parent[x], g);   // x is no root (p != x): its parent becomes its grandparent, an ancestor
        x = g;
    }
}

// The root of member x by a walk that writes nothing: for a pass that stores its results into the array it reads
// (knn_cluster_flatten_kernel).  x descends strictly.
template <class A>
KNN_UF_FN int knn_uf_root(const int *parent, int x)
{
    for (;;) {
        const int p = A::load(&parent[x]);
        if (p == x)
            return x;
        x = p;
    }
}

// Members a and b end in one set; returns a member of that set that was its root at some moment during the call (the smaller of
// the two roots last found) — what a lane caches as "my root, as far as I know".
template <class A>
KNN_UF_FN int knn_uf_unite(int *parent, int a, int b)
{
    for (;;) {
        const int ra = knn_uf_find<A>(parent, a), rb = knn_uf_find<A>(parent, b);
        if (ra == rb)
            return ra;
        const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        const int seen = A::cas(&parent[hi], hi, lo);
        if (seen == hi)
            return lo;
        a = lo;      // hi was hooked by another lane meanwhile: go on from what it hangs under now (seen < hi)
        b = seen;
    }
}
