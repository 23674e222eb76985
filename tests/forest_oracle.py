"""numpy restatement of knn_index_self_forest_within (include/knn_mi355x.h 2o) — test infrastructure, numpy only.

The definition, word for word: vertices are the rows; rows i < j are joined when their v0 distance E(i, j) is finite and <=
max_dist2; edges are ordered by (E's bits as unsigned, i, j); the minimum spanning forest is the set Kruskal accepts when it takes
the edges in that order; labels[i] = the smallest row of i's component.  The pairs are tests/cluster_oracle._pairs' — EVERY pair
decision goes through tests.topk_oracle.v0_dist2 — and Kruskal is a plain union-find over them.

Also here, for the tests that drive knn_debug_forest_round without a GPU: the candidates of one Borůvka round from frozen labels
(candidates), and the loop over rounds (run_rounds)."""
import numpy as np

from tests.cluster_oracle import _pairs

KEY_INIT = np.uint64(0x7F80000000000000)


def rounds_of(n):
    """ROUNDS(n) = max(1, ceil(log2 n))."""
    return max(1, (int(n) - 1).bit_length())


def pairs(R, k, max_dist2):
    """(a, b, bits) of cluster_oracle._pairs: every ordered pair a != b with a finite v0 distance <= max_dist2."""
    return _pairs(R, k, max_dist2)


def forest_of_pairs(n, a, b, bits):
    """dict(lo, hi int64 [edges], bits uint32 [edges] — sorted ascending by (bits, lo, hi) —, labels int32 [n])."""
    sel = a < b
    lo, hi, e = a[sel], b[sel], bits[sel]
    order = np.lexsort((hi, lo, e))
    lo, hi, e = lo[order], hi[order], e[order]
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    keep = []
    for t, (i, j) in enumerate(zip(lo.tolist(), hi.tolist())):
        ri, rj = find(i), find(j)
        if ri != rj:
            if ri < rj:
                parent[rj] = ri
            else:
                parent[ri] = rj
            keep.append(t)
    keep = np.asarray(keep, dtype=np.int64)
    labels = np.array([find(x) for x in range(n)], dtype=np.int32)
    return dict(lo=lo[keep], hi=hi[keep], bits=e[keep], labels=labels)


def forest(R, k, max_dist2):
    R = np.asarray(R, dtype=np.float32).reshape(-1, k)
    return forest_of_pairs(R.shape[0], *pairs(R, k, max_dist2))


def edge_table(keys, his):
    """The device call's edges (keys uint64 = bits << 32 | lo, his uint32) as rows (bits, lo, hi) sorted ascending."""
    keys = np.asarray(keys, dtype=np.uint64)
    his = np.asarray(his, dtype=np.uint32).astype(np.int64)
    t = np.stack([(keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), his], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))] if len(t) else t.reshape(0, 3)


def want_table(w):
    """The oracle's edges in edge_table's form."""
    return np.stack([w["bits"].astype(np.int64), w["lo"].astype(np.int64), w["hi"].astype(np.int64)], axis=1).reshape(-1, 3)


def roots_of(parent):
    """The root of every row of a forest with parent[x] <= x."""
    lab = np.asarray(parent, dtype=np.int64).copy()
    while True:
        jumped = lab[lab]
        if (jumped == lab).all():
            return lab
        lab = jumped


def candidates(n, a, b, bits, labels):
    """cand uint64 [n]: per row the smallest key (bits << 32 | row) of a row of ANOTHER component among its pairs, KEY_INIT: none."""
    cand = np.full(n, KEY_INIT, dtype=np.uint64)
    sel = labels[a] != labels[b]
    keys = (bits[sel].astype(np.uint64) << np.uint64(32)) | b[sel].astype(np.uint64)
    np.minimum.at(cand, a[sel], keys)
    return cand


def run_rounds(round_fn, n, a, b, bits, threads=1, limit=64):
    """Borůvka through round_fn (multicore_hw2_amd.debug_forest_round) until a round adds nothing: dict(table (bits, lo, hi) sorted,
    raw = the number of edges stored, parent, rounds = count[1], calls)."""
    parent = np.arange(n, dtype=np.int32)
    keys = np.full(max(n, 1), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    his = np.full(max(n, 1), 0xDEADBEEF, dtype=np.uint32)
    count = np.zeros(2, dtype=np.uint32)
    calls = 0
    while calls < limit:
        cand = candidates(n, a, b, bits, roots_of(parent))
        added = round_fn(parent, cand, keys[:n] if n else keys[:0], his[:n] if n else his[:0], count, threads=threads)
        calls += 1
        if added == 0:
            break
    e = int(count[0])
    assert e <= max(n - 1, 0)
    assert (keys[e:] == np.uint64(0xDEADBEEFDEADBEEF)).all() and (his[e:] == np.uint32(0xDEADBEEF)).all()
    return dict(table=edge_table(keys[:e], his[:e]), raw=e, parent=parent, rounds=int(count[1]), calls=calls)


def paired(levels, k, factor, rng):
    """2^levels rows paired at every level, in shuffled row order: bit l of a row's number moves it by factor^l along axis l % k, so
    the gap between the two halves of a level-l group (about factor^l) outgrows everything inside them.  Every Borůvka round then
    joins each component to its sibling alone — the components halve EXACTLY, and all ROUNDS(n) = levels rounds add an edge.
    Coordinates are integers below 2^24: exact in fp32."""
    n = 1 << levels
    R = np.zeros((n, k), dtype=np.float64)
    for level in range(levels):
        R[:, level % k] += ((np.arange(n) >> level) & 1) * float(factor) ** level
    assert R.max() < 2.0 ** 24
    return R[rng.permutation(n)].astype(np.float32)
