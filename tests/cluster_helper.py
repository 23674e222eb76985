"""knn_index_self_cluster_within — what its GPU tests share (test infrastructure): the call itself with poisoned outputs, and the
planted structures.  Expectations always come from tests/cluster_oracle.py.

The planted structures are stated in UNITS of the radius (`r`: a power of two; the call's max_dist2 is r * r), laid out one after
the other along axis 0 from `x0` on, four units apart, their inner extent along the LAST axis (axis 0 itself at k = 1); every
other coordinate is `rest`.  All coordinates are multiples of r / 4 — exactly representable, and so are the differences and the
squared distances the tests rely on.  They need 4 <= min_pts <= 5:
  chain     CHAIN rows a quarter unit apart: inner rows have 8 rows within the radius, the two ends 4 — every row core; rows two
            ends apart are far outside each other's radius, so only the union of many links makes it ONE cluster.  Twice: in
            descending row order (every unite hooks a root under a new smaller row) and in shuffled order;
  bridge    two runs of 9 rows a quarter unit apart, their nearest ends two units apart, and ONE row midway: it is within the
            radius of exactly one row of each run, at E == max_dist2 exactly on both sides — deg 2, not core.  The runs must stay
            two clusters, and the bridge takes the label of the run whose end row has the lower row number.  That run is given
            the HIGHER label (its other rows come later), so "the smaller label" is the wrong rule;
  copies    5 exact duplicates (deg 4 each: one cluster at distance 0) and, elsewhere, 2 duplicates (deg 1: noise);
  touching  two groups of 5 duplicates exactly one unit apart: E == max_dist2, linked, one cluster;
  apart     two groups of 5 duplicates one unit and one ulp apart: not linked, two clusters."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

from tests.count_helper import dev

CHAIN = 100


def run_cluster(ix, max_dist2, min_pts, want_core=True, slot=0, **flags):
    """One call: (labels int32 [n], core words uint32 [(n + 31) // 32] or None, last_stats) — outputs poisoned first."""
    n = ix.n
    labels = torch.full((n,), -7, dtype=torch.int32, device=dev())
    core = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev()) if want_core else None
    torch.cuda.synchronize()
    ix.self_cluster_within(max_dist2, min_pts, labels.data_ptr(), core_dev=core.data_ptr() if want_core else None, slot=slot, **flags)
    torch.cuda.synchronize()
    st = ix.last_stats()
    return labels.cpu().numpy(), (core.cpu().numpy().view(np.uint32) if want_core else None), st


def planted(k, r, x0, rest, rng):
    """(rows float32 [p][k], names: dict of structure -> row numbers WITHIN the planted block, in the block's row order)."""
    inner = k - 1
    rows, names = [], {}
    at = [np.float64(x0)]

    def put(name, us, order=None):
        """rows at inner coordinates us (units) in the next place along axis 0; order: their row order within the block."""
        us = np.asarray(us, dtype=np.float64)
        us = us - us.min()
        P = np.full((us.size, k), rest, dtype=np.float64)
        P[:, 0] = at[0]
        P[:, inner] = (at[0] if inner == 0 else 0.0) + us * r
        at[0] += ((us.max() if inner == 0 else 0.0) + 4.0) * r
        if order is not None:
            P = P[order]
        first = sum(len(x) for x in rows)
        rows.append(P)
        names[name] = first + np.arange(us.size)
        return first

    put("chain down", 0.25 * np.arange(CHAIN), order=np.arange(CHAIN)[::-1])
    put("chain mixed", 0.25 * np.arange(CHAIN), order=rng.permutation(CHAIN))
    # bridge: run A at u = -2 .. 0 (its end row at 0), run B at u = 2 .. 4 (its end row at 2), the bridge at u = 1.  Row order within
    # the block: two rows of B's far end first — core rows, so B's label is the lowest number here —, then A's end row, then B's end
    # row, then the bridge, then the rest: A's end row has the lower number of the two the bridge touches, and A the HIGHER label
    a_run, b_run = -0.25 * np.arange(9), 2.0 + 0.25 * np.arange(9)
    us = np.concatenate([a_run, b_run, [1.0]])
    a_end, b_end, bridge = 0, 9, 18
    order = np.array([17, 16, a_end, b_end, bridge] + [i for i in range(19) if i not in (17, 16, a_end, b_end, bridge)])
    first = put("bridge", us, order=order)
    pos = {int(src): first + t for t, src in enumerate(order)}
    names["bridge row"] = np.array([pos[bridge]])
    names["bridge A"] = np.array(sorted(pos[i] for i in range(0, 9)))
    names["bridge B"] = np.array(sorted(pos[i] for i in range(9, 18)))
    names["bridge A end"], names["bridge B end"] = np.array([pos[a_end]]), np.array([pos[b_end]])
    put("copies", np.zeros(5))
    put("two copies", np.zeros(2))
    put("touching", np.concatenate([np.zeros(5), np.ones(5)]), order=rng.permutation(10))
    first = put("apart", np.concatenate([np.zeros(5), np.ones(5)]))
    out = np.concatenate(rows).astype(np.float32)
    assert (out.astype(np.float64) == np.concatenate(rows)).all()            # exactly representable
    far = first + 5 + np.arange(5)
    out[far, inner] = np.nextafter(out[far, inner], np.float32(np.inf))      # one ulp beyond the unit
    names["apart near"], names["apart far"] = first + np.arange(5), far
    return out, names, float(at[0])


def assert_planted(labels, core, names, off, min_pts):
    """The statements about the planted structures that need no oracle; off: the block's first row in the shard."""
    assert 4 <= min_pts <= 5
    g = lambda name: names[name] + off
    for chain in ("chain down", "chain mixed"):
        rows = g(chain)
        assert core[rows].all(), chain
        assert (labels[rows] == rows.min()).all(), (chain, np.unique(labels[rows]))          # ONE cluster, its smallest row
    a, b, br = g("bridge A"), g("bridge B"), int(g("bridge row")[0])
    assert not core[br] and core[g("bridge A end")].all() and core[g("bridge B end")].all()
    la, lb = np.unique(labels[a]), np.unique(labels[b])
    assert la.size == 1 and lb.size == 1 and la[0] != lb[0], (la, lb)                         # two clusters still
    assert la[0] == a[core[a]].min() and lb[0] == b[core[b]].min()
    assert g("bridge A end")[0] < g("bridge B end")[0] and lb[0] < la[0]                     # the lower end row, the HIGHER label
    assert labels[br] == la[0], (labels[br], la, lb)
    assert (labels[g("copies")] == g("copies").min()).all() and core[g("copies")].all()
    assert (labels[g("two copies")] == -1).all() and not core[g("two copies")].any()
    assert (labels[g("touching")] == g("touching").min()).all()                               # E == max_dist2 links
    near, far = g("apart near"), g("apart far")
    assert (labels[near] == near.min()).all() and (labels[far] == far.min()).all()           # one ulp beyond does not
