"""Clusters of the radius graph (knn_index_self_cluster_within, its host form, knn_debug_cluster_plan, knn_debug_cluster_unite;
include/knn_mi355x.h 2m) without a GPU: the exported names, the kernels' own union-find lines (knn_cluster_uf.h) run on the host
against a plain numpy union-find, the plan's arithmetic, the argument rules in the header's order, and tests/cluster_oracle.py
against scikit-learn's DBSCAN where that is installed."""
import ctypes
import os

import numpy as np
import pytest

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
INF = float("inf")
NAN = float("nan")
vp = ctypes.c_void_p
NAMES = ("knn_index_self_cluster_within", "knn_index_self_cluster_within_host", "knn_debug_cluster_plan", "knn_debug_cluster_unite")
INIT, PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS = 1, 2, 4, 8, 16, 32
CHUNK = 65536


def test_the_four_names_are_declared_under_2m_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    section = header[header.index(" * 2m. Clusters of the radius graph"):header.index("/* Tuning / test hooks.")]
    L = pkg.lib()
    for name in NAMES:
        assert "int %s(" % name in section and name in pkg.EXPORTED_SYMBOLS, name
        getattr(L, name)
    assert "#define KNN_CLUSTER_NOISE (-1)" in section and pkg.CLUSTER_NOISE == -1
    for attr in ("self_cluster_within", "self_cluster_within_host"):
        assert callable(getattr(pkg.KnnIndex, attr))
    assert callable(pkg.debug_cluster_plan) and callable(pkg.debug_cluster_unite)


# ---- the union-find ---------------------------------------------------------------------------------------------------------------
def roots_of(parent):
    """find(x) for every x, read-only."""
    lab = np.asarray(parent, dtype=np.int64).copy()
    while True:
        nxt = lab[lab]
        if (nxt == lab).all():
            return lab
        lab = nxt


def check_forest(parent, n, pairs):
    assert (parent <= np.arange(n)).all() and (parent >= 0).all()            # parent[x] <= x for every x
    want = co.components(n, pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64))
    np.testing.assert_array_equal(roots_of(parent), want)                      # the same sets, root = the smallest member


@pytest.mark.parametrize("n, npairs, seed", [(1, 0, 1), (50, 20, 2), (1000, 700, 3), (5000, 9000, 4), (3000, 1500, 5)])
def test_unite_gives_the_components_of_its_pairs_in_every_order_and_twice_changes_nothing(n, npairs, seed):
    rng = np.random.default_rng(seed)
    pairs = rng.integers(0, n, size=(npairs, 2), dtype=np.int32)
    if npairs:
        pairs[::7, 1] = pairs[::7, 0]                                          # some pairs of a row with itself
    for order in range(4):
        p = pairs[rng.permutation(npairs)] if order else pairs
        if order == 3:
            p = p[:, ::-1]
        parent = np.arange(n, dtype=np.int32)
        pkg.debug_cluster_unite(parent, p)
        check_forest(parent, n, pairs)
        roots = roots_of(parent)
        pkg.debug_cluster_unite(parent, p)                                     # idempotent: the sets and the roots stay
        np.testing.assert_array_equal(roots_of(parent), roots)
        assert (parent <= np.arange(n)).all()
        again = parent.copy()
        pkg.debug_cluster_unite(parent, np.stack([np.arange(n), roots], axis=1).astype(np.int32))
        np.testing.assert_array_equal(roots_of(parent), roots)
        assert (parent <= again).all()                                         # a parent only ever moves towards the root


def test_a_descending_chain_ends_under_its_smallest_row():
    n = 4097
    chain = np.stack([np.arange(n - 1, 0, -1), np.arange(n - 2, -1, -1)], axis=1).astype(np.int32)   # (n-1, n-2), ..., (1, 0)
    for pairs in (chain, chain[::-1], chain[:, ::-1], chain[np.random.default_rng(9).permutation(n - 1)]):
        parent = np.arange(n, dtype=np.int32)
        pkg.debug_cluster_unite(parent, pairs)
        assert (parent <= np.arange(n)).all()
        assert (roots_of(parent) == 0).all()
        before = roots_of(parent)
        pkg.debug_cluster_unite(parent, pairs)
        np.testing.assert_array_equal(roots_of(parent), before)
    # two chains that share no row stay two sets
    parent = np.arange(n, dtype=np.int32)
    odd = chain[(chain[:, 0] >= 2000) | (chain[:, 0] < 1999)]                 # the link (1999, 1998) left out
    pkg.debug_cluster_unite(parent, odd)
    r = roots_of(parent)
    assert (r[:1999] == 0).all() and (r[1999:] == 1999).all()


def test_unite_refuses_rows_outside_the_array_and_a_forest_that_breaks_the_invariant():
    L = pkg.lib()
    parent = np.arange(8, dtype=np.int32)
    for bad in ([[0, 8]], [[-1, 2]]):
        with pytest.raises(pkg.KnnError):
            pkg.debug_cluster_unite(parent, bad)
        assert L.knn_last_error().decode().startswith("knn_debug_cluster_unite: a pair names a row outside")
    np.testing.assert_array_equal(parent, np.arange(8))
    broken = np.array([0, 2, 2], dtype=np.int32)
    with pytest.raises(pkg.KnnError):
        pkg.debug_cluster_unite(broken, [[0, 1]])
    assert "parent[x] <= x" in L.knn_last_error().decode()


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1500, CHUNK, CHUNK + 70, 16384 + 7, 1 << 20])
@pytest.mark.parametrize("core_given", [0, 1])
def test_the_plan_counts_chunks_launches_and_scratch(n, core_given):
    chunks = (n + CHUNK - 1) // CHUNK
    words = (n + 31) // 32
    for k, grid in ((3, 0), (3, 1), (40, 0)):
        p = pkg.debug_cluster_plan(k=k, n=n, num_cu=256, core_given=core_given, grid=grid)
        assert p["chunks"] == chunks
        assert p["slices"] == pkg.debug_self_plan(k=k, rows=min(n, CHUNK), K=0, shard_rows=n, num_cu=256, init=1)["slices"]
        assert p["launches_exact"] == 2 * chunks + 2 and p["launches_grid"] == 2 * chunks + 5
        assert p["scratch_bytes"] == 8 * n + (0 if core_given else 4 * words)
        assert p["count_bytes"] == (4 * n if grid else 0)
        assert p["way"] == (3 if grid else 1)
        assert p["launches"] == (p["launches_grid"] if grid else p["launches_exact"])


def test_the_plan_of_an_empty_shard_and_its_bad_inputs():
    p = pkg.debug_cluster_plan(k=3, n=0, num_cu=256, core_given=0, grid=1)
    assert p["chunks"] == 0 and p["scratch_bytes"] == 0 and p["way"] == 1 and p["count_bytes"] == 0
    good = dict(k=3, n=100, num_cu=256, core_given=0, grid=0)
    for bad in (dict(k=0), dict(n=-1), dict(n=1 << 31), dict(num_cu=0), dict(core_given=2), dict(grid=2), dict(k=5, grid=1)):
        with pytest.raises(pkg.KnnError):
            pkg.debug_cluster_plan(**dict(good, **bad))
        assert pkg.lib().knn_last_error().decode().startswith("knn_debug_cluster_plan: bad arguments")


# ---- the argument rules -----------------------------------------------------------------------------------------------------------
def _walk(who, rc, rules):
    """rules in the header's order: each one speaks when it alone is broken, and ahead of every rule behind it."""
    assert rc() == (EINVAL, who + "null index")
    for i, (broken, text) in enumerate(rules):
        assert rc(**broken) == (EINVAL, who + text), broken
        for later, _ in rules[i + 1:]:
            assert rc(**dict(later, **broken)) == (EINVAL, who + text), (broken, later)


def test_the_device_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    lab = vp(0x2000)

    def rc(slot=0, max_dist2=1.0, min_pts=3, labels=lab, core=None, flags=0):
        return (pkg.self_cluster_within_c()(None, slot, max_dist2, min_pts, labels, core, None, flags), L.knn_last_error().decode())

    who = "knn_index_self_cluster_within: "
    flag_text = "unknown flag (KNN_QUERY_COUNT_GRID alone is admitted"
    _walk(who, rc, [
        (dict(max_dist2=-0.5), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=COUNT_CELLS), flag_text + ": the call always writes its labels, and the cell-pruned way is not built for it)"),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(min_pts=0), "min_pts < 1"),
        (dict(labels=None), "null labels"),
    ])
    assert rc(max_dist2=NAN)[1] == who + "max_dist2 must be >= 0 and not NaN"
    for ok in (0.0, -0.0, INF):
        assert rc(max_dist2=ok)[1] == who + "null index"
    for flags in (INIT, PARTIAL, GRID, FRAMES, COUNT_CELLS, COUNT_GRID | COUNT_CELLS, COUNT_GRID | INIT, 1 << 31):
        assert rc(flags=flags)[1].startswith(who + flag_text), flags
    assert rc(flags=COUNT_GRID)[1] == who + "null index"
    assert rc(core=vp(0x3000))[1] == who + "null index"
    assert rc(slot=-1)[1] == who + "slot outside 0 .. 7" and rc(min_pts=-4)[1] == who + "min_pts < 1"


def test_the_host_call_rejects_its_bad_arguments_without_a_gpu():
    L = pkg.lib()
    labels = (ctypes.c_int * 4)()

    def rc(max_dist2=1.0, min_pts=3, flags=0, lab=ctypes.cast(labels, vp)):
        return (pkg.self_cluster_within_host_c()(None, max_dist2, min_pts, flags, lab, None, None), L.knn_last_error().decode())

    who = "knn_index_self_cluster_within_host: "
    _walk(who, rc, [
        (dict(max_dist2=NAN), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=COUNT_CELLS), "unknown flag (KNN_QUERY_COUNT_GRID alone is admitted: the call always writes its labels, and the "
                                  "cell-pruned way is not built for it)"),
        (dict(min_pts=0), "min_pts < 1"),
        (dict(lab=None), "null labels"),
    ])
    assert rc(flags=COUNT_GRID)[1] == who + "null index"


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def test_the_oracle_on_a_hand_made_set():
    """1-D, radius 1 (max_dist2 1), min_pts 3: rows 0..2 at 0, 1, 2 — the middle one core, its neighbours border —, a far pair
    (deg 1 each: noise), and a dense blob whose bridge row to the first group is not core."""
    R = np.array([0.0, 1.0, 2.0, 10.0, 11.0, 4.0, 4.0, 4.5, 3.0], dtype=np.float32).reshape(-1, 1)
    got = co.cluster(R, 1, 1.0, 3)
    np.testing.assert_array_equal(got["deg"], [1, 2, 2, 1, 1, 3, 3, 2, 3])
    np.testing.assert_array_equal(got["core"], [0, 1, 1, 0, 0, 1, 1, 1, 1])
    # 1-2-8-5/6-7 chain through core rows: one cluster, label = its smallest core row (1); row 0 borders on row 1
    np.testing.assert_array_equal(got["labels"], [1, 1, 1, -1, -1, 1, 1, 1, 1])
    np.testing.assert_array_equal(co.renumber(got["labels"]), [0, 0, 0, -1, -1, 0, 0, 0, 0])
    got = co.cluster(R, 1, 1.0, 4)       # rows 5, 6, 8 alone are core
    np.testing.assert_array_equal(got["core"], [0, 0, 0, 0, 0, 1, 1, 0, 1])
    # row 2 borders on row 8 (distance 1), row 7 on rows 5 and 6 at the same distance: the lower row's label — the same cluster
    np.testing.assert_array_equal(got["labels"], [-1, -1, 5, -1, -1, 5, 5, 5, 5])
    np.testing.assert_array_equal(co.core_mask_words(got["core"]), [0b101100000])
    everything = co.cluster(R, 1, 1.0, 1)["labels"]
    np.testing.assert_array_equal(everything, [0, 0, 0, 3, 3, 0, 0, 0, 0])


def test_the_oracle_agrees_with_scikit_learn_on_integer_points():
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(77)
    R = rng.integers(0, 24, size=(400, 2)).astype(np.float32)          # integer grid: every distance exact, duplicates included
    seen = set()
    for max_dist2, min_pts in ((1.0, 3), (4.0, 6), (2.0, 4), (9.0, 1), (1.0, 30)):
        got = co.cluster(R, 2, max_dist2, min_pts)
        sk = cluster.DBSCAN(eps=float(np.sqrt(max_dist2)), min_samples=min_pts, algorithm="brute").fit(R.astype(np.float64))
        core_sk = np.zeros(len(R), dtype=bool)
        core_sk[sk.core_sample_indices_] = True
        np.testing.assert_array_equal(got["core"], core_sk)
        np.testing.assert_array_equal(got["labels"] < 0, sk.labels_ < 0)                       # the same noise set
        mine = co.renumber(got["labels"])
        np.testing.assert_array_equal(mine[core_sk], sk.labels_[core_sk])                       # identical on core rows
        d = ((R[:, None, :].astype(np.float64) - R[None, :, :]) ** 2).sum(axis=2)
        for j in np.flatnonzero(~core_sk & (mine >= 0)):                                        # a border row: SOME core row's label
            near = core_sk & (d[j] <= max_dist2)
            assert mine[j] in mine[near], j
        seen.add((bool(core_sk.any()), bool((~core_sk & (mine >= 0)).any()), bool((mine < 0).any())))
    assert (True, True, True) in seen
