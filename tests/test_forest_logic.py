"""Minimum spanning forest of the radius graph (knn_index_self_forest_within, its host form, knn_debug_forest_plan,
knn_debug_forest_round; include/knn_mi355x.h 2o) — everything that needs no GPU: whole forests through the kernels' own pick and
hook lines with the host's atomics against Kruskal under the edge order (tests/forest_oracle.py), the same from several host
threads, the plan against hand-computed values, the argument rules in the header's order."""
import ctypes
import os

import numpy as np
import pytest

import multicore_hw2_amd as pkg
from tests import forest_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
INF, NAN = float("inf"), float("nan")
INIT, PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS = 1, 2, 4, 8, 16, 32
vp = ctypes.c_void_p
NAMES = ("knn_index_self_forest_within", "knn_index_self_forest_within_host", "knn_debug_forest_plan", "knn_debug_forest_round")


def test_the_four_names_are_declared_under_2o_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "knn_mi355x.h")).read()
    section = header[header.index(" * 2o. Minimum spanning forest"):]
    for name in NAMES:
        assert "int %s(" % name in section and name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    for word in ("cell-pruned way", "across shards", "mutual-reachability", "dendrogram", "mask of admitted rows", "radius per row"):
        assert word in section[section.index("Not built"):], word
    assert callable(pkg.debug_forest_plan) and callable(pkg.debug_forest_round)
    assert callable(pkg.KnnIndex.self_forest_within) and callable(pkg.KnnIndex.self_forest_within_host)


# ---- whole forests through knn_debug_forest_round ---------------------------------------------------------------------------------
def lattice(n, k, side, seed):
    """Integer-lattice rows: every squared distance a small integer, so equal distances and duplicates are everywhere."""
    return np.random.default_rng(seed).integers(0, side, size=(n, k)).astype(np.float32)


def check_forest(R, k, max_dist2, threads=1):
    n = R.shape[0]
    a, b, bits = fo.pairs(R, k, max_dist2)
    want = fo.forest_of_pairs(n, a, b, bits)
    got = fo.run_rounds(pkg.debug_forest_round, n, a, b, bits, threads=threads)
    table = got["table"]
    np.testing.assert_array_equal(table, fo.want_table(want))                     # the edge set is the oracle's
    assert got["raw"] == len(table) == len(np.unique(table, axis=0))              # no edge appears twice
    assert (table[:, 1] < table[:, 2]).all()
    assert got["rounds"] <= fo.rounds_of(n) and got["calls"] <= got["rounds"] + 1
    np.testing.assert_array_equal(fo.roots_of(got["parent"]), want["labels"])     # the final roots are the component minima
    assert len(table) == n - np.unique(want["labels"]).size
    return got, want


@pytest.mark.parametrize("k,n,side,seed", [(1, 97, 40, 1), (2, 131, 9, 2), (3, 211, 5, 3), (4, 300, 4, 4), (2, 300, 30, 5)])
@pytest.mark.parametrize("max_dist2", [1.0, 2.0, INF])
def test_lattice_rows_with_many_equal_distances_give_kruskals_forest(k, n, side, seed, max_dist2):
    got, want = check_forest(lattice(n, k, side, seed), k, max_dist2)
    if max_dist2 == INF:
        assert len(got["table"]) == n - 1 and (want["labels"] == 0).all()


def test_seventy_identical_rows_are_the_star_from_row_zero():
    R = np.full((70, 3), 2.5, dtype=np.float32)
    for cap in (0.0, INF):
        got, _ = check_forest(R, 3, cap)
        np.testing.assert_array_equal(got["table"], np.stack([np.zeros(69, int), np.zeros(69, int), np.arange(1, 70)], axis=1))
        assert got["rounds"] == 1


def test_duplicates_a_row_with_a_nan_and_an_isolated_row():
    R = lattice(120, 2, 6, 9)
    R[40:50] = R[7]                      # ten more copies of row 7
    R[33, 1] = np.nan                    # no edge at any radius
    R[90] = (1000.0, 1000.0)             # isolated at the finite radius, a leaf at +INF
    for cap in (1.0, INF):
        got, want = check_forest(R, 2, cap)
        assert want["labels"][33] == 33 and not (got["table"][:, 1:] == 33).any()
        assert (want["labels"][90] == 90) == (cap == 1.0)


def test_a_shard_of_one_row_and_of_none():
    got, _ = check_forest(np.zeros((1, 2), dtype=np.float32), 2, INF)
    assert got["raw"] == 0 and got["rounds"] == 0 and got["calls"] == 1
    count = np.zeros(2, dtype=np.uint32)
    assert pkg.debug_forest_round(np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), count) == 0
    assert count.tolist() == [0, 0]


@pytest.mark.parametrize("threads", [2, 5, 16])
def test_several_host_threads_on_one_array_give_the_same_forest(threads):
    for k, n, side, cap in ((2, 300, 7, 1.0), (3, 257, 4, INF)):
        R = lattice(n, k, side, 20 + threads)
        alone, _ = check_forest(R, k, cap)
        shared, _ = check_forest(R, k, cap, threads=threads)
        np.testing.assert_array_equal(shared["table"], alone["table"])
        assert shared["rounds"] == alone["rounds"]


@pytest.mark.parametrize("levels,k,factor", [(2, 1, 4), (3, 1, 4), (6, 1, 4), (3, 2, 3), (6, 2, 3), (10, 2, 3)])
def test_rows_paired_at_every_level_need_every_round_and_the_last_flatten(levels, k, factor):
    """The device call's own sequence on the RAW parent array: exactly ROUNDS(n) rounds, every one of which adds an edge, then the
    last flatten (a round of empty candidates).  Before it the array is a forest deeper than 1 — the last hook re-parented a root
    alone —, behind it parent[i] is the smallest row of i's component."""
    n = 1 << levels
    R = fo.paired(levels, k, factor, np.random.default_rng(70 + levels))
    a, b, bits = fo.pairs(R, k, INF)
    want = fo.forest_of_pairs(n, a, b, bits)
    assert fo.rounds_of(n) == levels and (want["labels"] == 0).all()
    parent = np.arange(n, dtype=np.int32)
    keys, his, count = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(2, np.uint32)
    for t in range(levels):
        cand = fo.candidates(n, a, b, bits, fo.roots_of(parent))
        assert pkg.debug_forest_round(parent, cand, keys, his, count) == n >> (t + 1)     # the components halve exactly
    assert count.tolist() == [n - 1, levels]
    np.testing.assert_array_equal(fo.edge_table(keys[:n - 1], his[:n - 1]), fo.want_table(want))
    assert (parent != want["labels"]).any()                                                # not the answer yet
    none = np.full(n, fo.KEY_INIT, dtype=np.uint64)
    assert pkg.debug_forest_round(parent, none, keys, his, count) == 0
    np.testing.assert_array_equal(parent, want["labels"])                                  # RAW, not roots_of
    assert count.tolist() == [n - 1, levels]


def test_the_round_refuses_a_broken_forest_and_a_bad_candidate():
    L = pkg.lib()
    good = lambda: (np.arange(4, dtype=np.int32), np.full(4, fo.KEY_INIT, dtype=np.uint64), np.zeros(4, np.uint64), np.zeros(4, np.uint32),
                    np.zeros(2, np.uint32))
    p, c, ek, eh, cnt = good()
    p[1] = 3
    with pytest.raises(pkg.KnnError):
        pkg.debug_forest_round(p, c, ek, eh, cnt)
    assert "parent[x] <= x" in L.knn_last_error().decode()
    for bad in (2, 7):                   # the row itself, a row outside
        p, c, ek, eh, cnt = good()
        c[2] = np.uint64((0x3F800000 << 32) | bad)
        with pytest.raises(pkg.KnnError):
            pkg.debug_forest_round(p, c, ek, eh, cnt)
        assert L.knn_last_error().decode().startswith("knn_debug_forest_round: a candidate names")


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
# by hand, 256 CUs: ROUNDS = max(1, ceil(log2 n)); chunks = ceil(n / 65536); slices of the first chunk = min(8192 / ceil(mc / 64),
# ceil(n / 1024)) evened out; launches = ROUNDS (5 + chunks) + 1 exact, ROUNDS (6 + chunks) + 1 grid (the last flatten); scratch =
# 20 n + 4 ceil(n / 32) + 4 (2 ROUNDS + 2)
PLAN = {
    1: dict(rounds=1, chunks=1, slices=1, launches_exact=7, launches_grid=8, scratch_bytes=40),
    2: dict(rounds=1, chunks=1, slices=1, launches_exact=7, launches_grid=8, scratch_bytes=60),
    65536: dict(rounds=16, chunks=1, slices=8, launches_exact=97, launches_grid=113, scratch_bytes=1319048),
    65537: dict(rounds=17, chunks=2, slices=8, launches_exact=120, launches_grid=137, scratch_bytes=1319080),
    1 << 20: dict(rounds=20, chunks=16, slices=8, launches_exact=421, launches_grid=441, scratch_bytes=21102760),
}


@pytest.mark.parametrize("n", sorted(PLAN))
def test_the_plan_counts_rounds_chunks_launches_and_scratch(n):
    assert pkg.forest_rounds(n) == fo.rounds_of(n) == PLAN[n]["rounds"]
    for k, grid in ((3, 0), (3, 1), (40, 0)):
        p = pkg.debug_forest_plan(k=k, n=n, num_cu=256, grid=grid)
        for key, value in PLAN[n].items():
            assert p[key] == value, (key, p)
        assert p["way"] == (3 if grid else 1)
        assert p["launches"] == (p["launches_grid"] if grid else p["launches_exact"])


def test_the_plan_of_an_empty_shard_and_its_bad_inputs():
    p = pkg.debug_forest_plan(k=3, n=0, num_cu=256, grid=1)
    assert p["rounds"] == 0 and p["chunks"] == 0 and p["scratch_bytes"] == 0 and p["way"] == 1 and p["launches"] == 0
    good = dict(k=3, n=100, num_cu=256, grid=0)
    for bad in (dict(k=0), dict(n=-1), dict(n=1 << 31), dict(num_cu=0), dict(grid=2), dict(k=5, grid=1)):
        with pytest.raises(pkg.KnnError):
            pkg.debug_forest_plan(**dict(good, **bad))
        assert pkg.lib().knn_last_error().decode().startswith("knn_debug_forest_plan: bad arguments")


# ---- the argument rules -----------------------------------------------------------------------------------------------------------
def _walk(who, rc, rules):
    """rules in the header's order: each one speaks when it alone is broken, and ahead of every rule behind it."""
    assert rc() == (EINVAL, who + "null index")
    for i, (broken, text) in enumerate(rules):
        assert rc(**broken) == (EINVAL, who + text), broken
        for later, _ in rules[i + 1:]:
            assert rc(**dict(later, **broken)) == (EINVAL, who + text), (broken, later)


FLAG_TEXT = ("unknown flag (KNN_QUERY_COUNT_GRID alone is admitted: the call always writes its outputs, and the cell-pruned way is "
             "not built for it)")


def test_the_device_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()

    def rc(slot=0, max_dist2=1.0, labels=vp(0x2000), keys=vp(0x3000), his=vp(0x4000), count=vp(0x5000), flags=0):
        return (pkg.self_forest_within_c()(None, slot, max_dist2, labels, keys, his, count, None, flags), L.knn_last_error().decode())

    who = "knn_index_self_forest_within: "
    null_text = "null labels, edge keys, edge hi or count"
    _walk(who, rc, [
        (dict(max_dist2=-0.5), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=COUNT_CELLS), FLAG_TEXT),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(labels=None), null_text),
    ])
    for name in ("keys", "his", "count"):
        assert rc(**{name: None})[1] == who + null_text
    assert rc(max_dist2=NAN)[1] == who + "max_dist2 must be >= 0 and not NaN"
    for ok in (0.0, -0.0, INF):
        assert rc(max_dist2=ok)[1] == who + "null index"
    for flags in (INIT, PARTIAL, GRID, FRAMES, COUNT_CELLS, COUNT_GRID | COUNT_CELLS, COUNT_GRID | INIT, 1 << 31):
        assert rc(flags=flags)[1] == who + FLAG_TEXT, flags
    assert rc(flags=COUNT_GRID)[1] == who + "null index"
    assert rc(slot=-1)[1] == who + "slot outside 0 .. 7"


def test_the_host_call_rejects_its_bad_arguments_without_a_gpu():
    L = pkg.lib()
    lo, hi = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()

    def rc(max_dist2=1.0, flags=0, lo=ctypes.cast(lo, vp), hi=ctypes.cast(hi, vp)):
        return (pkg.self_forest_within_host_c()(None, max_dist2, flags, None, lo, hi, None, None), L.knn_last_error().decode())

    who = "knn_index_self_forest_within_host: "
    _walk(who, rc, [
        (dict(max_dist2=NAN), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=INIT), FLAG_TEXT),
        (dict(lo=None), "null lo or hi"),
    ])
    assert rc(hi=None)[1] == who + "null lo or hi"
    assert rc(flags=COUNT_GRID)[1] == who + "null index"


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def test_the_oracle_on_a_hand_made_set():
    # a line: 0 -1- 1 -1- 2 --3-- 5, and row 4 a copy of row 0
    R = np.array([[0.0], [1.0], [2.0], [5.0], [0.0]], dtype=np.float32)
    one, nine = int(np.float32(1.0).view(np.uint32)), int(np.float32(9.0).view(np.uint32))
    w = fo.forest(R, 1, 1.0)
    np.testing.assert_array_equal(fo.want_table(w), [[0, 0, 4], [one, 0, 1], [one, 1, 2]])   # (1, 1, 4) closes a cycle: not taken
    np.testing.assert_array_equal(w["labels"], [0, 0, 0, 3, 0])
    w = fo.forest(R, 1, INF)
    np.testing.assert_array_equal(fo.want_table(w), [[0, 0, 4], [one, 0, 1], [one, 1, 2], [nine, 2, 3]])
    np.testing.assert_array_equal(w["labels"], [0, 0, 0, 0, 0])
