"""Clusters on the routed ways (knn_index_self_cluster_within_routed, its host form, knn_debug_cluster_routed_plan,
knn_debug_cluster_pair; include/knn_mi355x.h 2n) without a GPU: the exported names, the argument rules in the header's order, the
plan's way against knn_debug_count_plan's and its launches against knn_debug_cluster_plan's, the link kernels' own decision lines
compiled for the host, and the shards of tests/test_cluster_routed_cells_gpu.py: that they are what it takes them for."""
import ctypes
import os

import numpy as np
import pytest

import multicore_hw2_amd as pkg
from tests import cluster_routed_rows as rr
from tests.cluster_helper import assert_planted
from tests.cluster_rows import largest_cluster, shares, spanning
from tests.topk_oracle import v0_dist2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
INF = float("inf")
NAN = float("nan")
vp = ctypes.c_void_p
NAMES = ("knn_index_self_cluster_within_routed", "knn_index_self_cluster_within_routed_host", "knn_debug_cluster_routed_plan",
         "knn_debug_cluster_pair")
INIT, PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS = 1, 2, 4, 8, 16, 32
FLAG_TEXT = "unknown flag (KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS)"


def test_the_two_names_and_the_two_hooks_are_declared_under_2n_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    section = header[header.index(" * 2n. Clusters on the routed ways"):header.index("/* Tuning / test hooks.")]
    L = pkg.lib()
    for name in NAMES:
        assert "int %s(" % name in section and name in pkg.EXPORTED_SYMBOLS, name
        getattr(L, name)
    for attr in ("self_cluster_within_routed", "self_cluster_within_routed_host"):
        assert callable(getattr(pkg.KnnIndex, attr))
    for attr in ("self_cluster_within_routed_c", "self_cluster_within_routed_host_c", "debug_cluster_routed_plan", "debug_cluster_pair"):
        assert attr in pkg.__all__ and callable(getattr(pkg, attr)), attr
    m2 = header[header.index(" * 2m. Clusters of the radius graph"):header.index(" * 2n. Clusters on the routed ways")]
    assert "Not built: clusters across shards" in m2 and "2n" in m2        # 2m's list lost its first item and points here


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
        return (pkg.self_cluster_within_routed_c()(None, slot, max_dist2, min_pts, labels, core, None, flags), L.knn_last_error().decode())

    who = "knn_index_self_cluster_within_routed: "
    _walk(who, rc, [
        (dict(max_dist2=-0.5), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=INIT), FLAG_TEXT),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(min_pts=0), "min_pts < 1"),
        (dict(labels=None), "null labels"),
    ])
    assert rc(max_dist2=NAN)[1] == who + "max_dist2 must be >= 0 and not NaN"
    for ok in (0.0, -0.0, INF):
        assert rc(max_dist2=ok)[1] == who + "null index"
    for flags in (INIT, PARTIAL, GRID, FRAMES, 1 << 31, COUNT_CELLS | INIT, COUNT_GRID | COUNT_CELLS | PARTIAL):
        assert rc(flags=flags) == (EINVAL, who + FLAG_TEXT), flags
    for flags in (COUNT_GRID, COUNT_CELLS, COUNT_GRID | COUNT_CELLS):
        assert rc(flags=flags)[1] == who + "null index", flags
    assert rc(core=vp(0x3000))[1] == who + "null index"
    assert rc(slot=-1)[1] == who + "slot outside 0 .. 7" and rc(min_pts=-4)[1] == who + "min_pts < 1"


def test_the_host_call_rejects_its_bad_arguments_without_a_gpu():
    L = pkg.lib()
    labels = (ctypes.c_int * 4)()

    def rc(max_dist2=1.0, min_pts=3, flags=0, lab=ctypes.cast(labels, vp)):
        return (pkg.self_cluster_within_routed_host_c()(None, max_dist2, min_pts, flags, lab, None, None), L.knn_last_error().decode())

    who = "knn_index_self_cluster_within_routed_host: "
    _walk(who, rc, [
        (dict(max_dist2=NAN), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=INIT), FLAG_TEXT),
        (dict(min_pts=0), "min_pts < 1"),
        (dict(lab=None), "null labels"),
    ])
    for flags in (PARTIAL, GRID, FRAMES, 1 << 31):
        assert rc(flags=flags) == (EINVAL, who + FLAG_TEXT), flags
    for flags in (COUNT_GRID, COUNT_CELLS, COUNT_GRID | COUNT_CELLS):
        assert rc(flags=flags)[1] == who + "null index", flags


def test_2ms_call_still_refuses_the_cells_flag_with_its_own_text():
    rv = pkg.self_cluster_within_c()(None, 0, 1.0, 3, vp(0x2000), None, None, COUNT_CELLS)
    assert rv == EINVAL and "the cell-pruned way is not built for it" in pkg.lib().knn_last_error().decode()


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def _inputs(rows, **over):
    base = dict(k=16, m=rows, n=rows, radius_finite=1, flag_grid=0, flag_cells=1, has_grid=0, has_cells=1, centred=0, rows_u8=0,
                bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=0)
    base.update(over)
    return base


ROUTE = [
    ("cells", 1 << 20, dict(), 4),
    ("bins", 1 << 20, dict(rows_u8=1, bins=1), 4),
    ("sharded", 1 << 20, dict(sharded=1), 4),
    ("path 2", 1 << 20, dict(path=2), 4),
    ("k 32", 1 << 20, dict(k=32), 4),
    ("rows 5", 5, dict(), 4),
    ("no flag", 1 << 20, dict(flag_cells=0), 1),
    ("infinite radius", 1 << 20, dict(radius_finite=0), 1),
    ("cells 2", 1 << 20, dict(cells=2), 1),
    ("path 1", 1 << 20, dict(path=1), 1),
    ("path 3", 1 << 20, dict(path=3), 1),
    ("per-cell frames", 1 << 20, dict(centred=1), 1),
    ("u8 rows in cell frames", 1 << 20, dict(rows_u8=1), 1),
    ("k 33", 1 << 20, dict(k=33), 1),
    ("rows 4", 4, dict(), 1),
    ("no layout", 1 << 20, dict(has_cells=0), 1),
    ("grid", 16391, dict(k=3, flag_grid=1, flag_cells=0, has_grid=1, has_cells=0, radius_rings=3), 3),
    ("grid before cells", 1 << 18, dict(k=4, flag_grid=1, has_grid=1, radius_rings=3), 3),
    ("grid flag on a cell layout", 1 << 20, dict(flag_grid=1), 4),
    ("grid flag alone on a cell layout", 1 << 20, dict(flag_grid=1, flag_cells=0), 1),
]


@pytest.mark.parametrize("name,rows,over,way", ROUTE, ids=[c[0] for c in ROUTE])
@pytest.mark.parametrize("core_given", [0, 1])
def test_the_plans_way_is_the_routed_counts_and_its_launches_on_ways_1_and_3_are_2ms(name, rows, over, way, core_given):
    inp = _inputs(rows, **over)
    cnt = pkg.debug_count_plan(**inp)
    p = pkg.debug_cluster_routed_plan(core_given=core_given, **inp)
    assert p["way"] == cnt["way"] == way, (name, p, cnt)
    words = (rows + 31) // 32
    assert p["scratch_bytes"] == 8 * rows + (0 if core_given else 4 * words)
    assert p["count_bytes"] == (0 if way == 1 else 4 * rows) and p["count_bytes"] == cnt["scratch_bytes"]
    if way != 4:
        old = pkg.debug_cluster_plan(k=inp["k"], n=rows, num_cu=256, core_given=core_given, grid=1 if way == 3 else 0)
        assert old["way"] == way and p["launches"] == p["launches_outliers"] == old["launches"], (name, p, old)
        assert p["chunks"] == old["chunks"] and p["scratch_bytes"] == old["scratch_bytes"] and p["count_bytes"] == old["count_bytes"]
        assert p["passes"] == 0 and p["pass_m"] == 0
    else:
        assert p["passes"] == cnt["passes"] == (rows + 1023) // 1024 and p["pass_m"] == cnt["pass_m"] == min(rows, 1024)


def test_on_way_4_the_launches_grow_by_a_pass_of_each_sweep_from_1024_to_1025_rows():
    # a pass of the degree step: prep, match, scan, count re-rank of the slices and of the overflow area, commit, gated self-scan = 7;
    # of the link sweep: the same front of 3, link re-rank of the slices and of the overflow area, the gated twin = 6; core; flatten
    one = pkg.debug_cluster_routed_plan(**_inputs(1024))
    two = pkg.debug_cluster_routed_plan(**_inputs(1025))
    assert (one["way"], one["passes"], one["pass_m"]) == (4, 1, 1024) and (two["way"], two["passes"], two["pass_m"]) == (4, 2, 1024)
    assert one["launches"] == 7 + 6 + 2 and two["launches"] == one["launches"] + 7 + 6
    assert one["launches_outliers"] == one["launches"] + 2 and two["launches_outliers"] == two["launches"] + 4
    big = pkg.debug_cluster_routed_plan(**_inputs(rr.N17))
    assert big["passes"] == 129 and big["launches"] == 129 * 13 + 2


def test_the_plans_bad_inputs():
    L = pkg.lib()
    who = "knn_debug_cluster_routed_plan: bad arguments"
    for over in (dict(m=99), dict(n=(1 << 31), m=(1 << 31)), dict(m=0, n=0), dict(path=4), dict(cells=3), dict(num_cu=0), dict(k=0),
                 dict(k=5, has_grid=1), dict(centred=2)):
        with pytest.raises(pkg.KnnError):
            pkg.debug_cluster_routed_plan(**_inputs(100, **over))
        assert L.knn_last_error().decode().startswith(who), over
    with pytest.raises(pkg.KnnError):
        pkg.debug_cluster_routed_plan(core_given=2, **_inputs(100))
    assert L.knn_last_error().decode().startswith(who)


# ---- the pair decision --------------------------------------------------------------------------------------------------------------
def test_the_pair_decision_in_all_eight_cases_and_for_the_own_row():
    for own_core in (0, 1):
        for row_core in (0, 1):
            for below in (0, 1):
                row, own = (3, 2000) if below else (2000, 3)
                want = "nothing"
                if row_core and own_core and below:
                    want = "unite"                                  # the owner of the LARGER row alone unites
                if row_core and not own_core:
                    want = "border"                                 # whichever of the two rows is the larger
                assert pkg.debug_cluster_pair(own_core, row_core, row, own) == want, (own_core, row_core, below)
            assert pkg.debug_cluster_pair(own_core, row_core, 77, 77) == "nothing"
    # every unordered pair of core rows is united exactly once: by one of its two ordered forms
    for a, b in ((0, 1), (5, 1 << 30), (1023, 1024)):
        assert sorted([pkg.debug_cluster_pair(1, 1, a, b), pkg.debug_cluster_pair(1, 1, b, a)]) == ["nothing", "unite"]
    for bad in ((2, 0, 1, 2), (0, -1, 1, 2), (0, 1, -1, 2), (0, 1, 1, 1 << 31)):
        with pytest.raises(pkg.KnnError):
            pkg.debug_cluster_pair(*bad)
        assert pkg.lib().knn_last_error().decode().startswith("knn_debug_cluster_pair: bad arguments")
    f = pkg.lib().knn_debug_cluster_pair
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)]
    assert f(1, 1, 1, 2, None) == EINVAL


# ---- the shards of the GPU file -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 16, 20])
def test_the_planted_shards_are_what_the_gpu_test_takes_them_for(k):
    R, names, off, r, min_pts = rr.planted17(k)
    plen = rr.planted_rows(names)
    assert R.shape == (rr.N17, k) and 4 <= min_pts <= 5
    assert off % rr.PASS != 0 and off // rr.PASS != (off + plen - 1) // rr.PASS            # the block straddles a pass boundary
    chain = names["chain down"] + off
    assert chain.min() < 64 * rr.PASS <= chain.max()                                       # ... inside its first chain
    assert abs(off + plen // 2 - rr.N17 // 2) < rr.N17 // 16                               # the middle of the row order
    # the radius: the power of two nearest (in the logarithm) the median 8th-neighbour distance of the uniform rows
    d8 = np.sqrt(np.median(rr.kth_neighbour_dist2(R, k, np.arange(256), 8).astype(np.float64)))
    assert r == 2.0 ** round(np.log2(d8)), (k, d8, r)
    # no uniform row within the radius of a planted one (with room): the planted statements hold whatever the uniform rows do
    P = R[off:off + plen]
    U = np.concatenate([R[:off], R[off + plen:]])
    assert U.min() >= 0.0 and U.max() < 1.0 and P[:, 0].min() > 1.0
    assert float(v0_dist2(P, U, k).min()) > 1.25 * r * r, k
    # the block alone, by the oracle: the statements of assert_planted
    from tests import cluster_oracle as co
    w = co.cluster(P, k, r * r, min_pts)
    assert_planted(w["labels"], w["core"], names, 0, min_pts)


def test_the_long_box_has_every_kind_of_row_a_large_cluster_and_clusters_across_passes():
    R, cap = rr.long_box()
    w = rr.want_long_box()                                        # (the oracle finishes here: about 20 s)
    labels = w["labels"]
    assert R.shape == (rr.N17, rr.LONG_K) and float(R[:, 0].max()) > 15.0 and float(R[:, 1:].max()) < 1.0
    assert 5 <= np.median(w["deg"]) <= 15, np.median(w["deg"])
    core, border, noise = shares(w)
    assert min(core, border, noise) >= 0.02, (core, border, noise)
    assert largest_cluster(labels) >= 1000
    assert spanning(labels, at=rr.PASS).size >= 1                  # a cluster with rows on both sides of row 1024
    ok = labels >= 0
    reps, inv = np.unique(labels[ok], return_inverse=True)
    passes = (np.flatnonzero(ok) // rr.PASS).astype(np.int64)
    lo, hi = np.full(reps.size, 1 << 40), np.full(reps.size, -1)
    np.minimum.at(lo, inv, passes)
    np.maximum.at(hi, inv, passes)
    assert reps.size >= 10 and ((hi - lo) >= 2).any()              # some cluster spans two non-adjacent passes


def test_the_fallback_shard_has_its_two_rows_in_two_passes_the_far_one_in_the_last():
    R, far, bad = rr.fallback_rows(8)
    last = (rr.N17 - 1) // rr.PASS
    assert far // rr.PASS == last and 0 < bad // rr.PASS < last - 1
    assert (R[far] == np.float32(1e6)).all() and np.isnan(R[bad]).sum() == 1
    keep = np.ones(rr.N17, dtype=bool)
    keep[[far, bad]] = False
    assert np.isfinite(R[keep]).all() and R[keep].max() < 1.0
