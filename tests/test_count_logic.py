"""knn_index_count_within on the CPU: which way answers a call (knn_count_route, restated here and compared through
knn_debug_count_plan), the entry points' argument errors (they are decided before anything touches a device), and the numpy oracle
the GPU tests expect from (tests/count_oracle.py) on a hand-made case."""
import ctypes
import itertools

import numpy as np
import pytest

import multicore_hw2_amd as pkg
from tests.count_oracle import counts, counts_of, kinds, radii
from tests.topk_oracle import v0_dist2

EINVAL = -1
CELL_BATCH = 1024
BASE = dict(k=16, m=96, n=1 << 20, radius_finite=1, flag_grid=0, flag_cells=0, has_grid=0, has_cells=0, centred=0, rows_u8=0, bins=0,
            sharded=0, path=0, cells=0, num_cu=256, radius_rings=0)


def slices_of(m, n, num_cu):
    """The exact count scan's slices for the call's first chunk of queries: about 32 waves per CU, at least 1024 rows each."""
    qg = -(-min(m, 65536) // 64)
    s = max(1, min(num_cu * 32 // qg, (n + 1023) // 1024, 65535))
    per = -(-n // s)
    return -(-n // per)


def expect(i):
    """The route of the issue, restated: {way, passes, pass_m, scratch_bytes}."""
    if i["has_grid"] and i["flag_grid"] and i["path"] in (0, 3):
        return dict(way=3, passes=0, pass_m=0, scratch_bytes=4 * i["m"])
    one_frame = i["has_cells"] and not i["centred"] and (not i["rows_u8"] or i["bins"])
    if (i["flag_cells"] and i["radius_finite"] and one_frame and i["k"] <= 32 and i["m"] >= 5 and i["path"] in (0, 2) and
            i["cells"] != 2):
        return dict(way=4, passes=-(-i["m"] // CELL_BATCH), pass_m=min(i["m"], CELL_BATCH), scratch_bytes=4 * i["m"])
    return dict(way=1, passes=0, pass_m=0, scratch_bytes=0)


def check(i):
    got = pkg.debug_count_plan(**i)
    want = expect(i)
    assert {n: got[n] for n in want} == want, (i, got)
    assert got["slices"] == slices_of(i["m"], i["n"], i["num_cu"]), (i, got)
    if want["way"] == 3:
        rings = i["radius_rings"] if i["radius_finite"] else 0
        g = pkg.debug_grid_within_plan(k=i["k"], K=1, m=i["m"], has_grid=1, path=i["path"], flag=1, radius_rings=rings)
        assert (got["rmax"], got["blocks"], got["waves"]) == (g["rmax"], g["blocks"], g["waves"]), (i, got, g)
        assert got["blocks"] == -(-i["m"] // 4) and got["waves"] == 4
    else:
        assert (got["rmax"], got["blocks"], got["waves"]) == (0, 0, 0), (i, got)
    return got


def test_the_default_is_the_exact_count_and_a_flag_without_the_structure_changes_nothing():
    assert check(BASE)["way"] == 1
    for flags in itertools.product((0, 1), repeat=2):
        for radius_finite in (0, 1):
            got = check(dict(BASE, flag_grid=flags[0], flag_cells=flags[1], radius_finite=radius_finite))
            assert got["way"] == 1 and got["scratch_bytes"] == 0
    # the structures without a flag: every call without a flag takes the exact count
    assert check(dict(BASE, k=3, has_grid=1))["way"] == 1
    assert check(dict(BASE, has_cells=1))["way"] == 1
    assert check(dict(BASE, has_cells=1, rows_u8=1, bins=1, sharded=1))["way"] == 1


def test_the_grid_way_needs_the_index_the_flag_and_path_0_or_3():
    for k, m, path, radius_finite, rings in itertools.product((1, 2, 3, 4), (1, 3, 70, 5000), (0, 1, 2, 3), (0, 1),
                                                              (0, 1, 7, 16383, 16384, 1 << 30)):
        for has_grid, flag in itertools.product((0, 1), repeat=2):
            got = check(dict(BASE, k=k, m=m, n=16384, path=path, radius_finite=radius_finite, radius_rings=rings, has_grid=has_grid,
                             flag_grid=flag))
            assert (got["way"] == 3) == bool(has_grid and flag and path in (0, 3))
    # rmax follows the radius while the walk stays within the 2^15-cell budget, and +INF has no rings to follow
    plain = pkg.debug_grid_topk_plan(k=1, K=1, m=70, has_grid=1, path=0, flag=1)["rmax"]
    g = dict(BASE, k=1, m=70, n=16384, has_grid=1, flag_grid=1)
    assert check(dict(g, radius_rings=16383))["rmax"] == 16383
    assert check(dict(g, radius_rings=16384))["rmax"] == plain
    assert check(dict(g, radius_rings=16383, radius_finite=0))["rmax"] == plain
    assert check(dict(g, k=3, radius_rings=15))["rmax"] == 15 and check(dict(g, k=3, radius_rings=16))["rmax"] == \
        pkg.debug_grid_topk_plan(k=3, K=1, m=70, has_grid=1, path=0, flag=1)["rmax"]


def test_the_cell_way_needs_the_flag_a_finite_radius_and_a_one_frame_layout():
    seen = set()
    for k, m, path, cells in itertools.product((16, 20, 32, 33), (1, 4, 5, 96, 1024, 1030), (0, 1, 2, 3), (0, 1, 2)):
        for flag, radius_finite, has_cells, centred, rows_u8, bins, sharded in itertools.product((0, 1), repeat=7):
            if bins and not rows_u8:
                continue
            got = check(dict(BASE, k=k, m=m, path=path, cells=cells, flag_cells=flag, radius_finite=radius_finite, has_cells=has_cells,
                             centred=centred, rows_u8=rows_u8, bins=bins, sharded=sharded))
            seen.add(got["way"])
    assert seen == {1, 4}
    fp16 = dict(BASE, flag_cells=1, has_cells=1)
    assert check(fp16)["way"] == 4
    two = check(dict(fp16, m=1030))
    assert (two["passes"], two["pass_m"], two["scratch_bytes"]) == (2, 1024, 4 * 1030)
    assert check(dict(fp16, rows_u8=1, bins=1))["way"] == 4            # 8-bit rows in bin frames: the shard's one frame
    assert check(dict(fp16, sharded=1))["way"] == 4                    # cell-range shards as they are: no PARTIAL flag
    assert check(dict(fp16, radius_finite=0))["way"] == 1              # +INF under the cell flag
    assert check(dict(fp16, centred=1))["way"] == 1                    # per-cell frames (fp16 ...
    assert check(dict(fp16, centred=1, rows_u8=1))["way"] == 1         # ... and 8-bit rows in each cell's own frame)
    assert check(dict(fp16, rows_u8=1))["way"] == 1
    assert check(dict(fp16, has_cells=0))["way"] == 1                  # the dense filter layouts
    assert check(dict(fp16, m=4))["way"] == 1 and check(dict(fp16, m=5))["way"] == 4
    assert check(dict(fp16, k=33))["way"] == 1 and check(dict(fp16, k=32))["way"] == 4
    assert check(dict(fp16, cells=2))["way"] == 1 and check(dict(fp16, cells=1))["way"] == 4
    assert check(dict(fp16, path=1))["way"] == 1 and check(dict(fp16, path=3))["way"] == 1 and check(dict(fp16, path=2))["way"] == 4
    # both flags on an index with a grid index: the grid answers (such an index has no layouts)
    assert check(dict(BASE, k=3, has_grid=1, flag_grid=1, flag_cells=1))["way"] == 3


def test_bad_plan_inputs_are_einval():
    L = pkg.lib()
    f = L.knn_debug_count_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    out = (ctypes.c_longlong * 8)()

    def rc(**change):
        i = dict(BASE, **change)
        return f((ctypes.c_longlong * 16)(*[int(i[n]) for n in pkg.COUNT_PLAN_INPUTS]), out)

    assert rc() == 0
    for bad in (dict(k=0), dict(k=4097), dict(m=0), dict(m=1 << 31), dict(n=0), dict(radius_finite=2), dict(flag_grid=2),
                dict(flag_cells=-1), dict(has_grid=1), dict(k=3, has_grid=1, sharded=1), dict(has_cells=2), dict(centred=2),
                dict(rows_u8=2), dict(bins=2), dict(sharded=2), dict(path=4), dict(path=-1), dict(cells=3), dict(num_cu=0),
                dict(radius_rings=-1)):
        assert rc(**bad) == EINVAL, bad
        assert b"knn_debug_count_plan" in L.knn_last_error()
    assert f(None, out) == EINVAL and f((ctypes.c_longlong * 16)(), None) == EINVAL
    with pytest.raises(pkg.KnnError, match="knn_debug_count_plan"):
        pkg.debug_count_plan(**dict(BASE, m=0))


def test_the_entry_points_argument_errors_need_no_gpu():
    """Every rule has its own knn_last_error text and the index is looked at last, so the rules show without an index: nothing
    behind them is reached (the pointers here are never read)."""
    L = pkg.lib()
    vp = ctypes.c_void_p
    q, c = vp(0x1000), vp(0x2000)
    init, grid, cells = pkg.QUERY_INIT_KEYS, pkg.QUERY_COUNT_GRID, pkg.QUERY_COUNT_CELLS
    assert (grid, cells) == (16, 32)

    def rc(slot=0, m=7, queries=q, r2=1.0, counts=c, flags=init):
        return pkg.count_within_c()(None, slot, m, queries, r2, counts, None, flags), L.knn_last_error().decode()

    assert rc() == (EINVAL, "knn_index_count_within: null index")
    for flags in (0, init, grid, cells, init | grid | cells):
        assert rc(flags=flags)[1].endswith("null index")
    for flags in (2, 4, 8, 64, 1 << 31, init | 2, grid | 8):          # the top-K flags among them: not admitted here
        code, text = rc(flags=flags)
        assert code == EINVAL and "unknown flag" in text, (flags, text)
    for bad in (-1.0, -1e-30, float("nan"), -float("inf")):
        code, text = rc(r2=bad)
        assert code == EINVAL and "max_dist2" in text, (bad, text)
    for r2 in (0.0, -0.0, float("inf")):
        assert rc(r2=r2)[1].endswith("null index")
    for slot in (8, -1):
        code, text = rc(slot=slot)
        assert code == EINVAL and "slot" in text
    for m in (0, -3):
        code, text = rc(m=m)
        assert code == EINVAL and "m < 1" in text
    for kw in (dict(queries=None), dict(counts=None)):
        code, text = rc(**kw)
        assert code == EINVAL and "null queries or counts" in text
    host = np.zeros(4, dtype=np.uint32)
    Q = np.zeros((4, 3), dtype=np.float32)
    L.knn_index_count_within_host.argtypes = [vp, ctypes.c_int, vp, ctypes.c_float, vp]
    for args in ((None, 4, Q.ctypes.data_as(vp), 1.0, host.ctypes.data_as(vp)),):
        assert L.knn_index_count_within_host(*args) == EINVAL
        assert b"knn_index_count_within_host" in L.knn_last_error()


def test_the_oracle_on_a_hand_made_case():
    """k = 2, five rows: an ordinary one, a NaN row, a +INF row, a row whose distance overflows (3e38), and a second row at the
    first one's distance from query 0 (a boundary tie).  By hand: query 0 = (0, 0); rows (3, 4) and (-4, 3) are both at 25."""
    R = np.array([[3, 4], [np.nan, 0], [np.inf, 1], [3e38, 3e38], [-4, 3], [0, 1]], dtype=np.float32)
    Q = np.array([[0, 0], [3, 4], [np.nan, 0]], dtype=np.float32)
    d = v0_dist2(Q, R, 2)
    assert d[0, 0] == 25 and d[0, 4] == 25 and np.isnan(d[0, 1]) and np.isinf(d[0, 2]) and np.isinf(d[0, 3]) and d[0, 5] == 1
    below = float(np.nextafter(np.float32(25), np.float32(0)))
    for r2, want in ((25.0, [3, 2, 0]), (below, [1, 2, 0]), (0.0, [0, 1, 0]), (-0.0, [0, 1, 0]), (float("inf"), [3, 3, 0]),
                     (0.5, [0, 1, 0]), (1.0, [1, 1, 0]), (3e38, [3, 3, 0])):
        np.testing.assert_array_equal(counts_of(d, r2), np.array(want, dtype=np.uint32), err_msg=str(r2))
        np.testing.assert_array_equal(counts(Q, R, 2, r2, chunk=2), np.array(want, dtype=np.uint32), err_msg=str(r2))
    assert counts_of(d, 25.0).dtype == np.uint32
    # (query 1: (3, 4) itself; (-4, 3) at 49 + 1 = 50; (0, 1) at 9 + 9 = 18)
    assert kinds(d, 25.0) == (True, True, False)


def test_the_radii_come_from_the_distances_and_say_what_they_claim():
    rng = np.random.default_rng(3)
    k, n, m = 3, 500, 40
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Q[:, 0] += np.linspace(0.0, 1.5, m, dtype=np.float32)
    d = v0_dist2(Q, R, k)
    rs = dict(radii(d))
    assert list(rs) == ["at", "below", "zero", "inf", "under_all", "large"]
    assert (d == np.float32(rs["at"])).any() and rs["below"] < rs["at"] and rs["zero"] == 0.0 and rs["inf"] == float("inf")
    for name in ("at", "below"):
        z, p, _ = kinds(d, rs[name])
        assert z and p
    assert (counts_of(d, rs["at"]) != counts_of(d, rs["below"])).any()
    assert (counts_of(d, rs["under_all"]) == 0).all() and (counts_of(d, rs["inf"]) == n).all()
    assert kinds(d, rs["large"])[2] and counts_of(d, rs["large"]).max() >= 100
    with pytest.raises(AssertionError):
        radii(v0_dist2(R[:3], R, k))      # the queries coincide with rows: nothing is below every distance
