"""knn_index_list_within, knn_counts_to_offsets and knn_keys_sort_segments on the CPU: the symbols and their Python mirror exist,
every argument rule of the three device calls is KNN_EINVAL with its own knn_last_error text and is decided before an index or a
device is touched, and the numpy oracle the GPU tests expect from (tests/list_oracle.py) on a hand-made case."""
import ctypes

import numpy as np

import multicore_hw2_amd as pkg
from tests.count_oracle import counts_of
from tests.list_oracle import holds_every_kind, kinds, lengths, lists_of, offsets_of
from tests.topk_oracle import v0_dist2

EINVAL = -1
vp = ctypes.c_void_p


def test_the_symbols_and_the_python_mirror_exist():
    L = pkg.lib()
    for name in ("knn_counts_to_offsets", "knn_index_list_within", "knn_keys_sort_segments", "knn_index_list_within_host"):
        assert name in pkg.EXPORTED_SYMBOLS and hasattr(L, name), name
    for name in ("list_within", "list_within_host"):
        assert callable(getattr(pkg.KnnIndex, name)), name
    for name in ("counts_to_offsets", "keys_sort_segments", "list_within_c", "counts_to_offsets_c", "keys_sort_segments_c"):
        assert callable(getattr(pkg, name)), name
    with open(pkg.os.path.join(pkg.os.path.dirname(pkg._HERE), "include", "knn_mi355x.h")) as f:
        header = f.read()
    for name in ("knn_counts_to_offsets", "knn_index_list_within", "knn_keys_sort_segments", "knn_index_list_within_host"):
        assert "int %s(" % name in header, name


def test_the_list_call_argument_errors_need_no_gpu():
    """Every rule has its own text and the index is looked at last, so the rules show with a null index: nothing behind them is
    reached (the pointers here are never read)."""
    L = pkg.lib()
    q, o, f, k = vp(0x1000), vp(0x2000), vp(0x3000), vp(0x4000)
    init, grid, cells = pkg.QUERY_INIT_KEYS, pkg.QUERY_COUNT_GRID, pkg.QUERY_COUNT_CELLS

    def rc(slot=0, m=7, queries=q, r2=1.0, offsets=o, fill=f, keys=k, flags=init):
        return pkg.list_within_c()(None, slot, m, queries, r2, offsets, fill, keys, None, flags), L.knn_last_error().decode()

    assert rc() == (EINVAL, "knn_index_list_within: null index")
    for flags in (0, init, grid, cells, init | grid | cells):
        assert rc(flags=flags)[1].endswith("null index")
    for flags in (2, 4, 8, 64, 1 << 31, init | 2, grid | 8):          # the top-K flags among them: not admitted here
        code, text = rc(flags=flags)
        assert code == EINVAL and text.startswith("knn_index_list_within") and "unknown flag" in text, (flags, text)
    for bad in (-1.0, -1e-30, float("nan"), -float("inf")):
        code, text = rc(r2=bad)
        assert code == EINVAL and text.startswith("knn_index_list_within") and "max_dist2" in text, (bad, text)
    for r2 in (0.0, -0.0, float("inf")):
        assert rc(r2=r2)[1].endswith("null index")
    for slot in (8, -1):
        code, text = rc(slot=slot)
        assert code == EINVAL and text.startswith("knn_index_list_within") and "slot" in text
    for m in (0, -3):
        code, text = rc(m=m)
        assert code == EINVAL and text.startswith("knn_index_list_within") and "m < 1" in text
    for kw in (dict(queries=None), dict(offsets=None), dict(fill=None), dict(keys=None)):
        code, text = rc(**kw)
        assert code == EINVAL and text.startswith("knn_index_list_within") and "null queries, offsets, fill or keys" in text
    # the first rule that fails speaks: the radius before the flag, the flag before the slot, the slot before m, m before the pointers
    assert "max_dist2" in rc(r2=-1.0, flags=2, slot=9, m=0, queries=None)[1]
    assert "unknown flag" in rc(flags=2, slot=9, m=0, queries=None)[1]
    assert "slot" in rc(slot=9, m=0, queries=None)[1]
    assert "m < 1" in rc(m=0, queries=None)[1]


def test_the_offsets_and_the_sort_argument_errors_need_no_gpu():
    L = pkg.lib()
    a, b, c = vp(0x1000), vp(0x2000), vp(0x3000)
    for m in (0, -1):
        assert pkg.counts_to_offsets_c()(0, a, m, b, None) == EINVAL
        assert L.knn_last_error().decode() == "knn_counts_to_offsets: m < 1"
        assert pkg.keys_sort_segments_c()(0, m, a, b, c, None) == EINVAL
        assert L.knn_last_error().decode() == "knn_keys_sort_segments: m < 1"
    for args in ((0, None, 5, b, None), (0, a, 5, None, None)):
        assert pkg.counts_to_offsets_c()(*args) == EINVAL
        assert L.knn_last_error().decode() == "knn_counts_to_offsets: null counts or offsets"
    for args in ((0, 5, None, b, c, None), (0, 5, a, None, c, None), (0, 5, a, b, None, None)):
        assert pkg.keys_sort_segments_c()(*args) == EINVAL
        assert L.knn_last_error().decode() == "knn_keys_sort_segments: null offsets, fill or keys"
    # the host call: one rule for its arguments, a null index among them
    off = np.zeros(5, dtype=np.int64)
    Q = np.zeros((4, 3), dtype=np.float32)
    ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
    f = L.knn_index_list_within_host
    f.argtypes = [vp, ctypes.c_int, vp, ctypes.c_float, vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_int)),
                  ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    assert f(None, 4, Q.ctypes.data_as(vp), 1.0, off.ctypes.data_as(vp), ctypes.byref(ind), ctypes.byref(d2)) == EINVAL
    assert b"knn_index_list_within_host" in L.knn_last_error()


def test_a_list_call_takes_the_way_the_count_plan_names():
    """knn_debug_count_plan describes a list call too: its scratch bytes — [m] unsigned on the grid and cell ways — are the list
    call's scratch cursor."""
    base = dict(k=16, m=1030, n=1 << 20, radius_finite=1, flag_grid=0, flag_cells=1, has_grid=0, has_cells=1, centred=0, rows_u8=0,
                bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=0)
    got = pkg.debug_count_plan(**base)
    assert (got["way"], got["passes"], got["pass_m"], got["scratch_bytes"]) == (4, 2, 1024, 4 * 1030)
    assert pkg.debug_count_plan(**dict(base, flag_cells=0))["scratch_bytes"] == 0


def test_the_oracle_on_a_hand_made_case():
    """The rows of tests/test_count_logic.py's hand-made case: query 0 = (0, 0); rows (3, 4) and (-4, 3) are both at 25, (0, 1) at 1;
    a NaN row, a +INF row and a row whose distance overflows are never listed."""
    R = np.array([[3, 4], [np.nan, 0], [np.inf, 1], [3e38, 3e38], [-4, 3], [0, 1]], dtype=np.float32)
    Q = np.array([[0, 0], [3, 4], [np.nan, 0]], dtype=np.float32)
    d = v0_dist2(Q, R, 2)

    def key(dist, idx):
        return (np.uint64(np.float32(dist).view(np.uint32)) << np.uint64(32)) | np.uint64(idx)

    got = lists_of(d, 25.0, base=100)
    np.testing.assert_array_equal(got[0], np.array([key(1, 105), key(25, 100), key(25, 104)], dtype=np.uint64))
    np.testing.assert_array_equal(got[1], np.array([key(0, 100), key(18, 105)], dtype=np.uint64))
    assert got[2].size == 0 and got[0].dtype == np.uint64
    below = float(np.nextafter(np.float32(25), np.float32(0)))
    np.testing.assert_array_equal(lists_of(d, below)[0], np.array([key(1, 5)], dtype=np.uint64))
    np.testing.assert_array_equal(lists_of(d, 25.0, gids=[7, 8, 9, 10, 11, 12])[0], np.array([key(1, 12), key(25, 7), key(25, 11)],
                                                                                             dtype=np.uint64))
    for r2 in (25.0, below, 0.0, -0.0, float("inf"), 0.5, 3e38):
        np.testing.assert_array_equal(lengths(lists_of(d, r2)), counts_of(d, r2), err_msg=str(r2))
    np.testing.assert_array_equal(offsets_of([3, 0, 0xFFFFFFFF, 0xFFFFFFFF, 2]),
                                  np.array([0, 3, 3, 3 + 0xFFFFFFFF, 3 + 2 * 0xFFFFFFFF, 5 + 2 * 0xFFFFFFFF], dtype=np.uint64))
    assert kinds(got) == (True, True, False)
    assert not holds_every_kind([got]) and holds_every_kind([got, [np.zeros(65, np.uint64)]])
