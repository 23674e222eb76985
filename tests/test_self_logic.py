"""Queries about the shard's own rows (knn_index_self_topk, knn_index_self_count_within, knn_index_self_list_within;
include/knn_mi355x.h 2i) without a GPU: the exported names, the argument rules of the three device calls in the header's order, the
call's plan (knn_debug_self_plan) against the plain scans' own hooks, and the cut of a slice around a block's window of own rows
(knn_debug_self_ranges, the kernels' own lines in csrc/knn_self_window.h)."""
import ctypes
import os
import re

import pytest

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
INT_MAX = 2**31 - 1
CHUNK = 65536
CUS = 256
vp = ctypes.c_void_p
NAMES = ("knn_index_self_topk", "knn_index_self_count_within", "knn_index_self_list_within", "knn_index_self_topk_host",
         "knn_index_self_list_within_host", "knn_debug_self_plan", "knn_debug_self_ranges")
INIT, PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS = 1, 2, 4, 8, 16, 32


def test_the_seven_names_are_declared_under_2i_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    at = header.index("2i. Queries about the shard's own rows")
    assert at > header.index("2h. Lists within a radius and top-K beyond 64 over a subset of the rows")
    for name in NAMES:
        m = re.search(r"^int %s\s*\(" % name, header, flags=re.M)
        assert m and m.start() > at, name
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    for name in ("self_topk_c", "self_count_within_c", "self_list_within_c", "self_topk_host_c", "self_list_within_host_c",
                 "debug_self_plan", "debug_self_ranges"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("self_topk", "self_count_within", "self_list_within", "self_topk_host", "self_list_within_host"):
        assert callable(getattr(pkg.KnnIndex, name)), name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for proto in (
            "int knn_index_self_topk(knn_index *idx, int slot, long long row_first, int rows, int K, float max_dist2, "
            "unsigned long long *keys_dev , int *indices_dev , void *stream, unsigned flags);",
            "int knn_index_self_count_within(knn_index *idx, int slot, long long row_first, int rows, float max_dist2, "
            "unsigned *counts_dev , void *stream, unsigned flags);",
            "int knn_index_self_list_within(knn_index *idx, int slot, long long row_first, int rows, float max_dist2, "
            "const unsigned long long *offsets_dev , unsigned *fill_dev , unsigned long long *keys_dev, void *stream, unsigned flags);",
            "int knn_index_self_topk_host(knn_index *idx, int K, float max_dist2, int *indices_host , float *dist2_host , "
            "int *counts_host );",
            "int knn_index_self_list_within_host(knn_index *idx, float max_dist2, long long *offsets_host , int **indices_out, "
            "float **dist2_out );",
            "int knn_debug_self_plan(const long long in[6], long long out[8]);",
            "int knn_debug_self_ranges(long long i0, long long i1, long long w0, long long w1, long long out[6]);"):
        assert proto in flat, proto


def _walk(who, rc, steps):
    """steps: (keyword overrides that break ONE more rule than the step before, the text that must speak).  Every earlier rule's
    breakage is mended in turn, so each text shows alone, in the header's order; the index — null throughout — speaks last but
    one, and the rule that needs the index cannot be reached without one."""
    broken = {}
    for over, _ in steps:
        broken.update(over)
    for i, (over, text) in enumerate(steps):
        assert rc(**broken) == (EINVAL, who + text), (who, text)
        for key in over:                      # mend this rule: the next one speaks
            del broken[key]
    assert not broken
    assert rc() == (EINVAL, who + "null index")


def test_the_top_k_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    k = vp(0x3000)

    def rc(slot=0, row_first=0, rows=7, K=8, r2=1.0, keys=k, flags=INIT):
        return pkg.self_topk_c()(None, slot, row_first, rows, K, r2, keys, None, None, flags), L.knn_last_error().decode()

    who = "knn_index_self_topk: "
    _walk(who, rc, [
        (dict(r2=-1.0), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=PARTIAL), "unknown flag (KNN_QUERY_INIT_KEYS, KNN_QUERY_TOPK_GRID, KNN_QUERY_TOPK_FRAMES)"),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(rows=0), "rows < 1"),
        (dict(row_first=-1), "row_first < 0"),
        (dict(K=65), "K outside 1 .. 64"),
        (dict(keys=None), "null keys"),
    ])
    assert rc(r2=float("nan"))[1] == who + "max_dist2 must be >= 0 and not NaN"
    assert rc(r2=-0.0) == (EINVAL, who + "null index") and rc(r2=float("inf")) == (EINVAL, who + "null index")
    for flags in (PARTIAL, COUNT_GRID, COUNT_CELLS, 64, 1 << 31, INIT | PARTIAL, GRID | COUNT_GRID):
        assert rc(flags=flags)[1].startswith(who + "unknown flag"), flags
    for flags in (0, INIT, GRID, FRAMES, INIT | GRID | FRAMES):
        assert rc(flags=flags) == (EINVAL, who + "null index"), flags
    assert rc(slot=-1)[1] == who + "slot outside 0 .. 7" and rc(rows=-5)[1] == who + "rows < 1"
    assert rc(K=0)[1] == who + "K outside 1 .. 64" and rc(K=64) == (EINVAL, who + "null index")
    # rows * K: behind K, ahead of the pointers
    assert rc(rows=INT_MAX // 8 + 1, K=8, keys=None)[1] == who + "rows * K above INT_MAX"
    assert rc(rows=INT_MAX // 8, K=8, keys=None)[1] == who + "null keys"
    assert rc(rows=INT_MAX // 8 + 1, K=65)[1] == who + "K outside 1 .. 64"


def test_the_count_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    c = vp(0x3000)

    def rc(slot=0, row_first=0, rows=7, r2=1.0, counts=c, flags=INIT):
        return pkg.self_count_within_c()(None, slot, row_first, rows, r2, counts, None, flags), L.knn_last_error().decode()

    who = "knn_index_self_count_within: "
    _walk(who, rc, [
        (dict(r2=float("nan")), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=GRID), "unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)"),
        (dict(slot=-1), "slot outside 0 .. 7"),
        (dict(rows=0), "rows < 1"),
        (dict(row_first=-1), "row_first < 0"),
        (dict(counts=None), "null counts"),
    ])
    for flags in (PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS, 64, 1 << 31, INIT | COUNT_GRID):
        assert rc(flags=flags)[1].startswith(who + "unknown flag"), flags
    assert rc(flags=0) == (EINVAL, who + "null index")


def test_the_list_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    o, f, k = vp(0x1000), vp(0x2000), vp(0x3000)

    def rc(slot=0, row_first=0, rows=7, r2=1.0, offsets=o, fill=f, keys=k, flags=INIT):
        return (pkg.self_list_within_c()(None, slot, row_first, rows, r2, offsets, fill, keys, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_self_list_within: "
    _walk(who, rc, [
        (dict(r2=-0.5), "max_dist2 must be >= 0 and not NaN"),
        (dict(flags=COUNT_CELLS), "unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)"),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(rows=-1), "rows < 1"),
        (dict(row_first=-7), "row_first < 0"),
        (dict(offsets=None), "null offsets, fill or keys"),
    ])
    assert rc(fill=None)[1] == who + "null offsets, fill or keys" and rc(keys=None)[1] == who + "null offsets, fill or keys"
    for flags in (PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS, 64, 1 << 31, INIT | PARTIAL):
        assert rc(flags=flags)[1].startswith(who + "unknown flag"), flags
    assert rc(flags=0) == (EINVAL, who + "null index")


def test_the_host_calls_reject_their_bad_arguments_without_a_gpu():
    L = pkg.lib()
    p = vp(0x1000)
    ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
    who = "knn_index_self_topk_host: "
    f = pkg.self_topk_host_c()
    for args, text in (((None, 8, -1.0, p, None, None), "max_dist2 must be >= 0 and not NaN"), ((None, 0, 1.0, p, None, None), "K outside 1 .. 64"),
                       ((None, 65, 1.0, p, None, None), "K outside 1 .. 64"), ((None, 8, 1.0, None, None, None), "null indices"),
                       ((None, 8, 1.0, p, None, None), "null index")):
        assert (f(*args), L.knn_last_error().decode()) == (EINVAL, who + text)
    who = "knn_index_self_list_within_host: "
    g = pkg.self_list_within_host_c()
    for args, text in (((None, float("nan"), p, ctypes.byref(ind), ctypes.byref(d2)), "max_dist2 must be >= 0 and not NaN"),
                       ((None, 1.0, None, ctypes.byref(ind), ctypes.byref(d2)), "null offsets or indices"),
                       ((None, 1.0, p, None, ctypes.byref(d2)), "null offsets or indices"),
                       ((None, 1.0, p, ctypes.byref(ind), None), "null index")):
        assert (g(*args), L.knn_last_error().decode()) == (EINVAL, who + text)


@pytest.mark.parametrize("rows", [1, 64, 65, 65536, 65537])
@pytest.mark.parametrize("K", [0, -1, 1, 17, 64])
def test_the_plan_is_the_plain_scans_plan_for_the_same_numbers(rows, K):
    """Chunks, slices, LDS and list bytes are what the plain exact scans — and the masked ones, which restate them — plan for
    `rows` queries: the slot's buffers are sized as before."""
    for k, n in ((16, 1 << 20), (3, 70000), (129, max(rows, 3149))):
        for init in (0, 1):
            p = pkg.debug_self_plan(k=k, rows=rows, K=K, shard_rows=n, num_cu=CUS, init=init)
            plain = pkg.debug_masked_plan(k=k, m=rows, K=max(K, 0), rows=n, num_cu=CUS, init=init)
            first = min(rows, CHUNK)
            assert p["chunks"] == plain["chunks"] == (rows + CHUNK - 1) // CHUNK
            assert p["chunk_rows"] == plain["chunk_m"] == first
            assert p["groups"] == (first + 63) // 64
            assert p["slices"] == plain["slices"] and 1 <= p["slices"] <= (n + 1023) // 1024
            assert p["lds_bytes"] == plain["lds_bytes"] == (max(K, 0) * 64 * 8)
            assert p["part_bytes"] == plain["part_bytes"]
            assert p["launches"] == p["chunks"] * (2 if K > 0 else 1)
            if K > 0:
                scratch = pkg.debug_topk_scratch(way=1, m=rows, K=K, n=n, num_cu=CUS, init=init, within=0, pass_m=0, grid_scratch_bytes=0)
                assert p["part_bytes"] >= scratch["part_bytes"] >= p["slices"] * first * K * 8 > 0
                if p["chunks"] == 1:
                    assert p["part_bytes"] == scratch["part_bytes"] == p["slices"] * first * K * 8
            else:
                count = pkg.debug_count_plan(k=k, m=rows, n=n, radius_finite=1, flag_grid=0, flag_cells=0, has_grid=0, has_cells=0, centred=0,
                                             rows_u8=0, bins=0, sharded=0, path=0, cells=0, num_cu=CUS, radius_rings=0)
                assert p["slices"] == count["slices"] and p["part_bytes"] == 0
            through = 0 if K < 1 or K == 64 else rows * (K + 1) * 8 + (0 if init else rows * K * 8)
            assert p["through_bytes"] == through


def test_the_plan_rejects_bad_inputs():
    ok = dict(k=16, rows=100, K=8, shard_rows=5000, num_cu=CUS, init=1)
    pkg.debug_self_plan(**ok)
    for bad in (dict(k=0), dict(rows=0), dict(K=-2), dict(K=65), dict(shard_rows=99), dict(num_cu=0), dict(init=2),
                dict(rows=INT_MAX // 8 + 1, shard_rows=1 << 31)):
        with pytest.raises(pkg.KnnError, match="knn_debug_self_plan: bad arguments"):
            pkg.debug_self_plan(**{**ok, **bad})


WINDOWS = [
    ("before the slice", 1000, 2000, 100, 164),
    ("ending where the slice begins", 1000, 2000, 936, 1000),
    ("after the slice", 1000, 2000, 2500, 2564),
    ("beginning where the slice ends", 1000, 2000, 2000, 2064),
    ("inside", 1000, 2000, 1500, 1564),
    ("at the slice's first rows", 1000, 2000, 1000, 1064),
    ("at the slice's last rows", 1000, 2000, 1936, 2000),
    ("covering the slice", 1010, 1040, 1000, 1064),
    ("exactly the slice", 1000, 1064, 1000, 1064),
    ("straddling the first end", 1000, 2000, 990, 1054),
    ("straddling the last end", 1000, 2000, 1990, 2054),
    ("empty, inside", 1000, 2000, 1500, 1500),
    ("empty, outside", 1000, 2000, 10, 10),
    ("inverted", 1000, 2000, 1600, 1500),
    ("a short last window", 0, 3149, 3136, 3149),
    ("an empty slice", 700, 700, 690, 754),
    ("beyond 2^32", (1 << 32) - 10, (1 << 32) + 100, (1 << 32) - 3, (1 << 32) + 61),
]


@pytest.mark.parametrize("name,i0,i1,w0,w1", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_the_cut_around_the_window_is_exact_disjoint_and_ascending(name, i0, i1, w0, w1):
    r = pkg.debug_self_ranges(i0, i1, w0, w1)
    # ascending, touching: three disjoint ranges whose union is the slice
    assert r["b0"] == i0 and r["a1"] == max(i1, i0)
    assert r["b0"] <= r["b1"] == r["w0"] <= r["w1"] == r["a0"] <= r["a1"]
    # the middle range is exactly the window's rows that lie in the slice
    lo, hi = max(i0, w0), min(i1, w1)
    if lo < hi:
        assert (r["w0"], r["w1"]) == (lo, hi)
    else:
        assert r["w0"] == r["w1"]
    if i1 - i0 <= 4096 and i1 > i0:   # row by row
        want = [("w" if w0 <= i < w1 else "b" if i < w0 else "a") for i in range(i0, i1)]
        got = ["b"] * (r["b1"] - r["b0"]) + ["w"] * (r["w1"] - r["w0"]) + ["a"] * (r["a1"] - r["a0"])
        if w1 > w0:
            assert got == want
        else:
            assert "w" not in got and len(got) == len(want)


def test_every_block_of_a_call_cuts_its_slice_around_its_own_window():
    """The grid of one call: slices along the shard, windows of 64 along the call's rows — over all blocks every (query, row) pair
    with row = the query's own lies in some block's middle range, and only windows' rows do."""
    n, first, rows = 3149, 2090, 150
    slices = pkg.debug_self_plan(k=16, rows=rows, K=8, shard_rows=n, num_cu=CUS, init=1)["slices"]
    per = (n + slices - 1) // slices
    assert slices >= 3 and per % 64 != 0
    for g in range((rows + 63) // 64):
        w0, w1 = first + 64 * g, min(first + 64 * g + 64, first + rows)
        inside = []
        for s in range(slices):
            r = pkg.debug_self_ranges(s * per, min(n, s * per + per), w0, w1)
            inside += list(range(r["w0"], r["w1"]))
        assert inside == list(range(w0, w1))
