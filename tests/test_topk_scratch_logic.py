"""A workspace slot's top-K scratch: the sizes knn_topk_scratch_plan decides for a call, through
knn_debug_topk_scratch against a restatement of its rules.  No GPU."""
import ctypes
import itertools

import pytest

import multicore_hw2_amd as pkg

WAYS = (pkg.WAY_EXACT, pkg.WAY_FILTER, pkg.WAY_GRID, pkg.WAY_CELLS)
CELL_BATCH = 1024   # queries per pass of the cell-pruned way (KNN_CELL_BATCH)
MS = (1, 5, 1024, 1025, 2500)
KS = (1, 16, 64)
NUM_CU = 256


def _scratch(way, m, K, n=1 << 21, init=1, within=0):
    """The hook for a call as query_topk would state it: a pass of the cell-pruned way has min(m, 1024) queries, a grid call's
    lists are [m][K] keys."""
    return pkg.debug_topk_scratch(way=way, m=m, K=K, n=n, num_cu=NUM_CU, init=init, within=within,
                                  pass_m=min(m, CELL_BATCH) if way == pkg.WAY_CELLS else 0,
                                  grid_scratch_bytes=m * K * 8 if way == pkg.WAY_GRID else 0)


def _ccap(K, m):
    return min(4096 + 128 * K, (32 << 20) // m)


def test_cand_and_lists_match_their_rules():
    for way, init, within, m, K in itertools.product(WAYS, (0, 1), (0, 1), MS, KS):
        got = _scratch(way, m, K, init=init, within=within)
        filter_way = way in (pkg.WAY_FILTER, pkg.WAY_CELLS)
        if filter_way:
            cand = m * _ccap(K, m) * 8 + m * 4   # the lists, then the counters (which start at cand + m * ccap keys)
        elif way == pkg.WAY_GRID and not init:
            cand = m * K * 8
        else:
            cand = 0
        lists = m * K * 8 if within and filter_way else 0
        assert (got["cand_bytes"], got["lists_bytes"]) == (cand, lists), (way, init, within, m, K, got)
        assert got["part_bytes"] > 0


def test_part_of_the_cell_pruned_way_covers_the_call_a_pass_and_the_last_pass():
    for n, m, K in itertools.product((70000, 1 << 21), MS, KS):
        exact = lambda mm: _scratch(pkg.WAY_EXACT, mm, K, n=n)["part_bytes"]
        want = max([exact(m), exact(min(m, CELL_BATCH))] + ([exact(m % CELL_BATCH)] if m % CELL_BATCH else []))
        assert _scratch(pkg.WAY_CELLS, m, K, n=n)["part_bytes"] == want, (n, m, K)
        for way in (pkg.WAY_FILTER, pkg.WAY_GRID):
            assert _scratch(way, m, K, n=n)["part_bytes"] == exact(m), (way, n, m, K)


def test_part_does_not_shrink_from_1024_to_1025_queries():
    """The cell-pruned way: a call of 1025 queries still runs a pass of 1024, whose gated exact top-K needs what a call of 1024
    needs.  (Only this way: knn_topk_part_bytes itself is not monotonic in m — 1025 queries are 17 groups of 64 instead of 16, so
    the scan cuts the rows into fewer slices, 3944200 bytes after 4194304 at K 1 and 2^21 rows — and the other ways size `part` by
    it alone, at the m they launch with.)"""
    for n, K in itertools.product((70000, 1 << 21), KS):
        assert _scratch(pkg.WAY_CELLS, 1025, K, n=n)["part_bytes"] >= _scratch(pkg.WAY_CELLS, 1024, K, n=n)["part_bytes"], (n, K)
        assert _scratch(pkg.WAY_CELLS, 1025, K, n=n)["part_bytes"] >= _scratch(pkg.WAY_EXACT, 1024, K, n=n)["part_bytes"], (n, K)


@pytest.mark.parametrize("bad", [dict(m=0), dict(m=-3), dict(K=0), dict(K=65), dict(way=0), dict(way=5)])
def test_hook_rejects_bad_inputs(bad):
    inputs = dict(way=pkg.WAY_FILTER, m=100, K=8, n=1 << 20, num_cu=NUM_CU, init=1, within=0, pass_m=0, grid_scratch_bytes=0)
    inputs.update(bad)
    with pytest.raises(pkg.KnnError, match="knn_debug_topk_scratch"):
        pkg.debug_topk_scratch(**inputs)
    L = pkg.lib()
    vin = (ctypes.c_longlong * 9)(*[int(inputs[n]) for n in pkg.TOPK_SCRATCH_INPUTS])
    out = (ctypes.c_longlong * 3)()
    assert L.knn_debug_topk_scratch(vin, out) == -1   # KNN_EINVAL
    assert L.knn_debug_topk_scratch(None, None) != 0
