"""Which path answers a call (knn_query_route) and what an index is built with (knn_index_build_plan), the parts that need no
GPU: both plans against their rules restated here (DESIGN, "which path answers a call"), through knn_debug_query_route and
knn_debug_index_build_plan.  The restatements are written from the rules, not from the C code: a change to either side has to be
made in both places."""
import ctypes
import itertools
import os
import sys

import pytest

from tests.test_cells_topk_logic import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT, FILTER, GRID, CELLS = 1, 2, 3, 4


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import multicore_hw2_amd as p
    if not os.path.exists(p.lib_path):
        import __graft_entry__ as g
        g.build()
    return p


def _kt(k):
    return 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8


def _ccap(K, m):
    return min(4096 + 128 * K, (32 << 20) // m)


def _topk_cells_use(k, K, m, topk_cells, has_cells, centred, rows_u8, bins, sharded, other_path, n_outliers):
    """knn_cells_topk_plan's `use` (tests/test_cells_topk_logic.py checks the plan itself): the layout and the call allow it, and
    the option asks for it — the policy (0) declines everywhere for now."""
    layout = has_cells and (sharded != 1) and not other_path and not centred and (not rows_u8 or bins) and k <= 32
    call = m >= 5 and _ccap(K, m) >= 64 and n_outliers <= _ccap(K, m) // 2
    return bool(layout and call and topk_cells == 1)


def _route(k, K, m, n, path, cells, topk_cells, filter_usable, has_cells, centred, rows_u8, bins, has_grid, sharded, filter_wanted,
           n_outliers, init_keys):
    """(way, fill_keys_first, ccap): the issue's rules.  sharded: 0, 1, 2 = with KNN_QUERY_TOPK_PARTIAL."""
    grid_serves = has_grid and path in (0, 3)
    sized = n >= 65536 or filter_wanted
    if K == 0:
        if grid_serves:
            way = GRID
        else:
            cells_live = has_cells and (cells != 2 or sharded)
            use_filter = sharded or (filter_usable and (path == 2 or (path == 0 and (m >= 5 or cells_live) and sized)))
            if use_filter:
                way = CELLS if has_cells and _kt(k) <= 2 and (sharded or cells != 2 or centred) else FILTER
            else:
                way = EXACT
        return way, int(bool(init_keys and way in (EXACT, GRID))), 0
    ccap = _ccap(K, m)
    other_path = grid_serves or path in (1, 3)
    if _topk_cells_use(k, K, m, topk_cells, has_cells, centred, rows_u8, bins, sharded, other_path, n_outliers):
        way = CELLS
    elif (not sharded and filter_usable and not grid_serves and not (has_cells and (centred or rows_u8)) and
          n_outliers <= ccap // 2 and ccap >= 64 and (path == 2 or (path == 0 and m >= 5 and sized))):
        way = FILTER
    else:
        way = EXACT
    return way, 0, ccap


# (filter_usable, has_cells, centred, rows_u8, bins): the four cell-sorted layouts, the dense layouts ("no cells"), no layouts at all
INDEX_LAYOUTS = dict({name: (1, 1) + flags for name, flags in LAYOUTS.items()}, dense=(1, 0, 0, 0, 0), none=(0, 0, 0, 0, 0))
SCAN = dict(ncells=512, nitems=519, cap=384, several_slots=0, scan_blocks=0, scan_deal=0, num_cu=256, rec_cap=1 << 22)
MS = (1, 4, 5, 1024, 1025, 600000)      # (600000: ccap = 55, below 64)
NS = (1000, 4096, 65535, 65536, 1 << 20)
KDIMS = (3, 16, 17, 32, 33, 40)


def test_route_follows_the_rules_over_the_whole_product(pkg):
    names = pkg.QUERY_ROUTE_INPUTS
    at = {name: i for i, name in enumerate(names)}
    vin = (ctypes.c_longlong * len(names))()
    out = (ctypes.c_longlong * len(pkg.QUERY_ROUTE))()
    for name, v in SCAN.items():
        vin[at[name]] = v
    f = pkg.lib().knn_debug_query_route
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    i_m, i_no, i_n, i_k = at["m"], at["n_outliers"], at["n"], at["k"]
    ways = set()
    calls = 0
    outer = itertools.product(range(4), range(3), range(3), (0, 1, 8, 64), INDEX_LAYOUTS.values(), (0, 1), (0, 1, 2), (0, 1))
    for path, cells, topk_cells, K, (usable, has_cells, centred, rows_u8, bins), has_grid, sharded, filter_wanted in outer:
        if has_grid and sharded:      # the inputs' invariant: knn_index_create_sharded never builds a grid index
            continue
        init_keys = (path + cells + K) & 1 if not sharded else 1
        for name, v in (("path", path), ("cells", cells), ("topk_cells", topk_cells), ("K", K), ("filter_usable", usable),
                        ("has_cells", has_cells), ("centred", centred), ("rows_u8", rows_u8), ("bins", bins), ("has_grid", has_grid),
                        ("sharded", sharded), ("filter_wanted", filter_wanted), ("init_keys", init_keys)):
            vin[at[name]] = v
        for k in KDIMS:
            vin[i_k] = k
            for n in NS:
                vin[i_n] = n
                for m in MS:
                    vin[i_m] = m
                    half = _ccap(max(K, 1), m) // 2
                    for n_outliers in (half, half + 1):
                        vin[i_no] = n_outliers
                        assert f(vin, out) == 0
                        calls += 1
                        want = _route(k, K, m, n, path, cells, topk_cells, usable, has_cells, centred, rows_u8, bins, has_grid,
                                      sharded, filter_wanted, n_outliers, init_keys)
                        if (out[0], out[1], out[2]) != want:
                            raise AssertionError((dict(zip(names, list(vin))), list(out), want))
                        assert out[3] == int(K > 0 and out[0] == CELLS)      # the plan's `use` is the CELLS way of a top-K call
                        if out[1]:
                            assert out[0] in (EXACT, GRID)                   # the filter ways start their keys themselves
                        ways.add((K > 0, out[0]))
    assert ways == {(False, EXACT), (False, FILTER), (False, GRID), (False, CELLS), (True, EXACT), (True, FILTER), (True, CELLS)}
    assert calls > 2_000_000


def _ask(pkg, **changes):
    base = dict(SCAN, k=8, K=0, m=5, n=1 << 17, path=0, cells=0, topk_cells=0, filter_usable=1, has_cells=1, centred=0, rows_u8=0,
                bins=0, has_grid=0, sharded=0, filter_wanted=0, n_outliers=0, init_keys=1)
    return pkg.debug_query_route(**dict(base, **changes))


def test_centred_layout_under_cells_2_is_exact_below_five_queries_and_pruned_from_five(pkg):
    """The known oddity knn_query_route's comment records: per-cell frames have no full scan to go to."""
    assert _ask(pkg, centred=1, cells=2, m=4)["way"] == EXACT
    assert _ask(pkg, centred=1, cells=2, m=5)["way"] == CELLS
    assert _ask(pkg, centred=1, cells=0, m=4)["way"] == CELLS      # (`cells` 0: one query already takes the pruned scan)
    assert _ask(pkg, centred=0, cells=2, m=4)["way"] == EXACT
    assert _ask(pkg, centred=0, cells=2, m=5)["way"] == FILTER     # (the shard's one frame: the full scan reads it)


def test_keys_are_never_filled_ahead_of_the_filter_ways(pkg):
    for way_inputs, way in ((dict(), CELLS), (dict(has_cells=0), FILTER), (dict(path=1), EXACT), (dict(has_grid=1, k=3), GRID)):
        for init in (0, 1):
            r = _ask(pkg, init_keys=init, **way_inputs)
            assert r["way"] == way and r["fill_keys_first"] == int(init and way in (EXACT, GRID)), (way_inputs, init, r)
    assert _ask(pkg, K=8, init_keys=1, path=1)["fill_keys_first"] == 0      # top-K: every way writes its lists itself


def test_topk_takes_the_cells_exactly_when_the_cells_topk_plan_says_use(pkg):
    seen = set()
    for k, K, m, n, topk_cells, cells, (lname, (centred, rows_u8, bins)), sharded, path, n_outliers in itertools.product(
            (8, 16, 20, 32, 33), (1, 8, 64), (4, 5, 1025, 600000), (1 << 17, 1 << 20), range(3), (0, 2), LAYOUTS.items(), (0, 1, 2),
            range(4), (0, 3000)):
        shape = dict(k=k, K=K, m=m, n=n, topk_cells=topk_cells, has_cells=1, centred=centred, rows_u8=rows_u8, bins=bins,
                     sharded=sharded, n_outliers=n_outliers, cells=cells)
        r = pkg.debug_query_route(**dict(SCAN, path=path, filter_usable=1, has_grid=0, filter_wanted=0, init_keys=1, **shape))
        p = pkg.debug_cells_topk_plan(**dict(SCAN, **shape))
        # (the plan's hook knows no `path`: a forced exact or grid path is the route's own veto)
        use = p["use"] and path in (0, 2)
        assert (r["way"] == CELLS) == bool(use) and r["topk_use"] == int(bool(use)), (shape, path, r, p)
        assert r["ccap"] == p["ccap"]
        if use:
            assert (r["passes"], r["pass_m"]) == (p["passes"], p["pass_m"])
        seen.add(bool(use))
    assert seen == {False, True}


def test_route_hook_rejects_what_the_entry_points_never_ask(pkg):
    for bad in (dict(n=0), dict(m=0), dict(K=65), dict(path=4), dict(cells=3), dict(topk_cells=3), dict(has_grid=1, sharded=1),
                dict(num_cu=0)):
        with pytest.raises(pkg.KnnError):
            _ask(pkg, **bad)


# ---- what an index is built with ---------------------------------------------------------------------------------------------

def _size_rule(k):
    return 1 << 19 if k <= 12 else 1 << 20 if k <= 16 else 1 << 22 if k <= 21 else 1 << 23 if k <= 23 else 1 << 24 if k <= 25 else 1 << 62


def _build_plan(k, n, on_device, build_filter, build_grid, path, cells, ingest, cells_build):
    filter_wanted = build_filter > 0
    want_cells = k <= 32 and n >= 1 << 17 and (cells == 1 or (cells == 0 and build_filter == 2) or
                                                (cells == 0 and build_filter < 0 and n >= _size_rule(k)))
    if build_filter < 0:
        build_filter = int(path == 2 or n >= 65536 or (32 < k <= 4096 and n >= 4096))
        filter_wanted = bool(build_filter) and n < 65536 and path != 2
    grid_planned = k <= 4 and (path == 3 or (path == 0 and build_grid != 0 and (build_grid > 0 or n >= 16384)))
    want_layouts = n > 0 and path not in (1, 3) and build_filter != 0
    form = 0
    if n > 0 and not on_device and want_layouts and not grid_planned and ingest != 1:
        form = 1 if not want_cells else 2 if cells_build == 0 else 0
    return dict(filter_wanted=int(filter_wanted), want_cells=int(want_cells), build_filter=build_filter, grid_planned=int(grid_planned),
                want_layouts=int(want_layouts), ingest=form)


def test_index_build_plan_follows_the_rules(pkg):
    forms = set()
    for k in (3, 4, 5, 12, 13, 16, 21, 25, 26, 32, 33, 4096, 4097):
        edges = [4096, 16384, 65536, 1 << 17] + ([_size_rule(k)] if k <= 25 else [])
        ns = [0] + [e - 1 for e in edges] + edges
        for n, on_device, build_filter, build_grid, path, cells, ingest, cells_build in itertools.product(
                ns, (0, 1), (-1, 0, 1, 2), (-1, 0, 1), range(4), range(3), (0, 1), range(3)):
            args = dict(k=k, n_local=n, refs_on_device=on_device, build_filter=build_filter, build_grid=build_grid, path=path,
                        cells=cells, ingest=ingest, cells_build=cells_build)
            got = pkg.debug_index_build_plan(**args)
            assert got == _build_plan(k, n, on_device, build_filter, build_grid, path, cells, ingest, cells_build), args
            forms.add(got["ingest"])
    assert forms == {0, 1, 2}
    with pytest.raises(pkg.KnnError):
        pkg.debug_index_build_plan(k=0, n_local=1, refs_on_device=0, build_filter=-1, build_grid=-1, path=0, cells=0, ingest=0,
                                   cells_build=0)


def test_size_rule_is_the_literal_the_one_shot_cost_model_had_for_k_up_to_16(pkg):
    """plan_shard wrote `rows >= (k <= 12 ? 2^19 : 2^20)`; it calls knn_cells_size_rule(k) now — the row count from which the
    library's policy builds the cell-sorted layout, seen here through the build plan's want_cells."""
    for k in range(1, 17):
        literal = 1 << 19 if k <= 12 else 1 << 20
        assert _size_rule(k) == literal
        for n, want in ((literal - 1, 0), (literal, 1)):
            got = pkg.debug_index_build_plan(k=k, n_local=n, refs_on_device=1, build_filter=-1, build_grid=-1, path=0, cells=0,
                                             ingest=0, cells_build=0)
            assert got["want_cells"] == want, (k, n)
