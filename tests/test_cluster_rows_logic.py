"""What the GPU tests of the cluster call's forms and grid walks rest on (tests/test_cluster_forms_gpu.py,
test_cluster_grid_walks_gpu.py, test_cluster_streams_gpu.py), asserted from the oracle alone on the shards of tests/cluster_rows.py:
core, border and noise rows are all common, the planted structures come out, the sheet's distances round, the held radius flips
one row's core bit, and every grid shard has the grid its test takes it for — the cells per axis, the rings its radius spans, the
ring limit the plan gives that count, the largest cell.  No GPU."""
import numpy as np
import pytest

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co
from tests import cluster_rows as cr
from tests.cluster_helper import assert_planted
from tests.topk_oracle import v0_dist2

SHARE = {name: 0.10 if name.startswith("uniform_planted") else 0.04 for name in cr.GRID}
CELLS_PER_AXIS = {"uniform_planted2": 73, "uniform_planted4": 8, "gradient": 17, "column": 17, "blobs": 17, "offset": 73,
                  "dead_axis": 73, "strip": 147}


def rmax_of(k, n, rings):
    return pkg.debug_self_routed_plan(k=k, m=n, n=n, radius_finite=1, flag_grid=1, flag_cells=0, has_grid=1, has_cells=0, centred=0,
                                      rows_u8=0, bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=rings)["rmax"]


@pytest.mark.parametrize("k", cr.SHEET_KS)
def test_the_sheet_has_rows_of_every_kind_the_planted_block_and_distances_that_round(k):
    R, names, off = cr.sheet(k)
    assert R.shape == (cr.SHEET_N, k) and R.dtype == np.float32 and not R.flags.writeable and np.isfinite(R).all()
    assert 1 <= cr.SHEET_N % 64 <= 32                                       # the core kernel's last wave fills ONE word
    assert cr.sheet(k)[0] is R                                              # made once
    w = cr.want_sheet(k)
    s = cr.shares(w)
    print(f"sheet k={k}: core {s[0]:.3f} border {s[1]:.3f} noise {s[2]:.3f} of {cr.SHEET_N} rows, {np.unique(w['labels']).size - 1} "
          f"clusters, largest {cr.largest_cluster(w['labels'])}")
    assert min(s) >= 0.04, s
    assert_planted(w["labels"], w["core"], names, off, cr.SHEET_MIN_PTS)
    # min_pts = 1: every row is core, so the labels are components and nothing is noise
    w1 = cr.want_sheet(k, cr.SHEET_CAP, 1)
    assert w1["core"].all() and (w1["labels"] >= 0).all() and np.unique(w1["labels"]).size > 20
    # the distances round: the fp32 sum differs from the float64 sum of the same fp32 differences
    rows = np.arange(0, cr.SHEET_OFF, 2)
    d32 = v0_dist2(R[rows], R, k)
    R64 = R.astype(np.float64)
    d64 = np.zeros(d32.shape)
    for j in range(k):
        diff = R64[rows, j:j + 1] - R64[None, :, j]
        d64 += diff * diff
    others = rows[:, None] != np.arange(cr.SHEET_N)[None, :]
    rounded = (d32.astype(np.float64) != d64)[others].mean()
    print(f"sheet k={k}: {rounded:.4f} of the distances round")
    assert rounded > 0.99, rounded


@pytest.mark.parametrize("k", cr.SHEET_KS)
def test_the_held_radius_makes_its_row_core_and_the_next_float_below_does_not(k):
    row, e4, below = cr.held_radius(k)
    R, names, off = cr.sheet(k)
    assert 0.9 < e4 < 1.0 and np.float32(below) == np.nextafter(np.float32(e4), np.float32(0)) and np.float32(e4) == e4
    d = v0_dist2(R[row:row + 1], R, k)[0]
    d[row] = np.inf
    assert (d <= np.float32(e4)).sum() == 4 and (d <= np.float32(below)).sum() == 3 and (d == np.float32(e4)).sum() == 1
    at, under = cr.want_sheet(k, e4, cr.SHEET_MIN_PTS), cr.want_sheet(k, below, cr.SHEET_MIN_PTS)
    assert at["core"][row] and not under["core"][row]
    assert at["deg"][row] == 4 and under["deg"][row] == 3
    # a `<` for the `<=` of the hit rule would answer `below` at E4: a different core mask, in that row at least
    assert not np.array_equal(co.core_mask_words(at["core"]), co.core_mask_words(under["core"]))


@pytest.mark.parametrize("name", list(cr.GRID))
def test_the_grid_shards_have_rows_of_every_kind_and_the_grid_their_tests_take_them_for(name):
    R = cr.rows_of(name)
    r, min_pts = cr.GRID[name]
    n, k = R.shape
    assert n == (cr.CHUNK + 70 if name == "strip" else cr.N) and R.dtype == np.float32 and not R.flags.writeable
    assert np.isfinite(R).all() and cr.rows_of(name) is R
    w = cr.want(name)
    assert cr.want(name) is w and not w["labels"].flags.writeable           # the reference: made once, left unchanged
    s = cr.shares(w)
    gs = cr.grid_shape(R, r)
    print(f"{name}: radius 2^{int(np.log2(r))} min_pts {min_pts}: core {s[0]:.3f} border {s[1]:.3f} noise {s[2]:.3f} of {n} rows, "
          f"{np.unique(w['labels']).size - 1} clusters, largest {cr.largest_cluster(w['labels'])}, degrees {w['deg'].min()} .. "
          f"{w['deg'].max()}, {int(w['deg'].sum())} ordered pairs; grid {gs['g']} cells on {gs['live']} live axes, largest cell "
          f"{gs['max_cell']} rows, the radius spans {gs['rings']} rings")
    assert min(s) >= SHARE[name], s
    assert gs["g"] == CELLS_PER_AXIS[name] and gs["max_cell"] <= 2048
    if name.startswith("uniform_planted"):
        _, names, off = cr.uniform_planted(k)
        assert_planted(w["labels"], w["core"], names, off, min_pts)
    if name == "gradient":
        assert 3 <= gs["rings"] <= 6 and rmax_of(k, n, gs["rings"]) == 6                       # multi-ring under the plain limit
        assert cr.largest_cluster(np.where(w["core"], w["labels"], -1)) >= 10000               # one component of most core rows
    elif name == "column":
        assert 7 <= gs["rings"] <= 15 and rmax_of(k, n, gs["rings"]) == gs["rings"]            # the plan's radius_rings branch
    elif name == "strip":
        assert gs["rings"] > 90 and rmax_of(k, n, gs["rings"]) == 16                           # past the k = 2 budget: gives up
        assert cr.spanning(w["labels"]).size >= 2
        assert pkg.debug_cluster_plan(k=2, n=n, num_cu=256, core_given=1, grid=1)["chunks"] == 2
    elif name == "dead_axis":
        assert gs["live"] == 2 and (R[:, 1] == np.float32(0.375)).all() and gs["widths"][1] == 1.0
    elif name == "offset":
        assert R.min() >= 4096.0 and R.max() <= 4097.0
    else:
        assert gs["rings"] <= 3
    if name == "blobs":
        assert gs["max_cell"] >= 256                                                           # cells of hundreds of rows


def test_the_column_at_min_pts_1_hangs_on_single_links_and_its_other_radii_are_what_the_tests_say():
    """min_pts 1: the components of the radius graph; many rows are joined to their component by ONE link (a bridge of the graph:
    a core row of degree 1), so a walk that stops a ring early splits a component.  And the radii of the shared give-up word's
    test, from the grid alone: 2^-9 spans more rings than the budget allows, so the plain limit 6 stands and a batch gives up."""
    R = cr.column()
    r, _ = cr.GRID["column"]
    w = cr.want("column", r * r, 1)
    assert w["core"].all() and (w["labels"] >= 0).all()
    comps = np.unique(w["labels"]).size
    print(f"column, min_pts 1: {comps} components, largest {cr.largest_cluster(w['labels'])}, {int((w['deg'] == 1).sum())} rows of degree 1")
    assert comps >= 100 and cr.largest_cluster(w["labels"]) >= 200 and (w["deg"] == 1).sum() >= 500
    n, k = R.shape
    assert rmax_of(k, n, cr.grid_shape(R, 2.0 ** -9)["rings"]) == 6 and cr.grid_shape(R, 2.0 ** -9)["rings"] > 15
    wide = cr.want("column", 2.0 ** -18, 60)
    print(f"column at 2^-9, min_pts 60: core {wide['core'].mean():.3f}, degrees {wide['deg'].min()} .. {wide['deg'].max()}")
    assert 0.05 < wide["core"].mean() < 0.95


def test_the_strips_small_radius_is_a_few_rings_and_finds_pairs():
    R = cr.strip()
    small = 2.0 ** -14
    assert cr.grid_shape(R, small)["rings"] <= 16
    w = cr.want("strip", small * small, 2)
    s = cr.shares(w)
    print(f"strip at 2^-14, min_pts 2: core {s[0]:.3f} noise {s[2]:.3f}")
    assert 0.04 <= s[0] <= 0.96
