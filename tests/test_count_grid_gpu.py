"""knn_index_count_within on the uniform-grid index (KNN_QUERY_COUNT_GRID) on the GPU against tests/count_oracle.py.  Bar: exact
counts at every radius; knn_index_last_stats tells the way (3 with the flag, 1 without) and whether the batch gave up ([2])."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count, dev_counts
from tests.count_oracle import counts_of, radii
from tests.test_within_grid_gpu import rows_and_queries
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_radius_on_the_smallest_shard_that_gets_a_grid(k):
    n, m = 16384, 70
    R, Q = rows_and_queries(k, n, m, 300 + k)
    d = v0_dist2(Q, R, k)
    ix = pkg.KnnIndex(k, R, base_index=5)
    try:
        for name, r2 in radii(d):
            want = counts_of(d, r2)
            got = count(ix, Q, r2, grid=True)
            st = ix.last_stats()
            assert st[0] == 3, (name, st)
            if r2 != float("inf"):
                assert st[:3] == [3, 0, 0], (name, st)      # every finite radius of the list ends every walk
            else:
                print(f"k={k}: +INF on the grid way: last_stats {st}")   # exact, whichever way it ends
            np.testing.assert_array_equal(got, want, err_msg=f"k={k} {name} r2={r2} (grid)")
            got = count(ix, Q, r2)
            assert ix.last_stats()[:3] == [1, 0, 0], (name, ix.last_stats())
            np.testing.assert_array_equal(got, want, err_msg=f"k={k} {name} r2={r2} (no flag)")
        # a fold on the grid way adds, -0 counts as 0, the cell flag changes nothing here, and non-finite queries count nothing
        r2 = radii(d)[0][1]
        want = counts_of(d, r2)
        held = np.arange(m, dtype=np.uint32) * 3
        np.testing.assert_array_equal(count(ix, Q, r2, counts=dev_counts(m, fill=held), init=False, grid=True), held + want)
        np.testing.assert_array_equal(count(ix, Q, -0.0, grid=True), counts_of(d, 0.0))
        np.testing.assert_array_equal(count(ix, Q, r2, cells=True), want)
        assert ix.last_stats()[0] == 1
        Qbad = Q.copy()
        Qbad[7, 0] = np.nan
        Qbad[9, k - 1] = np.inf
        want_bad = want.copy()
        want_bad[[7, 9]] = 0
        np.testing.assert_array_equal(count(ix, Qbad, r2, grid=True), want_bad)
        assert ix.last_stats()[:3] == [3, 0, 0]
        # option path = 1: the flag is accepted and the exact count answers
        pkg.set_option("path", 1)
        np.testing.assert_array_equal(count(ix, Q, r2, grid=True), want)
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_ties_at_the_boundary_on_a_lattice():
    """The lattice of tests/test_within_grid_gpu.py's tie test: the radius exactly a lattice distance — runs of ties at the
    boundary, all inside — and one ulp below it; radius 0 counts the copies of a query that sits on a row."""
    rng = np.random.default_rng(21)
    k, n = 3, 4000
    R = rng.integers(0, 3, (n, k)).astype(np.float32)
    R[rng.choice(n, 100, replace=False)] = R[17]
    Q = np.concatenate([rng.integers(0, 3, (60, k)).astype(np.float32),
                        (rng.integers(0, 6, (70, k)) * 0.5 - 0.25).astype(np.float32),
                        R[17:18]])
    d = v0_dist2(Q, R, k)
    pkg.set_option("path", 3)
    ix = pkg.KnnIndex(k, R)
    try:
        for d2 in (0.1875, 0.6875, 0.0):
            for r2 in (np.float32(d2), np.nextafter(np.float32(d2), np.float32(0))):
                if r2 < 0:
                    continue
                want = counts_of(d, r2)
                got = count(ix, Q, float(r2), grid=True)
                assert ix.last_stats()[0] == 3, ix.last_stats()
                np.testing.assert_array_equal(got, want, err_msg=f"r2={r2}")
        at, below = counts_of(d, 0.1875), counts_of(d, np.nextafter(np.float32(0.1875), np.float32(0)))
        assert (at > 64).any() and (at - below > 64).any()        # the case is what it says: more than 64 ties at the boundary
        assert (counts_of(d, 0.0) == 0).any() and (counts_of(d, 0.0) > 64).any()
    finally:
        ix.close()


def test_a_radius_ends_the_walk_in_an_empty_region_and_a_walk_past_the_cell_budget_gives_up():
    """The k = 1 construction of tests/test_within_grid_gpu.py: a query two box widths out, the near end of the box empty.  A
    radius below that query's nearest distance ends its walk at the first face bound — count 0, no give-up.  A second query 20 box
    widths out with a radius that spans more rings than the 2^15-cell budget: the plan keeps the plain rmax, the query gives up
    ([2] == 1) and the exact count answers the batch — once: the grid's partial counts are not committed."""
    rng = np.random.default_rng(5)
    k, n = 1, 16384
    R = (0.5 + 0.5 * rng.random((n, k))).astype(np.float32)
    R[0] = 0.0
    lo, width = float(R.min()), float(R.max() - R.min())
    Q = (0.6 + 0.3 * rng.random((21, k))).astype(np.float32)
    Q[11] = lo - 2.0 * width
    d = v0_dist2(Q, R, k)
    nearest = float(d[11].min())
    inside = float(np.median(np.sort(d[np.arange(21) != 11], axis=1)[:, 4]))
    ix = pkg.KnnIndex(k, R, base_index=300)
    try:
        assert inside < nearest
        for r2 in (inside, float(np.nextafter(np.float32(nearest), np.float32(0)))):
            for init in (True, False):
                got = count(ix, Q, r2, grid=True, init=init)
                assert ix.last_stats()[:3] == [3, 0, 0], (r2, init, ix.last_stats())
                assert got[11] == 0
                np.testing.assert_array_equal(got, counts_of(d, r2), err_msg=f"r2={r2} init={init}")
        assert (counts_of(d, inside)[np.arange(21) != 11] > 0).all()
        got = count(ix, Q, float("inf"), grid=True)
        print("+INF with a query in an empty region:", ix.last_stats())
        np.testing.assert_array_equal(got, np.full(21, n, np.uint32))
        Q2 = Q.copy()
        Q2[12] = lo - 20.0 * width
        d2 = v0_dist2(Q2, R, k)
        far = float(np.sort(d2[12])[3])
        assert counts_of(d2, far)[12] == 4
        rings = int(np.sqrt(far) / (width / 5000))
        assert rings > 16383
        assert pkg.debug_count_plan(k=k, m=21, n=n, radius_finite=1, flag_grid=1, flag_cells=0, has_grid=1, has_cells=0, centred=0,
                                    rows_u8=0, bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=rings)["rmax"] == \
            pkg.debug_grid_topk_plan(k=k, K=1, m=21, has_grid=1, path=0, flag=1)["rmax"]
        for init in (True, False):
            held = np.full(21, 1000, np.uint32)
            got = count(ix, Q2, far, grid=True, init=init, counts=dev_counts(21, fill=held))
            assert ix.last_stats()[:3] == [3, 0, 1], ix.last_stats()
            np.testing.assert_array_equal(got, counts_of(d2, far) + (0 if init else held), err_msg=f"beyond the budget, init={init}")
        got = count(ix, Q[:11], inside, grid=True)    # the next batch on the slot finds its word cleared
        assert ix.last_stats()[:3] == [3, 0, 0]
        np.testing.assert_array_equal(got, counts_of(d[:11], inside))
    finally:
        ix.close()
