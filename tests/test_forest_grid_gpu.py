"""knn_index_self_forest_within on the uniform-grid index (KNN_QUERY_COUNT_GRID) on the GPU: the scan kernel at KD 2 and 4
(tests/cluster_rows.uniform_planted) and at KD 1 and 3 (tests/test_within_grid_gpu.rows_and_queries: half the rows uniform, half in
a cluster, at a radius that leaves isolated rows, small components and one large one), a radius that spans ten rings
(cluster_rows.column: a walk ends on the radius clause or on the nearest foreign row, whichever comes first, and most components
hang on single links), and +INF with the flag, where rows
deep inside a component pass the ring limit, the round's exact scan answers and knn_index_last_stats [2] says so.  Bar: sorted
edges and labels equal tests/forest_oracle.py's and the exact way's on the same index; for the infinite radius (n = 20000: no
oracle) the exact way's alone."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import cluster_rows as cr
from tests import forest_oracle as fo
from tests.forest_helper import assert_forest, run_forest
from tests.test_within_grid_gpu import rows_and_queries

pytestmark = pytest.mark.gpu
BASE = 5
INF = float("inf")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


def both_ways(ix, R, cap, gave_up=0, want=None):
    w = want if want is not None else fo.forest(R, R.shape[1], cap)
    labels, table, count, st = run_forest(ix, cap, grid=True)
    print(f"grid: {len(table)} edges, {np.unique(labels).size} components, {count[1]} rounds of {fo.rounds_of(len(R))}, stats {st}")
    assert st == [3, 0, gave_up, 0], st
    assert_forest(labels, table, w)
    exact, etable, _, st = run_forest(ix, cap)
    assert st == [1, 0, 0, 0], st
    np.testing.assert_array_equal(etable, table)
    np.testing.assert_array_equal(exact, labels)
    return labels, table


@pytest.mark.parametrize("k", [2, 4])
def test_the_grid_scan_kernel_at_two_and_four_dimensions(k):
    R, names, off = cr.uniform_planted(k)
    r, _ = cr.PLANTED_SHAPE[k]
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        labels, table = both_ways(ix, R, r * r)
        g = lambda name: names[name] + off
        assert (labels[g("touching")] == g("touching").min()).all()                        # E == max_dist2 links
        near, far = g("apart near"), g("apart far")
        assert (labels[near] == near.min()).all() and (labels[far] == far.min()).all()    # one ulp beyond does not
        # under option path = 1 the flag changes nothing: the exact self-scan answers
        pkg.set_option("path", 1)
        forced, ftable, _, st = run_forest(ix, r * r, grid=True)
        assert st == [1, 0, 0, 0], st
        np.testing.assert_array_equal(ftable, table)
        np.testing.assert_array_equal(forced, labels)
    finally:
        pkg.set_option("path", 0)
        ix.close()


@pytest.mark.parametrize("k, r", [(1, 2.0 ** -13), (3, 2.0 ** -6)])
def test_the_grid_scan_kernel_at_one_and_three_dimensions(k, r):
    R, _ = rows_and_queries(k, 16384 + 7, 8, 6400 + k)            # the smallest shard that gets a grid index, and a few rows
    want = fo.forest(R, k, r * r)
    sizes = np.bincount(want["labels"])                           # on the CPU, before the GPU is touched
    print(f"k={k}: {(sizes == 1).sum()} isolated rows, {((sizes >= 3) & (sizes < 64)).sum()} components of 3 .. 63 rows, "
          f"the largest of {sizes.max()}")
    assert (sizes == 1).sum() >= 32 and ((sizes >= 3) & (sizes < 64)).sum() >= 32 and sizes.max() > 4096
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        both_ways(ix, R, r * r, want=want)
    finally:
        ix.close()


def test_a_radius_of_ten_rings_keeps_every_single_link():
    R = cr.column()
    r, _ = cr.GRID["column"]
    assert cr.grid_shape(R, r)["rings"] >= 2
    ix = pkg.KnnIndex(3, R, base_index=BASE)
    try:
        both_ways(ix, R, r * r)
    finally:
        ix.close()


def test_an_infinite_radius_with_the_flag_ends_on_the_exact_scan():
    n = 20000
    R = np.random.default_rng(6300).random((n, 3), dtype=np.float32)
    ix = pkg.KnnIndex(3, R, base_index=BASE)
    try:
        labels, table, count, st = run_forest(ix, INF, grid=True)
        print(f"+INF on the grid: {len(table)} edges, {count[1]} rounds of {fo.rounds_of(n)}, stats {st}")
        assert st == [3, 0, 1, 0], st
        assert len(table) == n - 1 and (labels == 0).all()
        exact, etable, _, st = run_forest(ix, INF)
        assert st == [1, 0, 0, 0], st
        np.testing.assert_array_equal(etable, table)
        np.testing.assert_array_equal(exact, labels)
    finally:
        ix.close()
