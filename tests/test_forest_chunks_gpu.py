"""knn_index_self_forest_within over two chunks of own rows and more than one slice on the GPU against tests/forest_oracle.py: k = 2,
n = 65536 + 700.  Uniform rows in a square sized so that a row has about 8 rows within the radius 2^-7, and tests/cluster_helper's
planted block — beyond the square along axis 0 — straddling row 65536.  On the exact way and on the grid way with the flag.  Bar:
both equal the oracle (sorted edges and labels) and so each other; knn_index_last_stats [0] = 1 / 3; the labels equal the cluster
call's at min_pts 1."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import forest_oracle as fo
from tests.cluster_helper import planted, run_cluster
from tests.forest_helper import assert_forest, run_forest

pytestmark = pytest.mark.gpu
BASE = 5
CHUNK = 65536
N = CHUNK + 700
RADIUS = 2.0 ** -7
OFF = CHUNK - 120                      # the planted block's 246 rows lie on both sides of row 65536


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


@functools.lru_cache(maxsize=None)
def shard():
    rng = np.random.default_rng(6200)
    P, names, end = planted(2, RADIUS, 4.0, 0.5, rng)
    side = RADIUS * np.sqrt(np.pi * N / 8.0)          # n pi r^2 / side^2 = 8
    U = (rng.random((N - len(P), 2)) * side).astype(np.float32)
    R = np.concatenate([U[:OFF], P, U[OFF:]])
    assert R.shape == (N, 2) and side < 2.0 and end < 8.0 and OFF < CHUNK < OFF + len(P)
    R.setflags(write=False)
    return R, names


@functools.lru_cache(maxsize=None)
def want():
    R, _ = shard()
    a, b, bits = fo.pairs(R, 2, RADIUS * RADIUS)
    print(f"{a.size / N:.2f} rows within the radius of a row")
    assert 6.0 < a.size / N < 10.0
    return fo.forest_of_pairs(N, a, b, bits)


@pytest.mark.parametrize("grid", [False, True])
def test_two_chunks_of_rows_on_the_exact_and_the_grid_way(grid):
    R, names = shard()
    w = want()
    plan = pkg.debug_forest_plan(k=2, n=N, num_cu=256, grid=int(grid))
    assert plan["chunks"] == 2 and plan["slices"] > 1
    ix = pkg.KnnIndex(2, R, base_index=BASE)
    try:
        labels, table, count, st = run_forest(ix, RADIUS * RADIUS, grid=grid)
        print(f"grid={grid}: {len(table)} edges, {np.unique(labels).size} components, {count[1]} rounds of {fo.rounds_of(N)}, stats {st}")
        assert st == ([3, 0, 0, 0] if grid else [1, 0, 0, 0]), st
        assert_forest(labels, table, w)
        for chain in ("chain down", "chain mixed"):
            rows = names[chain] + OFF
            assert (labels[rows] == rows.min()).all(), chain
        straddle = names["chain mixed"] + OFF
        assert straddle.min() < CHUNK <= straddle.max()                  # one component with rows in both chunks
        comp, _, _ = run_cluster(ix, RADIUS * RADIUS, 1, grid=grid)
        np.testing.assert_array_equal(labels, comp)
    finally:
        ix.close()
