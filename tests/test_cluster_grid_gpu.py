"""knn_index_self_cluster_within on the uniform-grid index (KNN_QUERY_COUNT_GRID) on the GPU against tests/cluster_oracle.py and
against the exact way: N = 16384 + 7, the smallest shard with a grid index, k = 3 and k = 1.  Bar: labels and core mask equal the
oracle's AND the exact way's bit for bit; knn_index_last_stats tells the way (3 with the flag) and whether a batch gave up ([2]),
after which the gated exact sweeps answer — over whatever the grid walk had united already."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co
from tests.cluster_helper import assert_planted, planted, run_cluster

pytestmark = pytest.mark.gpu
BASE = 5
N = 16384 + 7
# the radius (a power of two: the planted structures' unit) and min_pts per k: about two rows within the radius of a uniform row,
# so that core, border and noise rows are all common — the test asserts the shares by the oracle
SHAPE = {3: (2.0 ** -5, 4), 1: (2.0 ** -14, 4)}


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


@functools.lru_cache(maxsize=None)
def shard(k):
    """Uniform rows in the unit cube and, a quarter beyond it along axis 0, the planted block (no row with a non-finite coordinate:
    such a shard gets no grid index), in the middle of the row order."""
    r, _ = SHAPE[k]
    rng = np.random.default_rng(4400 + k)
    P, names, end = planted(k, r, 1.25, 0.5, rng)
    U = rng.random((N - len(P), k), dtype=np.float32)
    off = 9000
    R = np.concatenate([U[:off], P, U[off:]])
    assert R.shape == (N, k) and end < 8.0
    return R, names, off


@functools.lru_cache(maxsize=None)
def want(k):
    r, min_pts = SHAPE[k]
    return co.cluster(shard(k)[0], k, r * r, min_pts)


@pytest.mark.parametrize("k", [3, 1])
def test_the_grid_way_gives_the_oracles_and_the_exact_ways_labels_bit_for_bit(k):
    R, names, off = shard(k)
    r, min_pts = SHAPE[k]
    w = want(k)
    core, border, lab = w["core"], w["border"], w["labels"]
    shares = (core.mean(), border.mean(), (lab < 0).mean())
    print(f"k={k}: core {shares[0]:.3f} border {shares[1]:.3f} noise {shares[2]:.3f} of {N} rows, {np.unique(lab).size - 1} clusters")
    assert min(shares) >= 0.05, shares                                     # a condition on the inputs, by the oracle
    assert_planted(lab, core, names, off, min_pts)
    words = co.core_mask_words(core)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        got, gw, st = run_cluster(ix, r * r, min_pts, grid=True)
        assert st[:3] == [3, 0, 0], st
        np.testing.assert_array_equal(got, lab)
        np.testing.assert_array_equal(gw, words)
        assert_planted(got, core, names, off, min_pts)
        again, aw, st = run_cluster(ix, r * r, min_pts, grid=True, want_core=False, slot=2)
        assert st[:3] == [3, 0, 0] and aw is None
        np.testing.assert_array_equal(again, got)
        # without the flag, and under option path = 1, the exact self-scan answers: the same labels
        exact, ew, st = run_cluster(ix, r * r, min_pts)
        assert st == [1, 0, 0, 0], st
        np.testing.assert_array_equal(exact, got)
        np.testing.assert_array_equal(ew, gw)
        pkg.set_option("path", 1)
        forced, fw, st = run_cluster(ix, r * r, min_pts, grid=True)
        assert st == [1, 0, 0, 0], st
        np.testing.assert_array_equal(forced, got)
        np.testing.assert_array_equal(fw, gw)
        pkg.set_option("path", 0)
        # min_pts = 1 on the grid: the components of the radius graph
        comp, cw, st = run_cluster(ix, r * r, 1, grid=True)
        assert st[:3] == [3, 0, 0], st
        np.testing.assert_array_equal(comp, co.cluster(R, k, r * r, 1)["labels"])
        assert (cw == co.core_mask_words(np.ones(N, dtype=bool))).all()
    finally:
        ix.close()


def test_a_radius_that_outruns_the_ring_budget_gives_up_and_the_gated_sweeps_answer():
    """k = 3.  A batch gives up when some row's walk reaches the ring limit before its face bound passes the radius.  On a cubic
    cloud of this size a scalar radius of that many rings holds the whole shard (every pair a hit: one cluster, and an oracle of
    2.7e8 pairs), so the cloud here is a thin column: axis 0 spans [0, 1], axes 1 and 2 span 2^-10.  The cells are as thin, the
    radius 2^-9 spans about 35 rings of them — past the budget of 2^15 cells (15 rings at k = 3), so the plan keeps the plain ring
    limit 6 — while a row has only some 60 rows within it.  One row sits a box width away along axis 0, as in
    tests/test_self_routed_grid_gpu.py.  Both batches give up ([2] == 1); the degrees come from the gated self count, the links
    from the gated exact sweep over what the grid walk had united; the labels are the oracle's.  The next call on the slot, at a
    radius of a few rings, finds the word cleared."""
    k = 3
    rng = np.random.default_rng(4500)
    R = rng.random((N, k), dtype=np.float32)
    R[:, 1:] *= np.float32(2.0 ** -10)
    far = 5003
    R[far] = (-1.0, 2.0 ** -11, 2.0 ** -11)
    rad, min_pts = 2.0 ** -9, 60
    assert pkg.debug_self_routed_plan(k=k, m=N, n=N, radius_finite=1, flag_grid=1, flag_cells=0, has_grid=1, has_cells=0, centred=0,
                                      rows_u8=0, bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=35)["rmax"] == 6
    w = co.cluster(R, k, rad * rad, min_pts)
    print(f"give-up: degrees {w['deg'].min()} .. {w['deg'].max()}, core {w['core'].mean():.3f} border {w['border'].mean():.3f}, "
          f"{np.unique(w['labels']).size - 1} clusters")
    assert w["deg"][far] == 0 and w["labels"][far] == -1 and 0.05 < w["core"].mean() < 0.95
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        got, gw, st = run_cluster(ix, rad * rad, min_pts, grid=True)
        assert st[:3] == [3, 0, 1], st
        np.testing.assert_array_equal(got, w["labels"])
        np.testing.assert_array_equal(gw, co.core_mask_words(w["core"]))
        small = 2.0 ** -13
        w2 = co.cluster(R, k, small * small, 2)
        got, gw, st = run_cluster(ix, small * small, 2, grid=True)
        assert st[:3] == [3, 0, 0], st
        np.testing.assert_array_equal(got, w2["labels"])
        np.testing.assert_array_equal(gw, co.core_mask_words(w2["core"]))
    finally:
        ix.close()
