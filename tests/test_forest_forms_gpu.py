"""knn_index_self_forest_within on the exact self-scan in EVERY compiled form of knn_forest_scan_kernel<KC> on the GPU against
tests/forest_oracle.py: k = 7 (KC 1, a partial chunk), 17 (2), 48 (3), 49 (4), 80 (5), 81 (6), 112 (7), 113 (8, a partial last
chunk) and 129 (KC 0, the generic loop).  The rows: lattice walks (tests/forest_helper.walks: every squared distance a small
integer, so nearly every pick is a tie that the edge order alone decides) around tests/cluster_helper.planted at unit radius, n =
596 (n % 64 = 20: the last wave's done bits are one word), base_index != 0.  At max_dist2 = 1 and at +INF.  Bar: the sorted edges
and the labels equal the oracle's exactly; at the finite radius the labels equal the cluster call's at min_pts 1 on the same index."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import forest_oracle as fo
from tests.cluster_helper import planted, run_cluster
from tests.forest_helper import assert_forest, run_forest, walks

pytestmark = pytest.mark.gpu
BASE = 5
N, OFF = 596, 200
KS = (7, 17, 48, 49, 80, 81, 112, 113, 129)
INF = float("inf")


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


@functools.lru_cache(maxsize=None)
def rows(k):
    rng = np.random.default_rng(6100 + k)
    P, names, _ = planted(k, 1.0, 512.0, 0.0, rng)          # clear of the walks, which stay within a few dozen units of the origin
    W = walks(N - len(P), k, rng)
    R = np.concatenate([W[:OFF], P, W[OFF:]])
    assert R.shape == (N, k)
    R.setflags(write=False)
    return R, names


@functools.lru_cache(maxsize=None)
def want(k, cap):
    return fo.forest(rows(k)[0], k, cap)


@pytest.mark.parametrize("k", KS)
def test_every_scan_kernel_form_gives_the_oracles_forest(k):
    R, names = rows(k)
    g = lambda name: names[name] + OFF
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for cap in (1.0, INF):
            w = want(k, cap)
            labels, table, count, st = run_forest(ix, cap)
            print(f"k={k} (KC {(k + 15) // 16 if k <= 128 else 0}) cap {cap}: {len(table)} edges, {np.unique(labels).size} components, "
                  f"{count[1]} rounds of {fo.rounds_of(N)}")
            assert st == [1, 0, 0, 0], st
            assert_forest(labels, table, w)
            assert count[0] == len(table)
        # the finite radius again: the planted structures, and the cluster call's components on the same index
        labels, table, _, _ = run_forest(ix, 1.0)
        for chain in ("chain down", "chain mixed"):
            assert (labels[g(chain)] == g(chain).min()).all(), chain
        assert (labels[g("touching")] == g("touching").min()).all()                        # E == max_dist2 links
        near, far = g("apart near"), g("apart far")
        assert (labels[near] == near.min()).all() and (labels[far] == far.min()).all()    # one ulp beyond does not
        comp, _, _ = run_cluster(ix, 1.0, 1)
        np.testing.assert_array_equal(labels, comp)
    finally:
        ix.close()
