"""knn_index_self_forest_within on the GPU when ALL ROUNDS(n) queued rounds add an edge: rows paired at every level
(tests/forest_oracle.paired — every round joins each component to its sibling alone, so the components halve exactly), in shuffled
row order, at +INF.  No later round flattens the labels behind the last hook, which re-parents a root alone: the call's last
flatten must.  Bar: count_dev[1] == ROUNDS(n), sorted edges and labels equal tests/forest_oracle.py's (n = 4, 8, 64, 1024); at
n = 2^14 (a grid index; no oracle at that size) labels all 0 and n - 1 edges on the exact way, and the grid way's equal to them."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import forest_oracle as fo
from tests.forest_helper import assert_forest, run_forest

pytestmark = pytest.mark.gpu
BASE = 5
INF = float("inf")


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


@pytest.mark.parametrize("levels,k,factor", [(2, 1, 4), (3, 1, 4), (6, 1, 4), (3, 2, 3), (6, 2, 3), (10, 2, 3)])
def test_every_queued_round_adds_an_edge_and_the_labels_are_still_the_answer(levels, k, factor):
    n = 1 << levels
    R = fo.paired(levels, k, factor, np.random.default_rng(6800 + levels))
    w = fo.forest(R, k, INF)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        labels, table, count, st = run_forest(ix, INF)
        assert st == [1, 0, 0, 0], st
        assert count == [n - 1, fo.rounds_of(n)] and fo.rounds_of(n) == levels, count
        assert_forest(labels, table, w)
        assert (labels == 0).all()
        lab, lo, hi, _, info = ix.self_forest_within_host(INF)
        np.testing.assert_array_equal(lab, w["labels"])
        assert info == dict(edges=n - 1, components=1, rounds=levels, gave_up=0)
        # a radius that cuts the top level: two components, one round fewer, the labels their smallest rows
        cap = float(factor) ** (levels - 1) * 0.5
        w2 = fo.forest(R, k, cap * cap)
        labels, table, count, _ = run_forest(ix, cap * cap)
        assert count == [n - 2, levels - 1], count
        assert_forest(labels, table, w2)
    finally:
        ix.close()


def test_fourteen_rounds_on_a_grid_index_on_both_ways():
    levels, k = 14, 2
    n = 1 << levels
    R = fo.paired(levels, k, 3, np.random.default_rng(6900))
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        labels, table, count, st = run_forest(ix, INF)
        assert st == [1, 0, 0, 0], st
        assert count == [n - 1, levels] and (labels == 0).all(), count
        glabels, gtable, gcount, st = run_forest(ix, INF, grid=True)
        assert st[0] == 3 and st[1] == 0 and st[3] == 0, st
        assert gcount == count
        np.testing.assert_array_equal(gtable, table)
        np.testing.assert_array_equal(glabels, labels)
    finally:
        ix.close()
