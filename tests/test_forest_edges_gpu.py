"""knn_index_self_forest_within on the GPU, the small print: one row, two duplicates, radius 0, rows with non-finite coordinates,
an empty radius graph, the same call twice and two calls on two slots and streams at once, and the host form (sorted edges, the
optional NULL outputs, info).  tests/forest_helper.Outputs.read holds EVERY call to: at most n - 1 edges, count[1] <= ROUNDS(n),
poisoned outputs beyond count[0] keep their poison.  (E == max_dist2 links and one ulp beyond does not: the planted "touching" /
"apart" of tests/test_forest_forms_gpu.py and tests/test_forest_grid_gpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

import multicore_hw2_amd as pkg
from tests import forest_oracle as fo
from tests.forest_helper import Outputs, assert_forest, run_forest, walks

pytestmark = pytest.mark.gpu
BASE = 5
INF = float("inf")


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


def test_one_row_and_two_duplicates():
    ix = pkg.KnnIndex(3, np.array([[1.0, 2.0, 3.0]], dtype=np.float32), base_index=BASE)
    try:
        for cap in (0.0, 1.0, INF):
            labels, table, count, st = run_forest(ix, cap)
            assert labels.tolist() == [0] and len(table) == 0 and count == [0, 0] and st == [1, 0, 0, 0]
        lab, lo, hi, d2, info = ix.self_forest_within_host(INF)
        assert lab.tolist() == [0] and lo.size == hi.size == d2.size == 0
        assert info == dict(edges=0, components=1, rounds=1, gave_up=0)
    finally:
        ix.close()
    ix = pkg.KnnIndex(3, np.array([[1.0, 2.0, 3.0]] * 2, dtype=np.float32), base_index=BASE)
    try:
        for cap in (0.0, -0.0, INF):
            labels, table, count, _ = run_forest(ix, cap)
            assert labels.tolist() == [0, 0] and table.tolist() == [[0, 0, 1]] and count == [1, 1]
    finally:
        ix.close()


def test_radius_zero_joins_the_duplicates_alone_and_non_finite_rows_are_isolated():
    k, n = 5, 333
    rng = np.random.default_rng(6400)
    R = walks(n, k, rng)
    R[100], R[200], R[201] = R[3], R[3], R[17]                  # duplicates, for certain
    R[50, 2], R[51, 0], R[52, 4] = np.nan, np.inf, -np.inf
    bad = [50, 51, 52]
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for cap in (0.0, 1.0, 2.0, INF):
            w = fo.forest(R, k, cap)
            labels, table, count, st = run_forest(ix, cap)
            assert st == [1, 0, 0, 0]
            assert_forest(labels, table, w)
            assert (labels[bad] == bad).all() and not np.isin(table[:, 1:], bad).any()
            if cap == 0.0:
                assert (table[:, 0] == 0).all() and len(table) >= 3 and labels[100] == labels[200] == labels[3] and labels[201] == labels[17]
            if cap == INF:
                assert len(table) == n - 1 - len(bad) and count[1] <= fo.rounds_of(n)
    finally:
        ix.close()


def test_a_radius_below_every_distance_gives_no_edge():
    R = np.random.default_rng(6500).random((1000, 2), dtype=np.float32)
    ix = pkg.KnnIndex(2, R, base_index=BASE)
    try:
        labels, table, count, _ = run_forest(ix, 1e-12)
        assert (labels == np.arange(1000)).all() and len(table) == 0 and count == [0, 0]
    finally:
        ix.close()


def test_the_same_call_twice_and_two_calls_on_two_slots_and_streams_at_once():
    k, n = 3, 5000
    rng = np.random.default_rng(6600)
    R = np.round(rng.random((n, k)) * 24.0).astype(np.float32)   # a lattice: ties everywhere
    cap = 2.0
    w = fo.forest(R, k, cap)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        labels, table, count, _ = run_forest(ix, cap)
        assert_forest(labels, table, w)
        again, atable, acount, _ = run_forest(ix, cap)
        np.testing.assert_array_equal(atable, table)
        np.testing.assert_array_equal(again, labels)
        assert acount == count
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1, o2 = Outputs(n), Outputs(n)
        torch.cuda.synchronize()
        o1.call(ix, cap, slot=1, stream=s1.cuda_stream)
        o2.call(ix, INF, slot=2, stream=s2.cuda_stream)
        torch.cuda.synchronize()
        l1, t1, c1 = o1.read()
        l2, t2, c2 = o2.read()
        np.testing.assert_array_equal(t1, table)
        np.testing.assert_array_equal(l1, labels)
        assert c1 == count
        alone, ttable, tcount, _ = run_forest(ix, INF)
        np.testing.assert_array_equal(t2, ttable)
        np.testing.assert_array_equal(l2, alone)
        assert c2 == tcount and len(t2) == n - 1
    finally:
        ix.close()


def test_the_host_form_sorts_the_edges_and_tallies():
    k, n = 2, 700
    R = walks(n, k, np.random.default_rng(6700))
    R[600] = (500.0, 500.0)
    cap = 1.0
    w = fo.forest(R, k, cap)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        lab, lo, hi, d2, info = ix.self_forest_within_host(cap)
        np.testing.assert_array_equal(lab, w["labels"])
        np.testing.assert_array_equal(lo, w["lo"])                    # in the oracle's ORDER: ascending (E, i, j)
        np.testing.assert_array_equal(hi, w["hi"])
        np.testing.assert_array_equal(d2.view(np.uint32), w["bits"])
        assert info["edges"] == len(w["lo"]) and info["components"] == np.unique(w["labels"]).size == n - info["edges"]
        assert 1 <= info["rounds"] <= fo.rounds_of(n) and info["gave_up"] == 0
        none, lo2, hi2, nod2, info2 = ix.self_forest_within_host(cap, want_labels=False, want_dist2=False)
        assert none is None and nod2 is None and info2 == info
        np.testing.assert_array_equal(lo2, lo)
        np.testing.assert_array_equal(hi2, hi)
        # info may be NULL too
        lo3, hi3 = np.empty(n, np.int32), np.empty(n, np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert pkg.self_forest_within_host_c()(ix._h, cap, 0, None, vp(lo3), vp(hi3), None, None) == 0
        np.testing.assert_array_equal(lo3[:info["edges"]], lo)
        _, lo4, hi4, d4, info4 = ix.self_forest_within_host(INF)
        w4 = fo.forest(R, k, INF)
        np.testing.assert_array_equal(np.stack([lo4, hi4]), np.stack([w4["lo"], w4["hi"]]))
        np.testing.assert_array_equal(d4.view(np.uint32), w4["bits"])
        assert info4["edges"] == n - 1 and info4["components"] == 1
    finally:
        ix.close()
