"""knn_index_self_cluster_within on the uniform-grid index (KNN_QUERY_COUNT_GRID) on the GPU against tests/cluster_oracle.py and
against the exact way, on the shards of tests/cluster_rows.py: the grid link kernel at KD 2 and KD 4, walks of several rings that
no exact sweep repeats — under the plain ring limit (gradient) and under the plan's radius_rings limit (column) —, dense cells, a
box far from the origin, a dead axis, a give-up whose gated exact sweeps run in two chunks (strip), and the slot's give-up word
shared with a routed self count.  Bar: labels and core mask equal the oracle's AND the exact way's, element for element;
knn_index_last_stats tells the way and whether a batch gave up.  tests/test_cluster_rows_logic.py proves what each shard is."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co
from tests import cluster_rows as cr
from tests.cluster_helper import assert_planted, run_cluster
from tests.count_helper import dev

pytestmark = pytest.mark.gpu
BASE = 5


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


def assert_equals(got, words, w):
    np.testing.assert_array_equal(got, w["labels"])
    np.testing.assert_array_equal(words, co.core_mask_words(w["core"]))


def both_ways(ix, name, w, max_dist2=None, min_pts=None, gave_up=0):
    """One call on the grid and one without the flag: both the oracle's answer w.  Returns the grid way's labels and words."""
    r, mp = cr.GRID[name]
    cap, mp = (r * r if max_dist2 is None else max_dist2), (mp if min_pts is None else min_pts)
    got, gw, st = run_cluster(ix, cap, mp, grid=True)
    assert st[:3] == [3, 0, gave_up], st
    assert_equals(got, gw, w)
    exact, ew, st = run_cluster(ix, cap, mp)
    assert st == [1, 0, 0, 0], st
    np.testing.assert_array_equal(exact, got)
    np.testing.assert_array_equal(ew, gw)
    core = np.where(w["core"], got, -1)
    print(f"{name} (min_pts {mp}): largest cluster on the GPU {cr.largest_cluster(got)} rows, of core rows alone {cr.largest_cluster(core)}")
    return got, gw


@pytest.mark.parametrize("k", [2, 4])
def test_the_grid_link_kernel_at_two_and_four_dimensions(k):
    name = "uniform_planted%d" % k
    R, names, off = cr.uniform_planted(k)
    r, min_pts = cr.GRID[name]
    w = cr.want(name)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        got, _ = both_ways(ix, name, w)
        assert_planted(got, w["core"], names, off, min_pts)
        hl, hc, info = ix.self_cluster_within_host(r * r, min_pts, grid=True)
        assert ix.last_stats()[:3] == [3, 0, 0]
        np.testing.assert_array_equal(hl, co.renumber(w["labels"]))
        np.testing.assert_array_equal(hc, w["core"])
        assert info == dict(clusters=np.unique(w["labels"]).size - 1, core=int(w["core"].sum()), border=int(w["border"].sum()),
                            noise=int((w["labels"] < 0).sum()))
    finally:
        ix.close()


def test_walks_of_four_rings_under_the_plain_limit_and_thousands_of_waves_on_one_root():
    """gradient(): every walk goes to ring 3 or 4 and ends on the stop clause, no exact sweep behind it; 10.2 k core rows are ONE
    component (a cluster of 13.6 k rows with its border), so every wave of the dense end hooks into the same set, 64 lanes at a time for the same row.  Three calls: the
    forest's shape depends on the timing, the labels must not."""
    w = cr.want("gradient")
    ix = pkg.KnnIndex(3, cr.gradient(), base_index=BASE)
    try:
        got, gw = both_ways(ix, "gradient", w)
        for _ in range(2):
            again, aw, st = run_cluster(ix, cr.GRID["gradient"][0] ** 2, cr.GRID["gradient"][1], grid=True)
            assert st[:3] == [3, 0, 0], st
            np.testing.assert_array_equal(again, got)
            np.testing.assert_array_equal(aw, gw)
    finally:
        ix.close()


@pytest.mark.parametrize("min_pts", [8, 1])
def test_walks_past_ring_six_without_a_give_up_keep_every_single_link(min_pts):
    """column(): the radius spans 10 rings, the plan's limit is that count (its radius_rings branch), nothing gives up and nothing
    is swept again.  Most components hang on single links: one link dropped by an early stop splits a component."""
    r, _ = cr.GRID["column"]
    w = cr.want("column", r * r, min_pts)
    ix = pkg.KnnIndex(3, cr.column(), base_index=BASE)
    try:
        got, gw = both_ways(ix, "column", w, min_pts=min_pts)
        if min_pts == 1:
            assert (gw == co.core_mask_words(np.ones(cr.N, dtype=bool))).all() and (got >= 0).all()
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["blobs", "offset", "dead_axis"])
def test_dense_cells_a_box_far_from_the_origin_and_a_dead_axis(name):
    R = cr.rows_of(name)
    ix = pkg.KnnIndex(R.shape[1], R, base_index=BASE)
    try:
        both_ways(ix, name, cr.want(name))
    finally:
        ix.close()


def test_a_give_up_in_two_chunks_of_rows_and_the_word_cleared_for_the_next_call():
    """strip(): 149 rings, past the k = 2 budget, so the plain limit 16 stands and the batch gives up; the gated self count and the
    gated exact link sweep answer, each in two chunks of rows (n = 65536 + 70), over what the grid walk had united; clusters lie
    across row 65536.  The next call on the slot, at a radius of a few rings, finds the word cleared."""
    R = cr.strip()
    n = R.shape[0]
    w = cr.want("strip")
    assert pkg.debug_cluster_plan(k=2, n=n, num_cu=256, core_given=1, grid=1)["chunks"] == 2
    assert cr.spanning(w["labels"]).size >= 2
    ix = pkg.KnnIndex(2, R, base_index=BASE)
    try:
        both_ways(ix, "strip", w, gave_up=1)
        small = 2.0 ** -14
        both_ways(ix, "strip", cr.want("strip", small * small, 2), max_dist2=small * small, min_pts=2)
    finally:
        ix.close()


def test_the_give_up_word_of_a_slot_is_shared_with_the_routed_self_count_in_either_order():
    """column()'s index, slot 0.  A cluster call that gives up (radius 2^-9: 35 rings, limit 6), then a routed self count on the
    grid at 2^-22 (10 rings: the plan's limit) — it must not see the cluster call's word; then a count that gives up (2^-18), then a
    cluster call at 2^-11 that does not."""
    R = cr.column()
    n = cr.N
    r, min_pts = cr.GRID["column"]
    wide = 2.0 ** -9
    w_wide, w = cr.want("column", wide * wide, 60), cr.want("column")
    ix = pkg.KnnIndex(3, R, base_index=BASE)
    try:
        got, gw, st = run_cluster(ix, wide * wide, 60, grid=True)
        assert st[:3] == [3, 0, 1], st
        assert_equals(got, gw, w_wide)
        counts = torch.full((n,), 12345, dtype=torch.int32, device=dev())
        torch.cuda.synchronize()
        ix.self_count_within_routed(0, n, counts.data_ptr(), cap=r * r, grid=True, init=True)
        torch.cuda.synchronize()
        st = ix.last_stats()
        assert st[0] == 3 and st[2] == 0, st
        np.testing.assert_array_equal(counts.cpu().numpy(), w["deg"])
        # the other order
        counts.fill_(12345)
        torch.cuda.synchronize()
        ix.self_count_within_routed(0, n, counts.data_ptr(), cap=wide * wide, grid=True, init=True)
        torch.cuda.synchronize()
        st = ix.last_stats()
        assert st[0] == 3 and st[2] == 1, st
        np.testing.assert_array_equal(counts.cpu().numpy(), w_wide["deg"])
        got, gw, st = run_cluster(ix, r * r, min_pts, grid=True)
        assert st[:3] == [3, 0, 0], st
        assert_equals(got, gw, w)
    finally:
        ix.close()
