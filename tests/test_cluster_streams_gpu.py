"""knn_index_self_cluster_within calls that OVERLAP on the GPU: three streams, three slots, three (radius, min_pts) pairs on one
index, queued back to back and synchronised once — on the grid way (tests/cluster_rows.uniform_planted(2)) and on the exact way
(sheet(49)) — and two grid calls on two streams of which one gives up (column(): a give-up radius on a square cloud holds the
whole shard, an oracle of 2.7e8 pairs).  Every other cluster call of the suite is on the null stream, which serialises them.
Bar: every answer equals its oracle's exactly; a slot's give-up word is its own.  No graphs, three streams at the most."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co
from tests import cluster_rows as cr
from tests.count_helper import dev

pytestmark = pytest.mark.gpu
BASE = 5
SLOTS = (0, 3, 5)


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


def overlapped(ix, calls, grid):
    """calls: (max_dist2, min_pts, slot) each on a stream of its own, queued back to back, ONE synchronisation.  Returns
    [(labels, core words)] and knn_index_last_stats, which describes the call queued last."""
    n = ix.n
    streams = [torch.cuda.Stream() for _ in calls]
    outs = [(torch.full((n,), -7, dtype=torch.int32, device=dev()), torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev()))
            for _ in calls]
    torch.cuda.synchronize()                                               # the poison is in place before any stream starts
    for (cap, min_pts, slot), s, (labels, core) in zip(calls, streams, outs):
        ix.self_cluster_within(cap, min_pts, labels.data_ptr(), core_dev=core.data_ptr(), stream=s.cuda_stream, slot=slot, grid=grid)
    torch.cuda.synchronize()
    st = ix.last_stats()
    return [(labels.cpu().numpy(), core.cpu().numpy().view(np.uint32)) for labels, core in outs], st


def assert_equals(got, w):
    np.testing.assert_array_equal(got[0], w["labels"])
    np.testing.assert_array_equal(got[1], co.core_mask_words(w["core"]))


def test_three_grid_calls_on_three_streams_and_slots_each_give_their_own_oracles_answer():
    R, _, _ = cr.uniform_planted(2)
    r = cr.GRID["uniform_planted2"][0]
    shapes = [(r * r, 4), (r * r, 5), (r * r / 4, 2)]
    wants = [cr.want("uniform_planted2", cap, mp) for cap, mp in shapes]
    assert len({w["labels"].tobytes() for w in wants}) == 3               # three different answers
    ix = pkg.KnnIndex(2, R, base_index=BASE)
    try:
        got, st = overlapped(ix, [(cap, mp, slot) for (cap, mp), slot in zip(shapes, SLOTS)], grid=True)
        assert st[:3] == [3, 0, 0], st
        for g, w in zip(got, wants):
            assert_equals(g, w)
    finally:
        ix.close()


def test_three_exact_calls_on_three_streams_and_slots_each_give_their_own_oracles_answer():
    k = 49
    R, _, _ = cr.sheet(k)
    shapes = [(1.0, 5), (1.0, 4), (0.75, 3)]
    wants = [cr.want_sheet(k, cap, mp) for cap, mp in shapes]
    assert len({w["labels"].tobytes() for w in wants}) == 3
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        got, st = overlapped(ix, [(cap, mp, slot) for (cap, mp), slot in zip(shapes, SLOTS)], grid=False)
        assert st == [1, 0, 0, 0], st
        for g, w in zip(got, wants):
            assert_equals(g, w)
    finally:
        ix.close()


def test_a_call_that_gives_up_and_one_that_does_not_overlap_and_each_slot_keeps_its_own_word():
    """knn_index_last_stats describes the call queued last, so the pair runs in both orders: the word it reads is that call's
    slot's, whatever the other slot's walk raised meanwhile."""
    r, min_pts = cr.GRID["column"]
    wide = 2.0 ** -9
    w, w_wide = cr.want("column"), cr.want("column", wide * wide, 60)
    fine, gives_up = (r * r, min_pts), (wide * wide, 60)
    ix = pkg.KnnIndex(3, cr.column(), base_index=BASE)
    try:
        got, st = overlapped(ix, [gives_up + (3,), fine + (5,)], grid=True)
        assert st[:3] == [3, 0, 0], st
        assert_equals(got[0], w_wide)
        assert_equals(got[1], w)
        got, st = overlapped(ix, [fine + (5,), gives_up + (3,)], grid=True)
        assert st[:3] == [3, 0, 1], st
        assert_equals(got[0], w)
        assert_equals(got[1], w_wide)
    finally:
        ix.close()
