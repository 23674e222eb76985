"""knn_index_self_count_within_routed and knn_index_self_list_within_routed on the uniform-grid index (KNN_QUERY_COUNT_GRID) on the
GPU against tests/each_oracle.py over tests/self_oracle.self_dist2, and against the existing self calls.  Bar: exact counts and
sorted lists, the own row never listed, another copy of it listed at distance 0; knn_index_last_stats tells the way (3 with the
flag) and whether the batch gave up ([2]) and was answered by the gated self-scan."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.each_helper import dev_f32
from tests.self_oracle import self_dist2
from tests.self_routed_helper import (assert_own_row_absent, assert_same_answer, existing_pipeline, plant_duplicates,
                                      routed_pipeline, segment_numbers)

pytestmark = pytest.mark.gpu
BASE = 5
N = 16384 + 7                     # the smallest shard that gets a grid index, and a few rows
FIRST, ROWS = 5003, 70            # a window that starts inside a block of 64 rows: two waves' worth and six rows
INF = float("inf")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


def kind_max(r, kind):
    return float(r[eo.KINDS.index(kind)::len(eo.KINDS)].max())


@pytest.mark.parametrize("k", [3, 1, 2, 4])
def test_scalar_and_per_row_radii_are_exact_on_the_grid_and_never_list_the_own_row(k):
    R = np.random.default_rng(8100 + k).random((N, k), dtype=np.float32)
    src, twin, outside = plant_duplicates(R, FIRST)
    d = self_dist2(R, k, FIRST, ROWS)
    r = eo.radii_of(d)
    cap_list = kind_max(r, "held")
    eo.assert_every_kind_of_count(eo.counts_of(d, r))
    eo.assert_no_shared_radius_passes(d, r, cap_list)
    own = BASE + FIRST + np.arange(ROWS)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for form, rr, cap in (("scalar", None, cap_list), ("each", r, cap_list), ("each under +INF", r, INF)):
            radii = np.full(ROWS, cap, np.float32) if rr is None else rr
            lists = eo.lists_of(d, radii, cap, base=BASE)
            r_d = dev_f32(rr) if rr is not None else None
            got = routed_pipeline(ix, FIRST, ROWS, cap, r_d, grid=True)
            if cap < INF:
                assert all(st[:3] == [3, 0, 0] for st in got[4]), (k, form, got[4])     # a list-sized cap ends every walk
            else:
                assert all(st[0] == 3 for st in got[4]), (k, form, got[4])
                print(f"k={k}: +INF radii on the grid way: last_stats {got[4]}")         # exact, whichever way it ends
            assert_same_answer(got, lists, existing_pipeline(ix, FIRST, ROWS, cap, r_d), msg=f"k={k} {form}")
            assert_own_row_absent(got, own, msg=f"k={k} {form}")
            for j, others in ((src - FIRST, {twin, outside}), (twin - FIRST, {src, outside})):
                numbers, bits = segment_numbers(got, j)
                assert set(numbers[:2]) == {BASE + o for o in others} and (bits[:2] == 0).all(), (k, form, j, numbers[:4])
                if rr is not None:
                    assert numbers.size == 2, (k, form, j)       # a "zero" radius lists the copies alone
        # the cell flag changes nothing here; without a flag, and under option path = 1, the exact self-scan answers
        r_d = dev_f32(r)
        lists = eo.lists_of(d, r, cap_list, base=BASE)
        ref = existing_pipeline(ix, FIRST, ROWS, cap_list, r_d)
        for flags in (dict(cells=True), dict()):
            got = routed_pipeline(ix, FIRST, ROWS, cap_list, r_d, **flags)
            assert all(st == [1, 0, 0, 0] for st in got[4]), (flags, got[4])
            assert_same_answer(got, lists, ref, msg=f"k={k} {flags}")
        pkg.set_option("path", 1)
        got = routed_pipeline(ix, FIRST, ROWS, cap_list, r_d, grid=True)
        assert all(st == [1, 0, 0, 0] for st in got[4]), got[4]
        assert_same_answer(got, lists, ref, msg=f"k={k} path 1")
    finally:
        ix.close()


def test_a_row_in_an_empty_far_region_gives_up_and_the_gated_self_scan_answers():
    """k = 3: one row of the window sits a box width outside the others, so the grid's first axis is half empty.  Its "held" radius
    — its fifth nearest row, at least a box width away — spans about as many rings as an axis has cells (17), past the walk's
    budget of 2^15 cells (15 rings at k = 3): the plan keeps the plain ring limit, the row's walk ends in the empty half, the batch
    gives up ([2] == 1) and the gated self-scan answers every row exactly — once: nothing of the grid's walk is committed.  (At
    k = 1 a row cannot do this on the smallest shard: its axis has 5461 cells, fewer rings than the budget's 16383.)"""
    k = 3
    R = np.random.default_rng(8200).random((N, k), dtype=np.float32)
    far = FIRST + 0
    assert eo.KINDS[0] == "held"
    R[far] = (-1.0, 0.5, 0.5)
    d = self_dist2(R, k, FIRST, ROWS)
    r = eo.radii_of(d)
    cap = float(r[0])
    assert cap >= 1.0 and cap == kind_max(r, "held")
    assert pkg.debug_self_routed_plan(k=k, m=ROWS, n=N, radius_finite=1, flag_grid=1, flag_cells=0, has_grid=1, has_cells=0, centred=0,
                                      rows_u8=0, bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=17)["rmax"] == 6
    lists = eo.lists_of(d, r, cap, base=BASE)
    assert eo.lengths(lists)[0] == 5
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        r_d = dev_f32(r)
        got = routed_pipeline(ix, FIRST, ROWS, cap, r_d, grid=True)
        assert all(st[:3] == [3, 0, 1] for st in got[4]), got[4]
        assert_same_answer(got, lists, existing_pipeline(ix, FIRST, ROWS, cap, r_d), msg="gave up")
        assert_own_row_absent(got, BASE + FIRST + np.arange(ROWS))
        # the next batch on the slot, rows whose bounds end their walks, finds the word cleared
        first2 = FIRST + 1000
        d2 = self_dist2(R, k, first2, ROWS)
        r2 = eo.radii_of(d2)
        cap2 = kind_max(r2, "held")
        got = routed_pipeline(ix, first2, ROWS, cap2, dev_f32(r2), grid=True)
        assert all(st[:3] == [3, 0, 0] for st in got[4]), got[4]
        assert_same_answer(got, eo.lists_of(d2, r2, cap2, base=BASE), None, msg="the next batch")
    finally:
        ix.close()
