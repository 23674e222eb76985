"""knn_index_count_within_each and knn_index_list_within_each on the cell-pruned scan (KNN_QUERY_COUNT_CELLS) on the GPU against
tests/each_oracle.py.  Bar: exact counts and sorted lists at every kind of radius; "pruned" means knn_index_last_stats()[0] == 4,
[2] != 0 a pass that fell back and was answered by the exact scan."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.count_helper import dev_counts
from tests.each_helper import assert_segments, count_each, dev_f32, pipeline
from tests.test_within_cells_gpu import BINS, FP16, MATRIX, N17, OPTIONS, spread_queries
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
BASE = 11
INF = float("inf")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


def kind_max(r, kind):
    return float(r[eo.KINDS.index(kind)::len(eo.KINDS)].max())


@pytest.mark.parametrize("name,k,opts", MATRIX, ids=[c[0] for c in MATRIX])
def test_every_kind_of_radius_is_exact_and_a_list_sized_cap_stays_pruned(name, k, opts):
    rng = np.random.default_rng(N17 + 7 * k)
    m = 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    r = eo.radii_of(d)
    eo.assert_every_kind_of_count(eo.counts_of(d, r))
    eo.assert_no_shared_radius_passes(d, r)
    cap_list, cap_many = kind_max(r, "held"), kind_max(r, "many")    # the largest list-sized radius; the largest of the batch's finite ones
    eo.assert_no_shared_radius_passes(d, r, cap_list)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for cap in (cap_list, cap_many):
            lists = eo.lists_of(d, r, cap, base=BASE)
            counts, off, fill, keys, stats = pipeline([ix], dev_f32(Q), dev_f32(r), m, cap=cap, cells=True)
            assert all(st[0] == 4 for st in stats), (name, cap, stats)
            if cap == cap_list:
                assert all(st[2] == 0 for st in stats), (name, stats)
            else:
                print(f"{name}: cap at the largest > 64-hit radius: last_stats {stats}")   # pruned or not: not gated
            np.testing.assert_array_equal(counts, eo.lengths(lists), err_msg=f"{name} cap={cap}")
            np.testing.assert_array_equal(fill, counts)
            assert_segments(off, keys, lists, msg=f"{name} cap={cap}")
        eo.assert_every_kind_of_count(eo.counts_of(d, r, cap_many))
        # cap = +INF: nothing to prune with — the exact scan; so without the flag, and for m < 5
        want = eo.counts_of(d, r)
        np.testing.assert_array_equal(count_each(ix, Q, r, cells=True), want)
        assert ix.last_stats()[0] == 1
        want = eo.counts_of(d, r, cap_list)
        np.testing.assert_array_equal(count_each(ix, Q, r, cap=cap_list), want)
        assert ix.last_stats()[0] == 1
        np.testing.assert_array_equal(count_each(ix, Q[:4], r[:4], cap=cap_list, cells=True), want[:4])
        assert ix.last_stats()[0] == 1
        # a fold on the pruned way adds
        held = np.arange(m, dtype=np.uint32) * 5
        np.testing.assert_array_equal(count_each(ix, Q, r, cap=cap_list, counts=dev_counts(m, fill=held), init=False, cells=True),
                                      held + want)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0
    finally:
        ix.close()


def test_two_passes_advance_the_radii():
    """m = 1024 + 96: the first pass's queries are 16 copies of 64, so the oracle is evaluated for those 64 and for the second
    pass; the second pass's kinds start elsewhere in the cycle."""
    rng = np.random.default_rng(49)
    k, m1, m2 = 8, 1024, 96
    R = rng.random((N17, k), dtype=np.float32)
    Qa = spread_queries(rng, 64 + m2, k)
    Q1, Q2 = Qa[:64], Qa[64:]
    d1, d2 = v0_dist2(Q1, R, k), v0_dist2(Q2, R, k)
    r1, r2 = eo.radii_of(d1), eo.radii_of(d2, first_kind=4)
    cap = max(kind_max(r1, "held"), float(r2[(0 - 4) % 9::9].max()))
    Q = np.concatenate([np.tile(Q1, (m1 // 64, 1)), Q2])
    r = np.concatenate([np.tile(r1, m1 // 64), r2])
    eo.assert_no_shared_radius_passes(d1, r1, cap)
    eo.assert_no_shared_radius_passes(d2, r2, cap)
    eo.assert_a_stale_pointer_fails(d2, r2, r[:m2], cap)
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        counts, off, fill, keys, stats = pipeline([ix], dev_f32(Q), dev_f32(r), m1 + m2, cap=cap, cells=True)
        assert all(st[0] == 4 and st[2] == 0 for st in stats), stats
        w1, w2 = eo.lists_of(d1, r1, cap, base=BASE), eo.lists_of(d2, r2, cap, base=BASE)
        np.testing.assert_array_equal(counts[:m1].reshape(-1, 64), np.tile(eo.lengths(w1), (m1 // 64, 1)))
        np.testing.assert_array_equal(counts[m1:], eo.lengths(w2))
        np.testing.assert_array_equal(fill, counts)
        assert_segments(off, keys, w1, msg="first pass")
        assert_segments(off[m1:], keys, w2, msg="second pass")
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [FP16, BINS], ids=["fp16", "bins"])
def test_a_far_away_query_falls_back_exact_and_the_next_batch_is_pruned_again(opts):
    rng = np.random.default_rng(45)
    k, m = 16, 70
    R = rng.random((N17, k), dtype=np.float32)
    R[10, 3] = np.nan
    R[20, 0] = np.inf
    R[30] = 3e38
    Q = spread_queries(rng, m, k)
    Qfar = Q.copy()
    Qfar[0] = 1e6                      # a far-away query whose radius ("held") has candidates: nothing bounds it
    d, dfar = v0_dist2(Q, R, k), v0_dist2(Qfar, R, k)
    r = eo.radii_of(d)
    cap = kind_max(r, "held")
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for Qx, dx, fell in ((Qfar, dfar, 1), (Q, d, 0)):
            lists = eo.lists_of(dx, r, cap, base=BASE)
            counts, off, fill, keys, stats = pipeline([ix], dev_f32(Qx), dev_f32(r), m, cap=cap, cells=True)
            assert all(st[0] == 4 and st[2] == fell for st in stats), (fell, stats)
            np.testing.assert_array_equal(counts, eo.lengths(lists))
            np.testing.assert_array_equal(fill, counts)
            assert_segments(off, keys, lists, msg=f"fell back: {fell}")
        assert eo.counts_of(dfar, r, cap)[0] == 0 and eo.counts_of(d, r, cap)[0] > 0
    finally:
        ix.close()
