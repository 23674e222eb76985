"""knn_index_count_within_each and knn_index_list_within_each on the uniform-grid index (KNN_QUERY_COUNT_GRID) on the GPU against
tests/each_oracle.py.  Bar: exact counts and sorted lists at every kind of radius; knn_index_last_stats tells the way and whether
the batch gave up ([2])."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.count_helper import dev_counts
from tests.each_helper import assert_segments, count_each, dev_f32, pipeline
from tests.test_within_grid_gpu import rows_and_queries
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
BASE = 5
INF = float("inf")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_kind_of_radius_on_the_smallest_shard_that_gets_a_grid(k):
    n, m = 16384, 70
    R, Q = rows_and_queries(k, n, m, 300 + k)
    d = v0_dist2(Q, R, k)
    r = eo.radii_of(d)
    eo.assert_every_kind_of_count(eo.counts_of(d, r))
    eo.assert_no_shared_radius_passes(d, r)
    cap = float(r[(r < np.inf)].max())                # finite, and one of the oracle's radii: cap's rings end every walk
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for c in (cap, INF):
            lists = eo.lists_of(d, r, c, base=BASE)
            eo.assert_every_kind_of_count(eo.lengths(lists))
            counts, off, fill, keys, stats = pipeline([ix], dev_f32(Q), dev_f32(r), m, cap=c, grid=True)
            assert all(st[0] == 3 for st in stats), stats
            if c < INF:
                assert all(st[:3] == [3, 0, 0] for st in stats), stats
            else:
                print(f"k={k}: cap +INF with radii of +INF on the grid way: last_stats {stats}")   # exact, whichever way it ends
            np.testing.assert_array_equal(counts, eo.lengths(lists), err_msg=f"k={k} cap={c}")
            np.testing.assert_array_equal(fill, counts)
            assert_segments(off, keys, lists, msg=f"k={k} cap={c}")
        # a fold adds on the grid way; without the flag the exact scan answers
        want = eo.counts_of(d, r, cap)
        held = np.arange(m, dtype=np.uint32) * 3
        np.testing.assert_array_equal(count_each(ix, Q, r, cap=cap, counts=dev_counts(m, fill=held), init=False, grid=True), held + want)
        np.testing.assert_array_equal(count_each(ix, Q, r, cap=cap), want)
        assert ix.last_stats()[:3] == [1, 0, 0]
        # queries that can have no hit — a NaN radius, a negative one, a non-finite coordinate — count 0 and make nobody give up
        rbad, Qbad = r.copy(), Q.copy()
        rbad[np.isinf(rbad)] = np.nan
        rbad[0::9] = -1.0
        Qbad[7, 0] = np.nan
        Qbad[9, k - 1] = np.inf
        dbad = d.copy()
        dbad[[7, 9]] = np.nan
        want_bad = eo.counts_of(dbad, rbad, cap)
        assert (want_bad[np.isnan(rbad) | (rbad < 0)] == 0).all() and (want_bad > 0).any()
        for c in (cap, INF):
            np.testing.assert_array_equal(count_each(ix, Qbad, rbad, cap=c, grid=True), want_bad)
            st = ix.last_stats()
            if c < INF:
                assert st[:3] == [3, 0, 0], st
            else:
                print(f"k={k}: cap +INF, every radius finite, NaN or negative: last_stats {st}")
        none = np.where(np.arange(m) % 2 == 0, np.nan, -1.0).astype(np.float32)      # nobody has a candidate: nothing to walk
        np.testing.assert_array_equal(count_each(ix, Q, none, grid=True), np.zeros(m, np.uint32))
        assert ix.last_stats()[:3] == [3, 0, 0], ix.last_stats()
        # option path = 1: the flag is accepted and the stats show way 1
        pkg.set_option("path", 1)
        np.testing.assert_array_equal(count_each(ix, Q, r, cap=cap, grid=True), want)
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_ties_at_the_boundary_on_a_lattice_with_alternating_radii():
    """The lattice of tests/test_count_grid_gpu.py: the radii alternate between a lattice distance — runs of ties at the boundary,
    all inside — and one ulp below it."""
    rng = np.random.default_rng(21)
    k, n = 3, 4000
    R = rng.integers(0, 3, (n, k)).astype(np.float32)
    R[rng.choice(n, 100, replace=False)] = R[17]
    Q = np.concatenate([rng.integers(0, 3, (60, k)).astype(np.float32),
                        (rng.integers(0, 6, (70, k)) * 0.5 - 0.25).astype(np.float32),
                        R[17:18]])
    m = Q.shape[0]
    d = v0_dist2(Q, R, k)
    pkg.set_option("path", 3)
    ix = pkg.KnnIndex(k, R)
    try:
        for d2 in (0.1875, 0.6875):
            at, below = np.float32(d2), np.nextafter(np.float32(d2), np.float32(0))
            for phase in (0, 1):
                r = np.where((np.arange(m) + phase) % 2 == 0, at, below).astype(np.float32)
                lists = eo.lists_of(d, r, float(at))
                counts, off, fill, keys, stats = pipeline([ix], dev_f32(Q), dev_f32(r), m, cap=float(at), grid=True)
                assert all(st[0] == 3 for st in stats), stats
                np.testing.assert_array_equal(counts, eo.lengths(lists), err_msg=f"d2={d2} phase={phase}")
                assert_segments(off, keys, lists, msg=f"d2={d2} phase={phase}")
        c_at = eo.counts_of(d, np.full(m, 0.1875, np.float32))
        c_below = eo.counts_of(d, np.full(m, np.nextafter(np.float32(0.1875), np.float32(0))))
        assert (c_at > 64).any() and (c_at - c_below > 64).any()        # more than 64 ties at the boundary
        eo.assert_no_shared_radius_passes(d, np.where(np.arange(m) % 2 == 0, np.float32(0.1875),
                                                      np.nextafter(np.float32(0.1875), np.float32(0))).astype(np.float32))
    finally:
        ix.close()
