"""knn_index_list_within on the uniform-grid index (KNN_QUERY_COUNT_GRID) on the GPU against tests/list_oracle.py, on the shapes of
tests/test_count_grid_gpu.py.  Bar: exact lists and fill at every radius; knn_index_last_stats tells the way (3 with the flag, 1
without) and whether the batch gave up ([2]) — then the exact list answered it, once."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import dev_counts
from tests.count_oracle import radii
from tests.list_helper import PAD, assert_lists, check_list, dev_u64, list_call, segments
from tests.list_oracle import holds_every_kind, kinds, lengths, lists_of, offsets_of
from tests.test_within_grid_gpu import rows_and_queries
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_radius_on_the_smallest_shard_that_gets_a_grid(k):
    n, m = 16384, 70
    R, Q = rows_and_queries(k, n, m, 300 + k)
    d = v0_dist2(Q, R, k)
    want = {name: lists_of(d, r2, base=5) for name, r2 in radii(d)}
    assert holds_every_kind(want.values()) and kinds(want["at"])[:2] == (True, True) and kinds(want["large"])[2]
    ix = pkg.KnnIndex(k, R, base_index=5)
    try:
        for name, r2 in radii(d):
            check_list(ix, Q, r2, want[name], msg=f"k={k} {name} r2={r2} (grid)", grid=True)
            st = ix.last_stats()
            assert st[0] == 3, (name, st)
            if r2 != float("inf"):
                assert st[:3] == [3, 0, 0], (name, st)      # every finite radius of the list ends every walk
            check_list(ix, Q, r2, want[name], msg=f"k={k} {name} r2={r2} (no flag)")
            assert ix.last_stats()[:3] == [1, 0, 0], (name, ix.last_stats())
        # appending on the grid way goes behind the cursor, -0 counts as 0, the cell flag changes nothing here, non-finite queries
        # list nothing
        r2, w = radii(d)[0][1], want["at"]
        cnt = lengths(w)
        held = (np.arange(m, dtype=np.uint32) % 4)
        off = offsets_of(cnt.astype(np.uint64) + held)
        fill, keys = list_call(ix, Q, r2, off, fill=dev_counts(m, fill=held), init=False, grid=True)
        assert ix.last_stats()[:3] == [3, 0, 0]
        np.testing.assert_array_equal(fill, held + cnt)
        for j in range(m):
            assert (keys[int(off[j]):int(off[j]) + int(held[j])] == PAD).all()
            np.testing.assert_array_equal(np.sort(keys[int(off[j]) + int(held[j]):int(off[j + 1])]), w[j])
        check_list(ix, Q, -0.0, lists_of(d, 0.0, base=5), grid=True)
        check_list(ix, Q, r2, w, cells=True)
        assert ix.last_stats()[0] == 1
        Qbad = Q.copy()
        Qbad[7, 0] = np.nan
        Qbad[9, k - 1] = np.inf
        wbad = list(w)
        wbad[7] = wbad[9] = np.zeros(0, dtype=np.uint64)
        check_list(ix, Qbad, r2, wbad, grid=True)
        assert ix.last_stats()[:3] == [3, 0, 0]
        # an overflowing segment on the grid way: fill is the count, nothing leaves the segment
        rooms = np.where(cnt > 0, cnt - 1, 0).astype(np.uint64)
        off = np.concatenate([[np.uint64(1)], np.uint64(1) + np.cumsum(rooms)]).astype(np.uint64)
        fill, keys = list_call(ix, Q, r2, off, keys=dev_u64(np.full(int(off[-1]) + 1, PAD)), grid=True)
        np.testing.assert_array_equal(fill, cnt)
        assert keys[0] == PAD and keys[-1] == PAD
        for j in range(m):
            got = keys[int(off[j]):int(off[j + 1])]
            assert np.isin(got, w[j]).all() and np.unique(got).size == got.size
        # option path = 1: the flag is accepted and the exact list answers
        pkg.set_option("path", 1)
        check_list(ix, Q, r2, w, grid=True)
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_ties_at_the_boundary_on_a_lattice():
    """The lattice of tests/test_count_grid_gpu.py: the radius exactly a lattice distance — runs of ties at the boundary, all
    inside — and one ulp below it; radius 0 lists the copies of a query that sits on a row.  Five more rows sit off the lattice at
    (0.5, ..): the query on them has a list of five, and they tie at 0.1875 with the half-lattice queries around them."""
    rng = np.random.default_rng(21)
    k, n = 3, 4000
    R = rng.integers(0, 3, (n, k)).astype(np.float32)
    R[rng.choice(n, 100, replace=False)] = R[17]
    R = np.concatenate([R, np.full((5, k), 0.5, dtype=np.float32)])      # five rows off the lattice: a short list for the query on them
    Q = np.concatenate([rng.integers(0, 3, (60, k)).astype(np.float32),
                        (rng.integers(0, 6, (70, k)) * 0.5 - 0.25).astype(np.float32),
                        R[17:18], R[-1:]])
    d = v0_dist2(Q, R, k)
    pkg.set_option("path", 3)
    ix = pkg.KnnIndex(k, R)
    try:
        seen = []
        for d2 in (0.1875, 0.6875, 0.0):
            for r2 in (np.float32(d2), np.nextafter(np.float32(d2), np.float32(0))):
                if r2 < 0:
                    continue
                want = lists_of(d, r2)
                seen.append(want)
                check_list(ix, Q, float(r2), want, msg=f"r2={r2}", grid=True)
                assert ix.last_stats()[0] == 3, ix.last_stats()
        at, below = lengths(lists_of(d, 0.1875)), lengths(lists_of(d, np.nextafter(np.float32(0.1875), np.float32(0))))
        assert (at > 64).any() and (at - below > 64).any()        # the case is what it says: more than 64 ties at the boundary
        assert lengths(lists_of(d, 0.0))[-1] == 5 and holds_every_kind(seen)
    finally:
        ix.close()


def test_a_walk_past_the_cell_budget_gives_up_and_the_exact_list_answers_once():
    """The k = 1 construction of tests/test_count_grid_gpu.py: a second query 20 box widths out with a radius that spans more rings
    than the 2^15-cell budget gives up ([2] == 1); the other queries' walks have by then reserved places in the scratch cursor and
    stored keys — the exact list answers the batch from the untouched fill over the same places: the lists are exact and fill is
    the count, not twice it.  The next batch on the slot is back on the grid."""
    rng = np.random.default_rng(5)
    k, n = 1, 16384
    R = (0.5 + 0.5 * rng.random((n, k))).astype(np.float32)
    R[0] = 0.0
    lo, width = float(R.min()), float(R.max() - R.min())
    Q = (0.6 + 0.3 * rng.random((21, k))).astype(np.float32)
    Q[11] = lo - 2.0 * width
    d = v0_dist2(Q, R, k)
    nearest = float(d[11].min())
    inside = float(np.median(np.sort(d[np.arange(21) != 11], axis=1)[:, 4]))
    ix = pkg.KnnIndex(k, R, base_index=300)
    try:
        assert inside < nearest
        for r2 in (inside, float(np.nextafter(np.float32(nearest), np.float32(0)))):
            want = lists_of(d, r2, base=300)
            assert want[11].size == 0
            check_list(ix, Q, r2, want, msg=f"r2={r2}", grid=True)
            assert ix.last_stats()[:3] == [3, 0, 0], (r2, ix.last_stats())
        Q2 = Q.copy()
        Q2[12] = lo - 20.0 * width
        d2 = v0_dist2(Q2, R, k)
        far = float(np.sort(d2[12])[3])
        want = lists_of(d2, far, base=300)
        cnt = lengths(want)
        assert cnt[12] == 4 and (cnt > 64).any()
        for init in (True, False):
            held = np.full(21, 2, np.uint32) if not init else np.zeros(21, np.uint32)
            off = offsets_of(cnt.astype(np.uint64) + held)
            fill, keys = list_call(ix, Q2, far, off, fill=dev_counts(21, fill=np.full(21, 2, np.uint32)), init=init, grid=True)
            assert ix.last_stats()[:3] == [3, 0, 1], ix.last_stats()
            np.testing.assert_array_equal(fill, cnt + held, err_msg=f"beyond the budget, init={init}: fill is exact, not doubled")
            for j in range(21):
                h = int(held[j])
                assert (keys[int(off[j]):int(off[j]) + h] == PAD).all()
                np.testing.assert_array_equal(np.sort(keys[int(off[j]) + h:int(off[j + 1])]), want[j], err_msg=f"init={init} query {j}")
        want = lists_of(d[:11], inside, base=300)    # the next batch on the slot finds its word cleared
        check_list(ix, Q[:11], inside, want, grid=True)
        assert ix.last_stats()[:3] == [3, 0, 0]
    finally:
        ix.close()
