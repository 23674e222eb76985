"""Radius-bounded top-K on the uniform-grid index (knn_index_query_topk_within with KNN_QUERY_TOPK_GRID) on the GPU against the
numpy restatement of v0 (tests/topk_oracle.py), clipped at the radius.  Bar: bit-exact keys at every radius, the unpacked indices
those of the keys, and knn_index_last_stats telling the way (3) and whether the batch gave up ([2])."""
import ctypes

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index, topk_keys
from tests.within_helper import KS, clip, dev, dev_keys, host_keys, kinds, lengths, plain, radii, within

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


def rows_and_queries(k, n, m, seed):
    """Half the rows uniform in the unit box, half in a cluster about three cells of the grid wide (tighter, one cell would hold
    more rows than a grid index takes, and on one axis queries would coincide with rows in fp32), queries in both, and four queries
    just outside the box, near enough for the plain K = 64 walk to finish: at one radius a query of the cluster has K rows inside,
    its neighbour fewer, one outside none."""
    rng = np.random.default_rng(seed)
    wide = np.float32({1: 0.05, 2: 0.04, 3: 0.17, 4: 0.35}[k])
    c = (0.3 + 0.3 * rng.random(k)).astype(np.float32)
    R = rng.random((n, k), dtype=np.float32)
    R[n // 2:] = c + wide * rng.random((n - n // 2, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Q[m // 2:] = c + wide * rng.random((m - m // 2, k), dtype=np.float32)
    Q[:4, 0] = np.float32(1.0 + {1: 0.004, 2: 0.05, 3: 0.15, 4: 0.3}[k])
    return R, Q


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_every_radius_on_the_smallest_shard_that_gets_a_grid(k):
    n, m = 16384, 70
    R, Q = rows_and_queries(k, n, m, 300 + k)
    want64 = topk_keys(Q, R, k, 64, base=5)
    ix = pkg.KnnIndex(k, R, base_index=5)
    try:
        for K in KS:
            want = want64[:, :K]
            for name, r2 in radii(want):
                got = within(ix, Q, K, r2, grid=True)
                st = ix.last_stats()
                assert st[:3] == [3, 0, 0], (K, name, st)
                np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"k={k} K={K} {name} r2={r2}")
            np.testing.assert_array_equal(within(ix, Q, K, float("inf"), grid=True), plain(ix, Q, K, grid=True))
        # -0 counts as 0, and without the flag the call goes where the plain call goes: the exact top-K, the same keys
        np.testing.assert_array_equal(within(ix, Q, 8, -0.0, grid=True), clip(want64[:, :8], 0.0))
        r2 = radii(want64[:, :8])[0][1]
        np.testing.assert_array_equal(within(ix, Q, 8, r2), clip(want64[:, :8], r2))
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_ties_at_the_boundary_on_a_lattice():
    """The lattice of test_ties_across_rings: the radius exactly a lattice distance — runs of ties at the boundary, all inside,
    the lowest numbers first — and one ulp below it; radius 0 keeps the duplicates of a query that sits on a row."""
    rng = np.random.default_rng(21)
    k, n = 3, 4000
    R = rng.integers(0, 3, (n, k)).astype(np.float32)
    R[rng.choice(n, 100, replace=False)] = R[17]
    Q = np.concatenate([rng.integers(0, 3, (60, k)).astype(np.float32),                # on the lattice
                        (rng.integers(0, 6, (70, k)) * 0.5 - 0.25).astype(np.float32),   # between its points and just outside
                        R[17:18]])
    want64 = topk_keys(Q, R, k, 64)
    pkg.set_option("path", 3)
    ix = pkg.KnnIndex(k, R)
    try:
        for K in KS:
            want = want64[:, :K]
            # lattice distances: 0.1875 = 3 x 0.25^2, the nearest point of an off-lattice query (its ~150 rows tie there: the K
            # lowest numbers stay), 0.6875 the next one, 0 the copies of a query that sits on a point
            for d2 in (0.1875, 0.6875, 0.0):
                for r2 in (np.float32(d2), np.nextafter(np.float32(d2), np.float32(0))):
                    if r2 < 0:
                        continue
                    got = within(ix, Q, K, float(r2), grid=True)
                    assert ix.last_stats()[0] == 3, ix.last_stats()
                    np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"K={K} r2={r2}")
        assert (keys_dist2(want64[:, 63]) == 0.1875).any()   # the case is what it says: 64 and more ties at the boundary
        assert kinds(want64, 0.0)[0] and kinds(want64, 0.0)[2]   # radius 0: queries with no duplicate and with 64 and more
    finally:
        ix.close()


def test_a_radius_ends_the_walk_where_the_plain_call_gives_up():
    """The construction of test_give_up_hands_the_batch_to_the_exact_top_k_once (k 1, a query two box widths out, the near end of
    the box empty).  With a radius below that query's nearest distance its walk ends at the first face bound: its list is all
    padding and the batch does NOT give up ([2] = 0), the others are exact.  With +INF the batch still gives up and is exact.  With
    a radius that spans more rings than the cell budget allows the plan keeps the plain rmax: the query gives up, and the exact
    top-K that answers the batch carries the limit — exact AND clipped."""
    rng = np.random.default_rng(5)
    k, n, K, base = 1, 16384, 8, 300
    R = (0.5 + 0.5 * rng.random((n, k))).astype(np.float32)
    R[0] = 0.0
    lo, width = float(R.min()), float(R.max() - R.min())
    Q = (0.6 + 0.3 * rng.random((21, k))).astype(np.float32)
    Q[11] = lo - 2.0 * width
    want = topk_keys(Q, R, k, K, base=base)
    nearest = float(keys_dist2(want)[11, 0])
    inside = float(np.median(keys_dist2(want)[np.arange(21) != 11, K // 2]))   # cuts the other queries' lists
    ix = pkg.KnnIndex(k, R, base_index=base)
    try:
        assert inside < nearest
        for r2 in (inside, float(np.nextafter(np.float32(nearest), np.float32(0)))):
            for init in (True, False):
                held = np.full((21, K), KEY_INIT)
                got = within(ix, Q, K, r2, grid=True, init=init, keys=None if init else dev_keys(21, K, fill=held))
                assert ix.last_stats()[:3] == [3, 0, 0], (r2, init, ix.last_stats())
                assert (got[11] == KEY_INIT).all()
                np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"r2={r2} init={init}")
        others = np.arange(21) != 11
        assert (lengths(want, inside)[others] < K).any() and (lengths(want, inside)[others] > 0).any()
        got = within(ix, Q, K, float("inf"), grid=True)
        assert ix.last_stats()[:3] == [3, 0, 1], ix.last_stats()
        np.testing.assert_array_equal(got, want)
        # a second query 20 box widths out and a radius that keeps 4 of its 8 rows: ~110000 rings of the one axis, beyond the
        # 2^15-cell budget (16383 rings)
        Q2 = Q.copy()
        Q2[12] = lo - 20.0 * width
        want2 = topk_keys(Q2, R, k, K, base=base)
        far = float(keys_dist2(want2)[12, 3])
        assert lengths(want2, far)[12] == 4 and (lengths(want2, far)[np.arange(21) != 12] == K).all()
        rings = int(np.sqrt(far) / (width / 5000))
        assert rings > 16383
        assert pkg.debug_grid_within_plan(k=k, K=K, m=21, has_grid=1, path=0, flag=1, radius_rings=rings)["rmax"] == \
            pkg.debug_grid_topk_plan(k=k, K=K, m=21, has_grid=1, path=0, flag=1)["rmax"]
        for init in (True, False):
            other = topk_keys(Q2, rng.random((500, k), dtype=np.float32), k, K, base=base + n)   # another shard's keys: they stay
            got = within(ix, Q2, K, far, grid=True, init=init, keys=None if init else dev_keys(21, K, fill=other))
            assert ix.last_stats()[:3] == [3, 0, 1], ix.last_stats()
            exp = clip(want2, far)
            if not init:
                exp = np.sort(np.concatenate([exp, other], axis=1), axis=1)[:, :K]
            np.testing.assert_array_equal(got, exp, err_msg=f"beyond the budget, init={init}")
        got = within(ix, Q[:11], K, inside, grid=True)   # the next batch on the slot finds its word cleared
        assert ix.last_stats()[:3] == [3, 0, 0]
        np.testing.assert_array_equal(got, clip(want[:11], inside))
    finally:
        ix.close()


def test_non_finite_queries_a_fold_with_keys_beyond_the_radius_and_two_slots():
    rng = np.random.default_rng(44)
    k, n, m = 3, 2 * 16384, 50
    R, Q = rows_and_queries(k, n, m, 44)
    perm = rng.permutation(n)
    R = R[perm]                                   # both shards hold rows of the cluster
    Qbad = Q.copy()
    Qbad[7, 1] = np.nan
    Qbad[9, 0] = np.inf
    a = pkg.KnnIndex(k, R[:n // 2], base_index=0)
    b = pkg.KnnIndex(k, R[n // 2:], base_index=n // 2)
    try:
        for K in (1, 8, 64):
            want_a = topk_keys(Q, R[:n // 2], k, K)
            want_b = topk_keys(Q, R[n // 2:], k, K, base=n // 2)
            r2 = radii(want_b)[0][1]
            # non-finite queries: all padding, nothing gives up
            got = within(b, Qbad, K, r2, grid=True)
            assert b.last_stats()[:3] == [3, 0, 0]
            exp = clip(want_b, r2)
            exp[[7, 9]] = KEY_INIT
            np.testing.assert_array_equal(got, exp)
            # the fold: shard a's PLAIN keys are held — keys beyond the radius among them — and stay; shard b adds its capped rows
            assert (keys_dist2(want_a)[want_a != KEY_INIT] > np.float32(r2)).any()
            got = within(b, Q, K, r2, grid=True, init=False, keys=dev_keys(m, K, fill=want_a))
            assert b.last_stats()[:3] == [3, 0, 0]
            exp = np.sort(np.concatenate([want_a, clip(want_b, r2)], axis=1), axis=1)[:, :K]
            np.testing.assert_array_equal(got, exp, err_msg=f"fold K={K}")
        # two slots in flight on two streams
        K = 17
        Qs = [Q, Q[::-1].copy()]
        wants = [topk_keys(q, R[:n // 2], k, K) for q in Qs]
        r2 = radii(wants[0])[0][1]
        streams = [torch.cuda.Stream(device=dev()) for _ in range(2)]
        q_d = [torch.from_numpy(q.reshape(-1)).to(dev()) for q in Qs]
        held = [(dev_keys(m, K), torch.full((m * K,), -7, dtype=torch.int32, device=dev())) for _ in range(2)]
        torch.cuda.synchronize()
        for j in range(2):
            a.query_topk_within(m, K, q_d[j].data_ptr(), r2, held[j][0].data_ptr(), init_keys=True, indices_dev=held[j][1].data_ptr(),
                                slot=j, stream=streams[j].cuda_stream, grid=True)
        torch.cuda.synchronize()
        assert a.last_stats()[:3] == [3, 0, 0]
        for j, (keys, ind) in enumerate(held):
            got = host_keys(keys, m, K)
            np.testing.assert_array_equal(got, clip(wants[j], r2), err_msg=f"slot {j}")
            np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    finally:
        a.close()
        b.close()


def test_a_negative_or_nan_radius_is_einval_and_launches_nothing():
    rng = np.random.default_rng(8)
    k, n, m, K = 2, 16384, 12, 8
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R)
    try:
        q_d = torch.from_numpy(Q.reshape(-1)).to(dev())
        keys = dev_keys(m, K, fill=np.full((m, K), 123))
        L = pkg.lib()
        vp = ctypes.c_void_p
        for bad in (-1.0, float("nan"), -float("inf")):
            for flags in (pkg.QUERY_INIT_KEYS, pkg.QUERY_INIT_KEYS | pkg.QUERY_TOPK_GRID, 0):
                assert L.knn_index_query_topk_within(ix._h, 0, m, K, vp(q_d.data_ptr()), bad, vp(keys.data_ptr()), None, None,
                                                     flags) == -1   # KNN_EINVAL
            with pytest.raises(pkg.KnnError, match="knn_index_query_topk_within"):
                ix.query_topk_within(m, K, q_d.data_ptr(), bad, keys.data_ptr(), init_keys=True, grid=True)
            with pytest.raises(pkg.KnnError, match="knn_index_query_topk_within_host"):
                ix.query_topk_within_host(Q, K, bad)
        # the plain call's bad arguments: K, m, the slot, an unknown flag
        for args in ((0, m, 65, 1), (0, 0, K, 1), (8, m, K, 1), (0, m, K, 16)):
            slot, mm, KK, flags = args
            assert L.knn_index_query_topk_within(ix._h, slot, mm, KK, vp(q_d.data_ptr()), 1.0, vp(keys.data_ptr()), None, None,
                                                 flags) == -1
        torch.cuda.synchronize()
        assert (host_keys(keys, m, K) == 123).all()   # nothing was launched
    finally:
        ix.close()
