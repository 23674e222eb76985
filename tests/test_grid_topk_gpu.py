"""Top-K on the uniform-grid index (KNN_QUERY_TOPK_GRID, include/knn_mi355x.h section 2c) on the GPU against the numpy
restatement of v0 (tests/topk_oracle.py).  Bar: bit-exact keys, in order — distance first, then the lowest global number —, the
unpacked indices those of the keys, and knn_index_last_stats telling the way (3) and whether the batch gave up ([2])."""
import ctypes

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import KEY_INIT, keys_index, topk_keys

pytestmark = pytest.mark.gpu
KS = (1, 2, 8, 17, 64)


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


def _dev():
    return torch.device("cuda:0")


def _keys(m, K, fill=None):
    t = torch.empty(m * K, dtype=torch.int64, device=_dev())
    if fill is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.uint64).reshape(-1).view(np.int64)))
    return t


def _host(keys, m, K):
    return keys.cpu().numpy().view(np.uint64).reshape(m, K)


def _topk(ix, Q, K, keys=None, init=True, slot=0, stream=0, grid=True):
    """One batch: keys [m][K] (numpy uint64) after the call; the indices it unpacked are checked against the keys."""
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    if keys is None:
        keys = _keys(m, K)
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=init, indices_dev=ind.data_ptr(), slot=slot, stream=stream,
                  grid=grid)
    torch.cuda.synchronize()
    got = _host(keys, m, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return got


def _one_nn(ix, Q):
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    keys = torch.empty(m, dtype=torch.int64, device=_dev())
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), init_keys=True)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_uniform_rows_on_the_smallest_shard_that_gets_a_grid(k):
    """n = 16384: the smallest shard the library gives a grid index.  m = 70 leaves the last block two of its four waves; m = 1
    and m = 5 one block and a second one with a single wave."""
    n, m = 16384, 70
    rng = np.random.default_rng(100 + k)
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    want = topk_keys(Q, R, k, 64, base=5)
    ix = pkg.KnnIndex(k, R, base_index=5)
    try:
        for K in KS:
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 3 and st[1] == 0 and st[2] == 0 and st[3] == 0, (K, st)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"k={k} K={K}")
        for mm in (1, 5):
            np.testing.assert_array_equal(_topk(ix, Q[:mm], 8), want[:mm, :8], err_msg=f"m={mm}")
            assert ix.last_stats()[0] == 3
        one = _one_nn(ix, Q)
        assert ix.last_stats()[:3] == [3, 0, 0]
        np.testing.assert_array_equal(_topk(ix, Q, 1)[:, 0], one)
        # without the flag the call goes where it went before: the exact top-K scan, same keys
        np.testing.assert_array_equal(_topk(ix, Q, 8, grid=False), want[:, :8])
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_ties_across_rings():
    """A lattice of three values per axis, 100 copies of one row: rows at equal distance sit in different rings of the walk, and
    the K-th place cuts through runs of equal distances and duplicates; the lowest numbers win."""
    rng = np.random.default_rng(21)
    k, n = 3, 4000
    R = rng.integers(0, 3, (n, k)).astype(np.float32)
    R[rng.choice(n, 100, replace=False)] = R[17]
    Q = np.concatenate([rng.integers(0, 3, (60, k)).astype(np.float32),                # on the lattice
                        (rng.integers(0, 6, (70, k)) * 0.5 - 0.25).astype(np.float32),   # between its points and just outside
                        R[17:18]])
    want = topk_keys(Q, R, k, 64)
    pkg.set_option("path", 3)
    ix = pkg.KnnIndex(k, R)
    try:
        for K in KS:
            np.testing.assert_array_equal(_topk(ix, Q, K), want[:, :K], err_msg=f"K={K}")
            assert ix.last_stats()[0] == 3, ix.last_stats()
    finally:
        ix.close()


def test_whole_grid_seen_and_non_finite_queries():
    """100 rows (and 64: exactly K) under K = 64: the rings cover every cell of the grid before the stop rule can hold.  NaN / Inf
    queries: every distance is NaN or +INF, the list is all KNN_KEY_INIT and nothing gives up.  Last, a finite query whose
    distances all overflow: the walk ends with the whole grid seen and no real key."""
    rng = np.random.default_rng(3)
    k, K = 3, 64
    pkg.set_option("path", 3)
    for n in (100, 64):
        R = rng.random((n, k), dtype=np.float32)
        Q = rng.random((9, k), dtype=np.float32)
        Q[2, 1] = np.nan
        Q[5, 0] = np.inf
        Q[7, 2] = -np.inf
        ix = pkg.KnnIndex(k, R, base_index=1000)
        try:
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 3 and st[2] == 0, st
            np.testing.assert_array_equal(got, topk_keys(Q, R, k, K, base=1000))
            assert (got[[2, 5, 7]] == KEY_INIT).all() and (got[0] < KEY_INIT).all()
        finally:
            ix.close()
    R = rng.random((70, k), dtype=np.float32)
    Q = rng.random((4, k), dtype=np.float32)
    Q[1] = 1.5e19   # d^2 overflows to +INF against every row
    ix = pkg.KnnIndex(k, R)
    try:
        got = _topk(ix, Q, K)
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, K))
        assert (got[1] == KEY_INIT).all()
    finally:
        ix.close()


def test_fold_over_two_index_range_shards():
    """Two shards of one set, each with its own grid index: the second call folds (no KNN_QUERY_INIT_KEYS) into the first one's
    keys and the result is the top-K of the whole set.  The kernel writes its lists to the slot's scratch, never into the
    caller's keys: a query with a NaN coordinate leaves what the keys held."""
    rng = np.random.default_rng(44)
    k, n, m = 3, 2 * 16384, 50
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Qnan = Q.copy()
    Qnan[7, 1] = np.nan
    a = pkg.KnnIndex(k, R[:n // 2], base_index=0)
    b = pkg.KnnIndex(k, R[n // 2:], base_index=n // 2)
    try:
        for K in (1, 8, 64):
            keys = _keys(m, K)
            first = _topk(a, Q, K, keys=keys).copy()
            assert a.last_stats()[0] == 3
            np.testing.assert_array_equal(first, topk_keys(Q, R[:n // 2], k, K))
            got = _topk(b, Q, K, keys=keys, init=False)
            assert b.last_stats()[:3] == [3, 0, 0]
            np.testing.assert_array_equal(got, topk_keys(Q, R, k, K), err_msg=f"K={K}")
            # the NaN query's row of the keys is shard a's answer before and after shard b's fold
            keys = _keys(m, K, fill=first)
            got = _topk(b, Qnan, K, keys=keys, init=False)
            want = topk_keys(Q, R, k, K)
            want[7] = first[7]
            np.testing.assert_array_equal(got, want, err_msg=f"NaN fold K={K}")
    finally:
        a.close()
        b.close()


def test_give_up_hands_the_batch_to_the_exact_top_k_once():
    """k = 1, n = 16384, K = 8: 20 queries inside the rows' box and one two box widths outside it.  On one axis an outside query has
    every row on one side, so with rows at the near end of the box the rule would stop it after a few rings; here that end is
    empty but for the one row that is the box's corner — the first K rows lie ~2730 cells in, far past rmax: the query gives up,
    the batch's word is raised and the gated exact top-K answers the batch (last_stats [2] = 1), with init and as a fold (a row
    folded by both kernels would stand in the keys twice).  The next batch on the slot, all inside, finds its word cleared."""
    rng = np.random.default_rng(5)
    k, n, K, base = 1, 16384, 8, 300
    plan = pkg.debug_grid_topk_plan(k=k, K=K, m=21, has_grid=1, path=0, flag=1)
    assert plan["use"] == 1 and plan["rmax"] + 1 < 5461   # 5461 = floor(n / 3): the grid's cells on the one axis
    R = (0.5 + 0.5 * rng.random((n, k))).astype(np.float32)
    R[0] = 0.0
    lo, width = float(R.min()), float(R.max() - R.min())
    Qin = (0.6 + 0.3 * rng.random((21, k))).astype(np.float32)
    Q = Qin.copy()
    Q[11] = lo - 2.0 * width
    other = rng.random((500, k), dtype=np.float32)   # another shard's rows, numbered from base + n
    held = topk_keys(Q, other, k, K, base=base + n)
    ix = pkg.KnnIndex(k, R, base_index=base)
    try:
        got = _topk(ix, Q, K)
        assert ix.last_stats()[:3] == [3, 0, 1], ix.last_stats()
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, K, base=base))
        got = _topk(ix, Q, K, keys=_keys(21, K, fill=held), init=False)
        assert ix.last_stats()[:3] == [3, 0, 1], ix.last_stats()
        want = np.sort(np.concatenate([topk_keys(Q, R, k, K, base=base), held], axis=1), axis=1)[:, :K]
        np.testing.assert_array_equal(got, want)
        for init in (True, False):
            got = _topk(ix, Qin, K, keys=None if init else _keys(21, K, fill=np.full((21, K), KEY_INIT)), init=init)
            assert ix.last_stats()[:3] == [3, 0, 0], ix.last_stats()
            np.testing.assert_array_equal(got, topk_keys(Qin, R, k, K, base=base))
        got = _topk(ix, Q, K)
        assert ix.last_stats()[2] == 1
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, K, base=base))
    finally:
        ix.close()


def test_skewed_grid_with_a_degenerate_axis():
    """Gaussian rows on two axes, the third constant: one cell per row of the grid on the dead axis, crowded cells in the middle
    and empty ones at the rim.  Exact whether or not a query of the rim gives up."""
    rng = np.random.default_rng(66)
    k, n, m, K = 3, 20000, 40, 64
    R = rng.standard_normal((n, k)).astype(np.float32)
    R[:, 2] = 0.75
    Q = rng.standard_normal((m, k)).astype(np.float32)
    Q[:, 2] = 0.75
    Q[::7, 2] = 0.8      # off the rows' plane
    Q[3, :2] = 6.0       # past the rim
    ix = pkg.KnnIndex(k, R)
    try:
        got = _topk(ix, Q, K)
        assert ix.last_stats()[0] == 3, ix.last_stats()
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, K))
    finally:
        ix.close()


def test_two_batches_in_flight_on_two_slots():
    rng = np.random.default_rng(77)
    k, n, m, K = 2, 16384, 33, 17
    R = rng.random((n, k), dtype=np.float32)
    Qs = [rng.random((m, k), dtype=np.float32) for _ in range(2)]
    streams = [torch.cuda.Stream(device=_dev()) for _ in range(2)]
    ix = pkg.KnnIndex(k, R)
    try:
        q_d = [torch.from_numpy(Q.reshape(-1)).to(_dev()) for Q in Qs]
        held = [(_keys(m, K), torch.full((m * K,), -7, dtype=torch.int32, device=_dev())) for _ in range(2)]
        torch.cuda.synchronize()
        for j in range(2):
            ix.query_topk(m, K, q_d[j].data_ptr(), held[j][0].data_ptr(), init_keys=True, indices_dev=held[j][1].data_ptr(), slot=j,
                          stream=streams[j].cuda_stream, grid=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[:3] == [3, 0, 0]
        for j, (keys, ind) in enumerate(held):
            got = _host(keys, m, K)
            np.testing.assert_array_equal(got, topk_keys(Qs[j], R, k, K), err_msg=f"slot {j}")
            np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    finally:
        ix.close()


def test_flag_where_there_is_no_grid_and_on_the_1nn_entry_points():
    rng = np.random.default_rng(8)
    k, n, m, K = 16, 5000, 12, 8
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R)
    try:
        want = topk_keys(Q, R, k, K)
        np.testing.assert_array_equal(_topk(ix, Q, K, grid=False), want)
        way = ix.last_stats()[0]
        np.testing.assert_array_equal(_topk(ix, Q, K, grid=True), want)
        assert ix.last_stats()[0] == way and way != 3
        q_d = torch.from_numpy(Q.reshape(-1)).to(_dev())
        keys = _keys(m, 1, fill=np.full(m, 123))
        L = pkg.lib()
        vp = ctypes.c_void_p
        for flags in (pkg.QUERY_TOPK_GRID, pkg.QUERY_TOPK_GRID | pkg.QUERY_INIT_KEYS):
            assert L.knn_index_query(ix._h, 0, m, vp(q_d.data_ptr()), vp(keys.data_ptr()), None, None, flags) == -1   # KNN_EINVAL
            assert L.knn_index_query_keys_ex(ix._h, 0, m, vp(q_d.data_ptr()), vp(keys.data_ptr()), None, flags) == -1
        torch.cuda.synchronize()
        assert (_host(keys, m, 1) == 123).all()   # nothing was launched
    finally:
        ix.close()
