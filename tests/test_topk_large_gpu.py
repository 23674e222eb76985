"""Top-K beyond 64 (knn_index_query_topk_large, include/knn_mi355x.h 2f) on the GPU against the numpy restatement of v0
(tests/topk_oracle.py, clipped with tests/within_helper.clip): every compiled form of the select and fill scans, K from 1 to 4096,
several slices and a second (clamped) wave of queries, NaN / +INF / 3e38 rows, every radius, cuts inside and outside a class of
equal distances, folds of index-range and cell-range shards, the any-K merge, the small ends, slot reuse, the chunk boundary and
the host call.  Bar: bit-exact keys."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count
from tests.shards_helper import Shards
from tests.test_count_exact_gpu import M, N, TIE_A, TIE_B, batch
from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index, topk_keys, v0_dist2
from tests.within_helper import clip, dev, dev_keys, host_keys, plain, radii, within

pytestmark = pytest.mark.gpu
INF = float("inf")
K_ALL = (1, 17, 64, 65, 100, 1000, N - 3, N, 4096)    # N - 3: exactly the finite rows; N and 4096: padded
K_FEW = (65, 1000)
FORMS = [1, 3, 16, 17, 32, 33, 128, 129]               # KC 1, 2, 3, 8 full and partial, KC 0


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


def large(ix, Q, K, r2=INF, keys=None, init=True, slot=0):
    """One call of query_topk_large: keys [m][K] (numpy uint64) after it; the indices it unpacked are those of the keys."""
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(dev())
    if keys is None:
        keys = dev_keys(m, K, fill=np.full(m * K, 0xDEADBEEFDEADBEEF, dtype=np.uint64) if init else np.full(m * K, KEY_INIT))
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    ix.query_topk_large(m, K, q_d.data_ptr(), keys.data_ptr(), max_dist2=r2, init_keys=init, indices_dev=ind.data_ptr(), slot=slot)
    torch.cuda.synchronize()
    got = host_keys(keys, m, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return got


def fold_of(held, want):
    """The K smallest of the caller's keys and a shard's list."""
    return np.sort(np.concatenate([held, want], axis=1), axis=1)[:, :want.shape[1]]


@pytest.mark.parametrize("k", FORMS)
def test_every_compiled_form_and_every_k(k):
    R, Q = batch(k, 8000 + k)
    full = topk_keys(Q, R, k, 4096, base=9)            # the whole order of every query: a prefix of it is the top-K
    assert ((full != KEY_INIT).sum(axis=1) == N - 3).all()
    ix = pkg.KnnIndex(k, R, base_index=9)
    try:
        for K in (K_ALL if k in (3, 17) else K_FEW):
            got = large(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 1 and st[1] == 0 and st[2] in (0, 1) and st[3] == 0, st
            np.testing.assert_array_equal(got, full[:, :K], err_msg=f"k={k} K={K}")
    finally:
        ix.close()


def test_k_up_to_64_equals_the_radius_bounded_call_bit_for_bit():
    k = 17
    R, Q = batch(k, 8100)
    Q = np.concatenate([Q, Q[:2]])
    Q[-2, 4] = np.nan                                   # a query with a NaN coordinate
    Q[-1] = 1e30                                        # ... and one whose distances overflow
    want = topk_keys(Q[:M], R, k, 64)
    r2 = radii(want)[0][1]
    ix = pkg.KnnIndex(k, R)
    try:
        for K in (1, 17, 64):
            for r in (INF, r2):
                ref = within(ix, Q, K, r)
                got = large(ix, Q, K, r)
                np.testing.assert_array_equal(got, ref, err_msg=f"K={K} r2={r}")
                np.testing.assert_array_equal(got[:M], clip(want[:, :K], r))
                assert (got[M:] == KEY_INIT).all()
    finally:
        ix.close()


def test_every_radius_at_k_100():
    k, K = 3, 100
    R, Q = batch(k, 8200)
    want = topk_keys(Q, R, k, K, base=9)
    d = v0_dist2(Q, R, k)
    tie = np.float32(d[3, TIE_A])
    assert d[3, TIE_A] == d[3, TIE_B]
    ix = pkg.KnnIndex(k, R, base_index=9)
    try:
        for name, r2 in radii(want) + [("tie", float(tie)), ("tie_below", float(np.nextafter(tie, np.float32(0))))]:
            got = large(ix, Q, K, r2)
            np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"{name} r2={r2}")
            assert ix.last_stats()[0] == 1
        # -0 counts as 0
        np.testing.assert_array_equal(large(ix, Q, K, -0.0), clip(want, 0.0))
    finally:
        ix.close()


@pytest.mark.parametrize("K", [65, 500])
def test_a_cut_inside_a_class_of_equal_distances_runs_the_index_passes(K):
    rng = np.random.default_rng(8300 + K)
    k, n, m = 3, 3000, 70
    R = rng.integers(0, 4, size=(n, k)).astype(np.float32)      # the integer lattice {0..3}^3: about 47 copies of each point
    Q = rng.integers(0, 4, size=(m, k)).astype(np.float32)
    more = topk_keys(Q, R, k, K + 1)
    assert (keys_dist2(more[:, K - 1]) == keys_dist2(more[:, K])).any()      # the K-th and the (K+1)-th share a distance word
    ix = pkg.KnnIndex(k, R)
    try:
        got = large(ix, Q, K)
        assert ix.last_stats() == [1, 0, 1, 0], ix.last_stats()
        np.testing.assert_array_equal(got, more[:, :K])
    finally:
        ix.close()


@pytest.mark.parametrize("K", [65, 500])
def test_no_cut_inside_a_class_leaves_the_index_passes_gated_off(K):
    rng = np.random.default_rng(8400 + K)
    k, n, m = 16, N, M
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    more = topk_keys(Q, R, k, K + 1)
    assert (keys_dist2(more[:, K - 1]) != keys_dist2(more[:, K])).all()
    ix = pkg.KnnIndex(k, R)
    try:
        got = large(ix, Q, K)
        assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()
        np.testing.assert_array_equal(got, more[:, :K])
    finally:
        ix.close()


@pytest.mark.parametrize("K", [100, 4096])
def test_two_index_range_shards_fold_to_the_whole_set(K):
    k = 17
    R, Q = batch(k, 8500)
    R[1600] = R[20]                                     # a cross-shard duplicate: the tie is decided by the global number
    want = topk_keys(Q, R, k, K)
    assert (keys_index(want) == 20).any() and (keys_index(want) == 1600).any()
    a, b = pkg.KnnIndex(k, R[:1500]), pkg.KnnIndex(k, R[1500:], base_index=1500)
    try:
        keys = dev_keys(M, K)
        large(a, Q, K, keys=keys, init=True)
        np.testing.assert_array_equal(large(b, Q, K, keys=keys, init=False), want)
        # the other order, the second shard's call folding into the first's lists
        keys = dev_keys(M, K)
        large(b, Q, K, keys=keys, init=True)
        np.testing.assert_array_equal(large(a, Q, K, keys=keys, init=False), want)
        # a radius: the caller's keys — below it and beyond it — are not clipped
        r2 = radii(want[:, :100])[0][1]
        held = np.full((M, K), KEY_INIT, dtype=np.uint64)
        held[:, 0] = (np.uint64(np.float32(r2 * 0.5).view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFF00)
        held[::2, 1] = (np.uint64(np.float32(r2 * 4.0).view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFF01)
        keys = dev_keys(M, K, fill=held)
        large(a, Q, K, r2, keys=keys, init=False)
        got = large(b, Q, K, r2, keys=keys, init=False)
        np.testing.assert_array_equal(got, fold_of(held, clip(want, r2)))
        assert (got == held[0, 0]).any() and (got[::2] == held[0, 1]).any()
    finally:
        a.close()
        b.close()


def test_a_cell_range_shard_pair_folds_to_the_global_list_with_gids():
    rng = np.random.default_rng(8600)
    k, n, m, K = 16, (1 << 19) + 5, 24, 100
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    want = topk_keys(Q, R, k, K)                        # the keys carry global row numbers: the ranks' gids
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=False)      # no seed layer attached
    try:
        keys = dev_keys(m, K)
        for r, ix in enumerate(sh.idx):
            got = large(ix, Q, K, keys=keys, init=(r == 0))
            assert ix.last_stats()[0] == 1
        np.testing.assert_array_equal(got, want)
        assert int(keys_index(want).max()) >= sh.rows[0].shape[0]      # numbers no local row of rank 0 has
    finally:
        sh.close()


def sorted_lists(rng, m, K, real):
    """m sorted lists of K keys: real[j] distinct keys below KEY_INIT, then padding."""
    out = np.full((m, K), KEY_INIT, dtype=np.uint64)
    for j in range(m):
        d = rng.integers(0x30000000, 0x40000000, size=real[j], dtype=np.uint64)
        out[j, :real[j]] = np.sort((d << np.uint64(32)) | rng.permutation(1 << 20)[:real[j]].astype(np.uint64))
    return out


@pytest.mark.parametrize("K", [8, 65, 4096])
def test_the_any_k_merge_in_place(K):
    rng = np.random.default_rng(8700 + K)
    m = 6
    A = sorted_lists(rng, m, K, [K, K // 2, 0, 1, K, K - 1])
    B = sorted_lists(rng, m, K, [K, K // 3, K, 0, 0, 2])
    B[4] = A[4]                                         # the same list twice: equal keys get distinct places
    a_d, b_d = dev_keys(m, K, fill=A), dev_keys(m, K, fill=B)
    pkg.keys_topk_merge_large(a_d.data_ptr(), b_d.data_ptr(), m, K)
    torch.cuda.synchronize()
    want = np.sort(np.concatenate([A, B], axis=1), axis=1)[:, :K]
    np.testing.assert_array_equal(host_keys(b_d, m, K), want)
    np.testing.assert_array_equal(host_keys(a_d, m, K), A)
    if K == 8:                                          # the 64-key merge gives the same lists where keys are distinct
        rows = [0, 1, 2, 3, 5]
        b2 = dev_keys(m, K, fill=B)
        pkg.keys_topk_merge(a_d.data_ptr(), b2.data_ptr(), m, K)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host_keys(b2, m, K)[rows], want[rows])


def test_the_small_ends():
    rng = np.random.default_rng(8800)
    k = 3
    R = rng.random((2000, k), dtype=np.float32)
    Q = rng.random((12, k), dtype=np.float32)
    ix, one, few = pkg.KnnIndex(k, R), pkg.KnnIndex(k, R[:1], base_index=3), pkg.KnnIndex(k, R[:64])
    empty = pkg.KnnIndex(k, R[:0], n_local=0)
    try:
        np.testing.assert_array_equal(large(ix, Q[:1], 200), topk_keys(Q[:1], R, k, 200))                # m = 1
        for K in (1, 65):
            np.testing.assert_array_equal(large(one, Q, K), topk_keys(Q, R[:1], k, K, base=3))           # n = 1
        np.testing.assert_array_equal(large(few, Q, 65), topk_keys(Q, R[:64], k, 65))                    # n = 64, K = 65
        assert (large(few, Q, 65)[:, 64] == KEY_INIT).all()
        # an empty shard leaves the keys alone, or writes padding under the init flag
        held = topk_keys(Q, R, k, 70)
        np.testing.assert_array_equal(large(empty, Q, 70, keys=dev_keys(12, 70, fill=held), init=False), held)
        assert (large(empty, Q, 70, init=True) == KEY_INIT).all()
        assert empty.last_stats() == [1, 0, 0, 0]
    finally:
        for i in (ix, one, few, empty):
            i.close()


def test_calls_of_every_kind_follow_one_another_on_a_slot():
    k, K, slot = 3, 300, 5
    R, Q = batch(k, 8900)
    d = v0_dist2(Q, R, k)
    r2 = float(np.median(d[np.isfinite(d)])) * 0.1
    want = topk_keys(Q, R, k, K)
    ix = pkg.KnnIndex(k, R)
    try:
        solo_top = plain(ix, Q, 8, slot=slot)
        solo_count = count(ix, Q, r2, slot=slot)
        np.testing.assert_array_equal(solo_top, want[:, :8])
        np.testing.assert_array_equal(solo_count, ((d <= np.float32(r2)) & np.isfinite(d)).sum(axis=1))
        np.testing.assert_array_equal(large(ix, Q, K, slot=slot), want)
        np.testing.assert_array_equal(plain(ix, Q, 8, slot=slot), solo_top)
        np.testing.assert_array_equal(count(ix, Q, r2, slot=slot), solo_count)
        np.testing.assert_array_equal(large(ix, Q, K, slot=slot), want)
        np.testing.assert_array_equal(large(ix, Q, K, r2, slot=slot), clip(want, r2))
    finally:
        ix.close()


def test_the_chunk_boundary_at_65536_queries():
    rng = np.random.default_rng(9000)
    k, n, m, K = 3, 1200, 65537, 65
    assert pkg.debug_topk_large_plan(k=k, m=m, K=K, rows=n, num_cu=256, init=1)["chunks"] == 2
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    picked = np.unique(np.concatenate([np.arange(64), np.arange(m - 64, m), [65535, 65536], rng.integers(0, m, size=200)]))
    want = topk_keys(Q[picked], R, k, K)
    ix = pkg.KnnIndex(k, R)
    try:
        got = large(ix, Q, K)
        np.testing.assert_array_equal(got[picked], want)
        assert (got[:, 1:] > got[:, :-1]).all()
    finally:
        ix.close()


def test_the_host_call():
    k, K = 17, 130
    R, Q = batch(k, 9100)
    want = topk_keys(Q, R, k, K, base=4)
    r2 = radii(want[:, :100])[0][1]
    ix = pkg.KnnIndex(k, R, base_index=4)
    try:
        for r in (INF, r2):
            w = clip(want, r)
            idx, d2, counts = ix.query_topk_large_host(Q, K, r)
            np.testing.assert_array_equal(idx, keys_index(w))
            np.testing.assert_array_equal(d2.view(np.uint32), keys_dist2(w).view(np.uint32))
            np.testing.assert_array_equal(counts, (w != KEY_INIT).sum(axis=1))
            assert np.isinf(d2[w == KEY_INIT]).all()
        assert (counts < K).any()
    finally:
        ix.close()
