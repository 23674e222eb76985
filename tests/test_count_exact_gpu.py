"""knn_index_count_within on the exact count scan (the default way) on the GPU against tests/count_oracle.py: every compiled form
of knn_exact_count_kernel<KC>, several slices, a second (clamped) wave of queries, rows that are NaN, +INF and 3e38, a boundary tie
across slices, every radius, with and without the init flag, a fold of two shards, m = 1, a non-finite query."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count, dev, dev_counts, host_counts
from tests.count_oracle import counts_of, radii
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
N, M = 3 * 1024 + 77, 70                       # several slices of >= 788 rows; a second wave of 6 queries, its lanes clamped
KS = [1] + [16 * n + j for n in range(1, 9) for j in (0, 1)]   # KC 1 .. 8 full and one dimension into the next; 129: KC 0
TIE_A, TIE_B = 10, 2100                         # two copies of one row, in different slices whatever the slice size >= 788


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


def batch(k, seed):
    """Rows in the unit box with a NaN, a +INF and a 3e38 row and one row held twice; queries inside the box and, one after the
    other, further outside it along the first axis (their nearest distances span a range: one radius leaves counts of 0 and of a
    few rows); the reach grows with k as the distances do."""
    rng = np.random.default_rng(seed)
    R = rng.random((N, k), dtype=np.float32)
    R[5, 0] = np.nan
    R[6, k - 1] = np.inf
    R[7] = 3e38
    R[TIE_B] = R[TIE_A]
    Q = rng.random((M, k), dtype=np.float32)
    Q[:, 0] += np.linspace(0.0, 1.5 if k <= 16 else 4.0, M, dtype=np.float32)
    return R, Q


@pytest.mark.parametrize("k", KS)
def test_every_compiled_form_at_every_radius(k):
    R, Q = batch(k, 7000 + k)
    d = v0_dist2(Q, R, k)
    tie = float(d[3, TIE_A])
    assert d[3, TIE_A] == d[3, TIE_B] and np.isnan(d[:, 5]).all() and np.isinf(d[:, 6]).all() and np.isinf(d[:, 7]).all()
    ix = pkg.KnnIndex(k, R, base_index=9)
    try:
        for name, r2 in radii(d) + [("tie", tie), ("tie_below", float(np.nextafter(np.float32(tie), np.float32(0))))]:
            got = count(ix, Q, r2)
            assert ix.last_stats()[:3] == [1, 0, 0], ix.last_stats()
            np.testing.assert_array_equal(got, counts_of(d, r2), err_msg=f"k={k} {name} r2={r2}")
        assert counts_of(d, tie)[3] - counts_of(d, np.nextafter(np.float32(tie), np.float32(0)))[3] >= 2   # both copies leave together
        assert (counts_of(d, float("inf")) == N - 3).all()
        # a flag on an index without the structure changes nothing
        r2 = radii(d)[0][1]
        np.testing.assert_array_equal(count(ix, Q, r2, grid=True, cells=True), counts_of(d, r2))
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_init_writes_a_fold_adds_and_two_shards_fold_to_the_whole_set():
    k = 17
    R, Q = batch(k, 7100)
    d = v0_dist2(Q, R, k)
    rs = dict(radii(d))
    whole = pkg.KnnIndex(k, R)
    a, b = pkg.KnnIndex(k, R[:1500]), pkg.KnnIndex(k, R[1500:], base_index=1500)
    try:
        for name in ("at", "large", "inf", "zero"):
            r2, want = rs[name], counts_of(d, rs[name])
            c = dev_counts(M, fill=0xDEADBEEF)
            np.testing.assert_array_equal(count(whole, Q, r2, counts=c, init=True), want, err_msg=name)     # = the count
            np.testing.assert_array_equal(count(whole, Q, r2, counts=c, init=False), 2 * want, err_msg=name)   # += the count
            np.testing.assert_array_equal(count(whole, Q, r2, counts=c, init=False), 3 * want, err_msg=name)
            held = np.arange(M, dtype=np.uint32) * 1000
            np.testing.assert_array_equal(count(whole, Q, r2, counts=dev_counts(M, fill=held), init=False), held + want)
            # two index-range shards: the first writes, the second folds
            c = dev_counts(M, fill=0xDEADBEEF)
            count(a, Q, r2, counts=c, init=True)
            np.testing.assert_array_equal(count(b, Q, r2, counts=c, init=False), want, err_msg=f"two shards, {name}")
        # a fold wraps modulo 2^32
        want = counts_of(d, rs["large"])
        got = count(whole, Q, rs["large"], counts=dev_counts(M, fill=0xFFFFFFFF), init=False)
        np.testing.assert_array_equal(got, (want.astype(np.uint64) + 0xFFFFFFFF).astype(np.uint32))
    finally:
        whole.close()
        a.close()
        b.close()


def test_one_query_a_non_finite_query_two_slots_and_the_host_call():
    k = 16
    R, Q = batch(k, 7200)
    d = v0_dist2(Q, R, k)
    rs = dict(radii(d))
    ix = pkg.KnnIndex(k, R)
    try:
        for name in ("at", "large", "inf"):
            r2 = rs[name]
            for j in (0, 33, M - 1):   # m = 1
                np.testing.assert_array_equal(count(ix, Q[j:j + 1], r2), counts_of(d[j:j + 1], r2), err_msg=f"m=1 {name} {j}")
            Qbad = Q.copy()
            Qbad[4, 2] = np.nan
            Qbad[9, 0] = np.inf
            Qbad[66, k - 1] = -np.inf
            want = counts_of(d, r2)
            want[[4, 9, 66]] = 0
            np.testing.assert_array_equal(count(ix, Qbad, r2), want, err_msg=f"non-finite queries, {name}")
            np.testing.assert_array_equal(ix.count_within_host(Q, r2), counts_of(d, r2), err_msg=f"host call, {name}")
        np.testing.assert_array_equal(ix.count_within_host(Q, -0.0), counts_of(d, 0.0))
        # two slots in flight on two streams
        streams = [torch.cuda.Stream(device=dev()) for _ in range(2)]
        Qs = [Q, Q[::-1].copy()]
        q_d = [torch.from_numpy(q.reshape(-1)).to(dev()) for q in Qs]
        held = [dev_counts(M, fill=7) for _ in range(2)]
        torch.cuda.synchronize()
        for j in range(2):
            ix.count_within(M, q_d[j].data_ptr(), rs["at"], held[j].data_ptr(), init=True, slot=j, stream=streams[j].cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host_counts(held[0]), counts_of(d, rs["at"]))
        np.testing.assert_array_equal(host_counts(held[1]), counts_of(d, rs["at"])[::-1])
    finally:
        ix.close()


def test_an_empty_shard_bad_arguments_launch_nothing_and_the_other_entry_points_reject_the_count_flags():
    k = 3
    rng = np.random.default_rng(5)
    R = rng.random((2000, k), dtype=np.float32)
    Q = rng.random((12, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R)
    empty = pkg.KnnIndex(k, R[:0], n_local=0)
    try:
        np.testing.assert_array_equal(count(empty, Q, 0.5, counts=dev_counts(12, fill=5), init=False), np.full(12, 5, np.uint32))
        np.testing.assert_array_equal(count(empty, Q, 0.5, counts=dev_counts(12, fill=5), init=True), np.zeros(12, np.uint32))
        L = pkg.lib()
        vp = ctypes.c_void_p
        q_d = torch.from_numpy(Q.reshape(-1)).to(dev())
        c = dev_counts(12, fill=123)
        keys = torch.full((12 * 8,), 123, dtype=torch.int64, device=dev())
        for args in ((0, 12, -1.0, 1), (0, 12, float("nan"), 1), (8, 12, 1.0, 1), (-1, 12, 1.0, 1), (0, 0, 1.0, 1), (0, 12, 1.0, 2),
                     (0, 12, 1.0, 4), (0, 12, 1.0, 8), (0, 12, 1.0, 64)):
            slot, m, r2, flags = args
            assert pkg.count_within_c()(ix._h, slot, m, vp(q_d.data_ptr()), r2, vp(c.data_ptr()), None, flags) == -1, args
        assert pkg.count_within_c()(ix._h, 0, 12, None, 1.0, vp(c.data_ptr()), None, 1) == -1
        assert pkg.count_within_c()(ix._h, 0, 12, vp(q_d.data_ptr()), 1.0, None, None, 1) == -1
        with pytest.raises(pkg.KnnError, match="knn_index_count_within"):
            ix.count_within(12, q_d.data_ptr(), -2.0, c.data_ptr(), init=True)
        with pytest.raises(pkg.KnnError, match="knn_index_count_within_host"):
            ix.count_within_host(Q, float("nan"))
        # the existing entry points keep rejecting bits 16 and 32
        for flags in (pkg.QUERY_COUNT_GRID, pkg.QUERY_COUNT_CELLS, 1 | pkg.QUERY_COUNT_GRID):
            assert L.knn_index_query(ix._h, 0, 12, vp(q_d.data_ptr()), vp(keys.data_ptr()), None, None, flags) == -1
            assert L.knn_index_query_topk(ix._h, 0, 12, 8, vp(q_d.data_ptr()), vp(keys.data_ptr()), None, None, flags) == -1
            assert L.knn_index_query_topk_within(ix._h, 0, 12, 8, vp(q_d.data_ptr()), 1.0, vp(keys.data_ptr()), None, None, flags) == -1
        torch.cuda.synchronize()
        assert (host_counts(c) == 123).all() and (keys.cpu().numpy() == 123).all()   # nothing was launched
    finally:
        ix.close()
        empty.close()
