"""Top-K queries (include/knn_mi355x.h section 2c) without a GPU: the numpy oracle the GPU tests compare against, and the
C-ABI's symbols and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_host_logic import ROOT, _built_lib
from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index, topk_keys

TOPK_SYMBOLS = ("knn_index_query_topk", "knn_keys_topk_merge", "knn_index_query_topk_host")


def _synthetic(rng, k, m, n):
    """Rows with ties, duplicates, NaN, +-inf and overflowing coordinates."""
    R = rng.integers(0, 4, (n, k)).astype(np.float32)   # coarse lattice: many equal distances
    R[5] = R[3]                                            # duplicates
    R[7] = R[3]
    R[11, 0] = np.nan
    R[13, min(1, k - 1)] = np.inf
    R[17, 0] = -np.inf
    R[19] = 3e38                                           # (q - r)^2 overflows to +inf
    R[23, :] = 1e19                                        # squares to 1e38: the sum overflows from k = 4 on
    Q = rng.integers(0, 4, (m, k)).astype(np.float32)
    Q[0] = R[3]
    return Q, R


def test_column_zero_is_v0_on_the_ta_samples(oracle):
    for k, m, n, Q, R in oracle.ta_samples():
        take = min(m, 48)
        Qs = Q.reshape(m, k)[:take]
        want = oracle.v0_keys(k, Qs, R, base=0)
        got = topk_keys(Qs, R, k, 8)
        np.testing.assert_array_equal(got[:, 0], want, err_msg=f"k={k} n={n}")


@pytest.mark.parametrize("k", [1, 3, 16])
def test_column_zero_is_v0_with_ties_nan_inf_and_overflow(oracle, k):
    rng = np.random.default_rng(k)
    Q, R = _synthetic(rng, k, 40, 300)
    for base in (0, 1000):
        got = topk_keys(Q, R, k, 17, base=base)
        np.testing.assert_array_equal(got[:, 0], oracle.v0_keys(k, Q, R, base=base))
    # the overflowing and non-finite rows are never candidates
    idx = keys_index(got)[keys_dist2(got) < np.inf] - 1000
    assert not set(idx.tolist()) & {11, 13, 17, 19}


def test_order_is_distance_then_lowest_index():
    """The uint64 order of the keys equals an independent (float64 distance, index) sort of all finite candidates."""
    rng = np.random.default_rng(3)
    k, K = 4, 33
    Q, R = _synthetic(rng, k, 25, 200)
    got = topk_keys(Q, R, k, K, base=50)
    for j in range(Q.shape[0]):
        d = np.zeros(R.shape[0], dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(k):
                diff = np.float32(Q[j, t]) - R[:, t]
                d = d + diff * diff
        fin = np.nonzero(np.isfinite(d))[0]
        order = fin[np.lexsort((fin, d[fin].astype(np.float64)))][:K]
        np.testing.assert_array_equal(keys_index(got[j]), order.astype(np.int32) + 50)
        np.testing.assert_array_equal(keys_dist2(got[j]), d[order])


def test_padding_when_fewer_rows_than_k():
    rng = np.random.default_rng(4)
    Q = rng.random((6, 3), dtype=np.float32)
    R = rng.random((5, 3), dtype=np.float32)
    R[2, 0] = np.nan                                       # 4 finite rows
    got = topk_keys(Q, R, 3, 8, base=9)
    assert (got[:, 4:] == KEY_INIT).all()
    assert (got[:, :4] < KEY_INIT).all()
    assert sorted(set(keys_index(got[:, :4]).ravel().tolist())) == [9, 10, 12, 13]
    assert np.all(got[:, 1:] >= got[:, :-1])


def test_header_declares_and_library_exports_the_topk_entry_points():
    path = _built_lib()
    import multicore_hw2_amd as pkg
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    L = ctypes.CDLL(path)
    for sym in TOPK_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pkg.EXPORTED_SYMBOLS, sym
        assert hasattr(L, sym), sym
    for name in ("query_topk", "query_topk_host"):
        assert callable(getattr(pkg.KnnIndex, name))
    assert callable(pkg.keys_topk_merge)


def test_topk_entry_points_reject_bad_arguments_without_a_gpu():
    _built_lib()
    import multicore_hw2_amd as pkg
    L = pkg.lib()
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    KNN_EINVAL = -1
    for K in (0, 65, -1):
        assert L.knn_keys_topk_merge(0, 4, K, p, p, None) == KNN_EINVAL
        assert b"1 <= K <= 64" in L.knn_last_error()
    assert L.knn_keys_topk_merge(0, 0, 4, p, p, None) == KNN_EINVAL           # m < 1
    assert L.knn_keys_topk_merge(0, 4, 4, None, p, None) == KNN_EINVAL
    assert L.knn_index_query_topk(None, 0, 4, 4, p, p, None, None, 0) == KNN_EINVAL
    assert L.knn_index_query_topk_host(None, 4, 4, p, p, None) == KNN_EINVAL


def test_kth_of_block_minima_threshold_keeps_every_true_top_k_row():
    """Host restatement of the filter top-K's threshold rule: blocks of disjoint rows, each row's score within
    eps of its distance (the filter's bound), thr(u) = u + 2 eps non-decreasing.  u_K = the K-th smallest per-block minimum
    that comes from a real row (padding blocks hold +INF); every true top-K row (brute force) scores <= thr(u_K).  Fewer than
    K blocks with a real row: no threshold (the fallback)."""
    rng = np.random.default_rng(9)
    for trial in range(200):
        n = int(rng.integers(1, 400))
        K = int(rng.integers(1, 65))
        nb = int(rng.integers(1, 80))
        d = rng.random(n) ** int(rng.integers(1, 4))
        d[rng.random(n) < 0.1] = d[0]                                  # ties
        eps = float(rng.random() * 0.05)
        score = d + rng.uniform(-eps, eps, n)
        block = rng.integers(0, nb, n)
        bmin = np.full(nb, np.inf)
        np.minimum.at(bmin, block, score)
        real = np.sort(bmin[np.isfinite(bmin)])
        true_top = np.lexsort((np.arange(n), d))[:K]
        if real.size < K:
            assert len(set(block.tolist())) < K                          # the device raises FALLBACK here
            continue
        thr = real[K - 1] + 2 * eps
        assert (score[true_top] <= thr).all(), (trial, n, K, nb)
