"""Radius-bounded top-K on the exact top-K scan (knn_index_query_topk_within on an index without layouts) on the GPU against the
numpy restatement of v0 (tests/topk_oracle.py), clipped at the radius: a row beyond the radius never enters a lane's list."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index, topk_keys
from tests.within_helper import KS, clip, dev_keys, lengths, plain, radii, within

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


def spread_queries(rng, m, k, reach=1.5):
    """Queries inside the rows' unit box and, one after the other, further outside it (up to `reach` along the first axis): their nearest distances span a range, so one
    radius leaves some lists full, some short and some empty."""
    Q = rng.random((m, k), dtype=np.float32)
    Q[:, 0] += np.linspace(0.0, reach, m, dtype=np.float32)
    return Q


@pytest.mark.parametrize("k,n,m,reach", [(16, 5000, 12, 1.5), (130, 2000, 5, 4.0)], ids=["k16", "k130_any_k_form"])
def test_every_radius_on_the_exact_scan(k, n, m, reach):
    rng = np.random.default_rng(900 + k)
    R = rng.random((n, k), dtype=np.float32)
    Q = spread_queries(rng, m, k, reach)
    want64 = topk_keys(Q, R, k, 64, base=7)
    ix = pkg.KnnIndex(k, R, base_index=7)
    try:
        for K in KS:
            want = want64[:, :K]
            for name, r2 in radii(want):
                got = within(ix, Q, K, r2)
                assert ix.last_stats()[0] == 1, ix.last_stats()
                np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"k={k} K={K} {name} r2={r2}")
            np.testing.assert_array_equal(within(ix, Q, K, float("inf")), plain(ix, Q, K))
        # a fold: the held keys — another shard's plain top-K, keys beyond the radius among them — stay
        K = 8
        want = want64[:, :K]
        r2 = radii(want)[0][1]
        held = topk_keys(Q, rng.random((300, k), dtype=np.float32), k, K, base=7 + n)
        assert (keys_dist2(held) > np.float32(r2)).any()
        got = within(ix, Q, K, r2, init=False, keys=dev_keys(m, K, fill=held))
        np.testing.assert_array_equal(got, np.sort(np.concatenate([held, clip(want, r2)], axis=1), axis=1)[:, :K])
    finally:
        ix.close()


def test_the_host_call_returns_indices_distances_and_counts():
    rng = np.random.default_rng(916)
    k, n, m, K = 16, 5000, 12, 17
    R = rng.random((n, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    want = topk_keys(Q, R, k, K, base=3)
    ix = pkg.KnnIndex(k, R, base_index=3)
    try:
        for name, r2 in radii(want):
            idx, d2, counts = ix.query_topk_within_host(Q, K, r2)
            exp = clip(want, r2)
            np.testing.assert_array_equal(idx, keys_index(exp), err_msg=name)
            np.testing.assert_array_equal(d2.view(np.uint32), keys_dist2(exp).view(np.uint32), err_msg=name)
            np.testing.assert_array_equal(counts, lengths(want, r2), err_msg=name)
            assert np.isinf(d2[exp == KEY_INIT]).all() and (idx[exp == KEY_INIT] == 0).all()
        idx0, d20 = ix.query_topk_host(Q, K)
        idx1, d21, counts = ix.query_topk_within_host(Q, K, float("inf"))
        np.testing.assert_array_equal(idx1, idx0)
        np.testing.assert_array_equal(d21.view(np.uint32), d20.view(np.uint32))
        assert (counts == K).all()
        L = pkg.lib()   # counts_host may be NULL
        i2, e2 = np.empty((m, K), np.int32), np.empty((m, K), np.float32)
        assert L.knn_index_query_topk_within_host(ix._h, m, K, Q.ctypes.data_as(ctypes.c_void_p), 0.5,
                                                  i2.ctypes.data_as(ctypes.c_void_p), e2.ctypes.data_as(ctypes.c_void_p), None) == 0
        np.testing.assert_array_equal(i2, keys_index(clip(want, 0.5)))
    finally:
        ix.close()
