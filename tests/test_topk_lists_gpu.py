"""The top-K list kernels alone (knn_exact.hip: topk_wave_merge under knn_topk_select_kernel, knn_topk_clip_kernel and
knn_topk_select_cand_kernel) on the GPU, at every K from 1 to 64: knn_keys_topk_merge against a two-line numpy merge over lists
built to sit on the merge's edges, and the fold and the clip of knn_index_query_topk_within against the sorted union of the held
keys and the oracle's clipped list (tests/topk_oracle.py, tests/within_helper.clip).  Bar: bit-exact keys."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.test_within_exact_gpu import spread_queries
from tests.topk_oracle import KEY_INIT, keys_dist2, topk_keys
from tests.within_helper import clip, dev_keys, host_keys, plain, radii, within

pytestmark = pytest.mark.gpu
OPTIONS = ("path", "cells")
# knn_keys_topk_merge(a, b) runs knn_topk_select_kernel with the wave's running list (topk_wave_merge's `a`) = b and the list that
# is merged in (its `b`) = a, so the wave-uniform early exit `b0 >= alast` fires when a[0] >= b[K - 1]: "exits" and "misses the exit
# by one key" are built in THAT orientation; their mirrors (a holds the K smallest) take the full merge and replace all of b
KINDS = ("random_tails", "exits_b_holds_the_smallest", "misses_the_exit_by_one_key", "a_holds_the_smallest",
         "b0_one_key_below_a_last", "a_all_padding", "b_all_padding", "equal_distances_interleaved", "both_full", "both_all_padding")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _pack(d, idx):
    return (np.asarray(d, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(idx, dtype=np.uint64)


def one_pair(rng, K, kind):
    """Two sorted lists of K keys without a key in common (global numbers are distinct across shards), padded with KEY_INIT."""
    d = (rng.random(2 * K, dtype=np.float32) * np.float32(rng.choice([1e-3, 1.0, 1e4]))).astype(np.float32)
    idx = rng.permutation(2 * K).astype(np.uint64) * np.uint64(65537) + np.uint64(rng.integers(0, 60000))   # distinct
    la, lb = K, K                                       # real entries of a and of b
    if kind == "equal_distances_interleaved":           # one distance, the indices alternate between a and b
        keys = np.sort(_pack(np.full(2 * K, d[0]), idx))
        a, b = keys[0::2].copy(), keys[1::2].copy()
    elif kind in ("exits_b_holds_the_smallest", "misses_the_exit_by_one_key"):
        keys = np.sort(_pack(d, idx))                   # b is full and holds the K smallest: a[0] >= b[K - 1], the kernel's exit
        b, a = keys[:K].copy(), keys[K:].copy()
        la = int(rng.integers(1, K + 1))
        if kind == "misses_the_exit_by_one_key":        # a[0] one key below b[K - 1]: no exit, a[0] takes b's last place
            a[0] = b[K - 1] - np.uint64(1)
            assert a[0] not in b and (K == 1 or a[0] > b[K - 2])
    elif kind in ("a_holds_the_smallest", "b0_one_key_below_a_last"):
        keys = np.sort(_pack(d, idx))                   # the mirror: a holds the K smallest, the full merge replaces all of b
        a, b = keys[:K].copy(), keys[K:].copy()
        lb = int(rng.integers(1, K + 1))
        if kind == "b0_one_key_below_a_last":           # b[0] one key below a[K - 1]: the only key of b that stays
            b[0] = a[K - 1] - np.uint64(1)
            assert b[0] not in a and (K == 1 or b[0] > a[K - 2])
    else:
        pick = rng.permutation(2 * K)
        keys = _pack(d, idx)
        a, b = np.sort(keys[pick[:K]]), np.sort(keys[pick[K:]])
        if kind == "random_tails":
            la, lb = int(rng.integers(0, K + 1)), int(rng.integers(0, K + 1))
    if kind in ("a_all_padding", "both_all_padding"):
        la = 0
    if kind in ("b_all_padding", "both_all_padding"):
        lb = 0
    a[la:] = KEY_INIT
    b[lb:] = KEY_INIT
    return a, b


def pairs(rng, m, K):
    a, b = np.empty((m, K), dtype=np.uint64), np.empty((m, K), dtype=np.uint64)
    for j in range(m):
        a[j], b[j] = one_pair(rng, K, KINDS[j % len(KINDS)])
    real = np.concatenate([a, b], axis=1)
    for j in range(m):   # no key in common but the padding
        r = real[j][real[j] != KEY_INIT]
        assert np.unique(r).size == r.size
    assert (np.diff(a.astype(object), axis=1) >= 0).all() and (np.diff(b.astype(object), axis=1) >= 0).all()
    return a, b


def _merge(a, b):
    m, K = a.shape
    a_d, b_d = dev_keys(m, K, fill=a), dev_keys(m, K, fill=b)
    pkg.keys_topk_merge(a_d.data_ptr(), b_d.data_ptr(), m, K)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_keys(a_d, m, K), a)        # a is read only
    return host_keys(b_d, m, K)


def test_keys_topk_merge_at_every_k_on_lists_that_sit_on_its_edges():
    """m = 67 (every kind of pair at least six times) at every K, and one list pair of every kind alone at K = 64.  The kinds:
    KEY_INIT tails of every length from none to the whole list; a[0] >= b[K - 1] with real keys and a full b (the kernel's
    wave-uniform early exit: b is the running list) and a[0] one key below b[K - 1] (misses it by one key); their mirrors, where a
    holds the K smallest and replaces b; a or b or both all padding; one distance with the indices alternating between a and b."""
    rng = np.random.default_rng(6400)
    wrong = []
    for K in range(1, 65):
        a, b = pairs(rng, 67, K)
        real = (a[:, 0] != KEY_INIT) & (b[:, K - 1] != KEY_INIT)            # real keys in a, a full b
        exits = a[:, 0] >= b[:, K - 1]                                          # topk_wave_merge's b0 >= alast
        assert (exits & real).any() and (~exits).any() and (real & (b[:, K - 1] - a[:, 0] == 1)).any()
        assert (b[:, 0] >= a[:, K - 1]).any() and (a[:, K - 1] - b[:, 0] == 1).any()   # the mirrors
        tails = (a == KEY_INIT).sum(axis=1)
        assert (tails == 0).any() and (tails == K).any()
        got = _merge(a, b)
        want = np.sort(np.concatenate([a, b], 1), 1)[:, :K]
        if not (got == want).all():
            j = int(np.flatnonzero((got != want).any(axis=1))[0])
            wrong.append((K, j, KINDS[j % len(KINDS)]))
    assert not wrong, f"(K, first wrong query, its kind): {wrong}"
    for kind in KINDS:
        a, b = (x[None, :] for x in one_pair(rng, 64, kind))
        np.testing.assert_array_equal(_merge(a, b), np.sort(np.concatenate([a, b], 1), 1)[:, :64], err_msg=f"m=1 K=64 {kind}")


@pytest.mark.parametrize("name,opts,k,n,way", [("dense_filter", {"path": 2, "cells": 2}, 16, 66000, 2), ("exact_scan", {"path": 1}, 16, 2500, 1)],
                         ids=["dense_filter", "exact_scan"])
def test_the_fold_and_the_clip_at_every_k(name, opts, k, n, way):
    """Every K from 1 to 64 folds into held keys — another shard's plain top-K of the same queries, keys beyond the radius among
    them, which stay — within a radius and as a plain call.  On the dense filter that is knn_topk_select_cand_kernel and
    knn_topk_clip_kernel's merge branch, on the exact scan knn_topk_select_kernel over the scan's three slices."""
    rng = np.random.default_rng(6500 + n)
    m, base = 33, 17
    R = rng.random((n, k), dtype=np.float32)
    Q = spread_queries(rng, m, k, 0.6)
    want64 = topk_keys(Q, R, k, 64, base=base)
    held64 = topk_keys(Q, rng.random((300, k), dtype=np.float32), k, 64, base=base + n)   # a disjoint index range
    r2 = radii(want64[:, :8])[0][1]
    assert (keys_dist2(held64[:, 0]) > np.float32(r2)).any() and (keys_dist2(held64[:, 0]) <= np.float32(r2)).any()
    for o, v in opts.items():
        pkg.set_option(o, v)
    ix = pkg.KnnIndex(k, R, base_index=base)
    try:
        wrong = []
        for K in range(1, 65):
            want, held = want64[:, :K], held64[:, :K]
            for call, exp_list in (("within", clip(want, r2)), ("plain", want)):
                keys = dev_keys(m, K, fill=held)
                got = within(ix, Q, K, r2, init=False, keys=keys) if call == "within" else plain(ix, Q, K, init=False, keys=keys)
                st = ix.last_stats()
                assert st[0] == way and st[2] == 0, (name, K, call, st)
                exp = np.sort(np.concatenate([held, exp_list], axis=1), axis=1)[:, :K]
                if not (got == exp).all():
                    wrong.append((K, call, int(np.flatnonzero((got != exp).any(axis=1))[0])))
        assert not wrong, f"{name}: (K, call, first wrong query): {wrong}"
    finally:
        ix.close()
