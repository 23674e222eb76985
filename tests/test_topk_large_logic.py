"""Top-K beyond 64 (knn_index_query_topk_large, include/knn_mi355x.h 2f) without a GPU: the argument rules of the three entry points,
the exported names, the call's plan (knn_debug_topk_large_plan) and the radix select on the host through the pick kernel's own
lines (knn_debug_radix_kth, csrc/knn_radix_pick.h) against np.partition."""
import ctypes
import os
import re

import numpy as np
import pytest

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
INT_MAX = 2**31 - 1
ALL = 0x7F7FFFFFFFFFFFFF
vp = ctypes.c_void_p


def test_the_new_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    for name in ("knn_index_query_topk_large", "knn_keys_topk_merge_large", "knn_index_query_topk_large_host",
                 "knn_debug_topk_large_plan", "knn_debug_radix_kth"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    assert re.search(r"#define KNN_TOPK_LARGE_MAX 4096\b", header) and pkg.TOPK_LARGE_MAX == 4096
    assert "2f. Top-K beyond 64" in header


def test_the_large_call_argument_errors_need_no_gpu():
    """Every rule has its own text and the index is looked at last, so the rules show with a null index: nothing behind them is
    reached (the pointers here are never read)."""
    L = pkg.lib()
    q, k = vp(0x1000), vp(0x2000)
    init = pkg.QUERY_INIT_KEYS

    def rc(slot=0, m=7, K=100, queries=q, r2=1.0, keys=k, flags=init):
        return pkg.query_topk_large_c()(None, slot, m, K, queries, r2, keys, None, None, flags), L.knn_last_error().decode()

    who = "knn_index_query_topk_large: "
    assert rc() == (EINVAL, who + "null index")
    assert rc(flags=0) == (EINVAL, who + "null index")
    texts = set()
    for K in (0, -1, 4097, 1 << 20):
        code, text = rc(K=K)
        assert code == EINVAL and text == who + "K outside 1 .. 4096", (K, text)
    texts.add(text)
    for K in (1, 64, 65, 4096):
        assert rc(K=K)[1].endswith("null index")
    for m in (0, -3):
        code, text = rc(m=m)
        assert code == EINVAL and text == who + "m < 1"
    texts.add(text)
    code, text = rc(m=INT_MAX // 4096 + 1, K=4096)
    assert code == EINVAL and text == who + "m * K above INT_MAX"
    texts.add(text)
    assert rc(m=INT_MAX // 4096, K=4096)[1].endswith("null index")
    for slot in (8, -1):
        code, text = rc(slot=slot)
        assert code == EINVAL and text == who + "slot outside 0 .. 7"
    texts.add(text)
    for bad in (-1.0, float("nan"), -float("inf")):
        code, text = rc(r2=bad)
        assert code == EINVAL and text == who + "max_dist2 must be >= 0 and not NaN", (bad, text)
    texts.add(text)
    for r2 in (0.0, -0.0, float("inf")):
        assert rc(r2=r2)[1].endswith("null index")
    # KNN_QUERY_INIT_KEYS alone: PARTIAL, TOPK_GRID, TOPK_FRAMES, both COUNT_* flags and a sixth bit are refused
    for flags in (pkg.QUERY_TOPK_PARTIAL, pkg.QUERY_TOPK_GRID, pkg.QUERY_TOPK_FRAMES, pkg.QUERY_COUNT_GRID, pkg.QUERY_COUNT_CELLS, 64,
                  1 << 31, init | pkg.QUERY_TOPK_PARTIAL, init | 64):
        code, text = rc(flags=flags)
        assert code == EINVAL and text.startswith(who + "unknown flag"), (flags, text)
    texts.add(text)
    for kw in (dict(queries=None), dict(keys=None)):
        code, text = rc(**kw)
        assert code == EINVAL and text == who + "null queries or keys"
    texts.add(text)
    assert len(texts) == 7


def test_the_merge_and_host_call_argument_errors_need_no_gpu():
    L = pkg.lib()
    a, b = vp(0x1000), vp(0x2000)

    def merge(m=5, K=100, a_=a, b_=b):
        return pkg.keys_topk_merge_large_c()(0, m, K, a_, b_, None), L.knn_last_error().decode()

    who = "knn_keys_topk_merge_large: "
    for K in (0, 4097):
        assert merge(K=K) == (EINVAL, who + "K outside 1 .. 4096")
    assert merge(m=0) == (EINVAL, who + "m < 1")
    assert merge(a_=None) == (EINVAL, who + "null list") and merge(b_=None) == (EINVAL, who + "null list")

    Q = np.zeros((4, 3), dtype=np.float32)
    ind = np.zeros((4, 100), dtype=np.int32)

    def host(m=4, K=100, queries=Q.ctypes.data, r2=1.0, out=ind.ctypes.data):
        return (pkg.query_topk_large_host_c()(None, m, K, vp(queries) if queries else None, r2, vp(out) if out else None, None, None),
                L.knn_last_error().decode())

    who = "knn_index_query_topk_large_host: "
    assert host() == (EINVAL, who + "null index")
    assert host(K=0) == (EINVAL, who + "K outside 1 .. 4096") and host(K=4097) == (EINVAL, who + "K outside 1 .. 4096")
    assert host(m=0) == (EINVAL, who + "m < 1")
    assert host(m=INT_MAX // 4096 + 1, K=4096) == (EINVAL, who + "m * K above INT_MAX")
    for bad in (-1.0, float("nan")):
        assert host(r2=bad) == (EINVAL, who + "max_dist2 must be >= 0 and not NaN")
    assert host(queries=None) == (EINVAL, who + "null queries or indices")
    assert host(out=None) == (EINVAL, who + "null queries or indices")


def plan(k=3, m=1024, K=100, rows=1 << 20, num_cu=256, init=1):
    return pkg.debug_topk_large_plan(k=k, m=m, K=K, rows=rows, num_cu=num_cu, init=init)


def test_the_plan_is_monotone_chunks_at_65536_and_fits_the_lds():
    p = plan()
    assert p["chunks"] == 1 and p["dist_passes"] == 4 and p["index_passes"] == 4
    assert 0 < p["lds_bytes"] <= 160 * 1024
    assert p["lds_bytes"] <= 64 * 1024                      # static LDS
    assert p["launches_ties"] - p["launches_clean"] == 2 * p["index_passes"]
    assert 1 <= p["slices"] <= 65535
    # monotone in m and K: a folding call holds the lists, an init call only the select's state
    for init in (0, 1):
        last = 0
        for m in (1, 63, 64, 65, 1000, 65536, 65537, 200000):
            b = plan(m=m, init=init)["scratch_bytes"]
            assert b >= last, (m, init)
            last = b
        last = 0
        for K in (1, 64, 65, 1000, 4096):
            b = plan(K=K, init=init)["scratch_bytes"]
            assert b >= last, (K, init)
            last = b
        assert plan(K=4096, init=0)["scratch_bytes"] > plan(K=65, init=0)["scratch_bytes"]
    assert plan(init=0)["scratch_bytes"] - plan(init=1)["scratch_bytes"] == 1024 * 100 * 8
    # the per-query histograms alone: 256 bins of 4 bytes
    assert plan(m=64)["scratch_bytes"] >= 64 * 256 * 4
    # a second chunk at m = 65537, with one more sequence of launches
    assert plan(m=65536, K=65)["chunks"] == 1 and plan(m=65537, K=65)["chunks"] == 2
    assert plan(m=65537, K=65)["launches_clean"] == 2 * plan(m=65536, K=65)["launches_clean"]
    # one slice per 1024 rows at the least, and never more slices than rows allow
    assert plan(rows=1)["slices"] == 1 and plan(rows=3149, m=70)["slices"] >= 3
    # bad inputs
    L = pkg.lib()
    for kw in (dict(K=0), dict(K=4097), dict(m=0), dict(m=INT_MAX // 4096 + 1, K=4096), dict(rows=0), dict(num_cu=0), dict(k=0),
               dict(init=2)):
        with pytest.raises(pkg.KnnError):
            plan(**kw)
        assert L.knn_last_error().decode().startswith("knn_debug_topk_large_plan")
    assert plan(m=INT_MAX // 4096, K=4096)["chunks"] == (INT_MAX // 4096 + 65535) // 65536


def pack(dist_words, indices):
    return (np.asarray(dist_words, dtype=np.uint64) << np.uint64(32)) | np.asarray(indices, dtype=np.uint64)


def check_kth(keys, K):
    """T of distinct keys: exactly min(K, n) keys are <= T, T is not below the K-th smallest; n < K: the all-pass value."""
    keys = np.asarray(keys, dtype=np.uint64)
    T, passes = pkg.debug_radix_kth(keys, K)
    assert 1 <= passes <= 8
    if keys.size < K:
        assert T == ALL and passes == 1
        return T, passes
    kth = int(np.partition(keys, K - 1)[K - 1])
    assert T >= kth and int((keys <= np.uint64(T)).sum()) == K, (hex(T), hex(kth), K)
    if keys.size > K:
        assert T < int(np.partition(keys, K)[K])
    if passes == 8:
        assert T == kth
    # the digits the passes fixed are the K-th key's
    shift = 64 - 8 * passes
    assert T >> shift == kth >> shift
    return T, passes


def test_radix_select_on_the_host_against_partition():
    rng = np.random.default_rng(4711)
    # random keys: finite non-negative float words, distinct indices
    for n, K in ((5000, 1), (5000, 65), (5000, 4096), (300, 300), (300, 299), (77, 64), (1, 1)):
        d = rng.random(n, dtype=np.float32) * np.float32(10.0)
        keys = pack(d.view(np.uint32), rng.permutation(n) + 9)
        check_kth(keys, K)
    # random 62-bit keys (every digit place is exercised)
    for n, K in ((4000, 1000), (4000, 1), (4000, 4000)):
        keys = np.unique(rng.integers(0, ALL, size=n, dtype=np.uint64))
        check_kth(keys, min(K, keys.size))
    # n < K: every candidate passes, decided by the first pass
    for n, K in ((0, 1), (10, 11), (64, 65), (100, 4096)):
        T, passes = check_kth(pack(np.arange(n) + 0x3F800000, np.arange(n)), K)
        assert T == ALL and passes == 1
    # K = n and K = 1
    keys = pack(rng.integers(0x30000000, 0x40000000, size=500), np.arange(500))
    check_kth(keys, 500)
    check_kth(keys, 1)


def test_the_index_passes_run_only_for_a_cut_inside_a_distance_class():
    rng = np.random.default_rng(4712)
    # one shared distance word, distinct indices: the cut falls inside the class, the index word's passes must run
    n = 3000
    keys = pack(np.full(n, 0x3F800000), rng.permutation(1 << 20)[:n])
    for K in (1, 65, 500, n - 1):
        T, passes = check_kth(keys, K)
        assert passes > 4, (K, passes)
        assert T >> 32 == 0x3F800000
    # ... down to the last digit when neighbours differ in the lowest byte only
    keys = pack(np.full(600, 0x40000000), np.arange(600) + (7 << 24))
    T, passes = check_kth(keys, 300)
    assert passes == 8 and T == int(np.sort(keys)[299])
    # K = n: the whole class passes, no index pass
    assert check_kth(keys, 600)[1] <= 4
    # all distance words distinct: the index passes are gated off
    words = rng.permutation(np.arange(0x3F000000, 0x3F000000 + 50000))[:4000]
    keys = pack(words, rng.integers(0, 1 << 32, size=4000, dtype=np.uint64))
    for K in (1, 65, 1000, 4000):
        assert check_kth(keys, K)[1] <= 4
    # a class of equal distances that does NOT hold the cut changes nothing
    keys2 = np.concatenate([keys, pack(np.full(100, int(np.sort(words)[10])), np.arange(100) + 5)])
    srt = np.sort(np.unique(keys2))
    K = 500
    assert srt[K - 1] >> np.uint64(32) != srt[K] >> np.uint64(32)
    assert check_kth(srt, K)[1] <= 4
    # bad arguments
    for K in (0, 4097):
        with pytest.raises(pkg.KnnError):
            pkg.debug_radix_kth(keys, K)
