"""The one call front of the one-way top-K forms (knn_api.cpp: topk_check, topk_one_way) and the staged rounds of the host calls
(topk_host_run, lists_host_round) on the GPU: what knn_index_query_topk_large, _masked, _large_masked and the exact branch of
knn_index_self_topk leave behind besides their answer — the timing bracket (knn_index_timing_read) and knn_index_last_stats, both as
the commit before the front reported them —, that a call folding into padding, an init call and the indices array agree, that
radius -0.0 is radius 0.0, what an empty shard does, and that every host call returns exactly what the device sequence it wraps
returns.  No result oracle here: tests/test_topk_large_gpu.py, test_masked_gpu.py, test_masked_lists_gpu.py, test_self_gpu.py,
test_list_exact_gpu.py and test_each_exact_gpu.py check the values."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import dev_counts, host_counts
from tests.each_helper import dev_f32
from tests.list_helper import PAD, dev_u64, host_u64

pytestmark = pytest.mark.gpu
# k = 3, n = 2000: no multiple of 64, and below the 16384 rows from which a grid index is built — no layout, every call on way 1
K_DIM, N, M, FIRST = 3, 2000, 20, 7
K_OF = {"query_topk_large": 100, "query_topk_masked": 5, "query_topk_large_masked": 100, "self_topk": 5}
ENTRIES = tuple(K_OF)
# (bracketed launches of one timed init call, last_stats()[2]) of every entry at these shapes: what commit cff69b3, the one before
# the front, reports (the rows hold no two equal distances to a query: the large forms' index passes stay off)
PARENT = {"query_topk_large": (1, 0), "query_topk_masked": (1, 0), "query_topk_large_masked": (1, 0), "self_topk": (1, 0)}
KEY_INIT = np.uint64(pkg.KEY_INIT)
R2 = 0.007      # a few rows within it of a row of 2000 in the unit cube


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


@functools.lru_cache(maxsize=None)
def rows():
    R = np.random.default_rng(9107).random((N, K_DIM), dtype=np.float32)
    R.setflags(write=False)
    return R


def queries():
    """The window's rows as the queries of the three entries that take queries: the self entry asks about the same rows."""
    return rows()[FIRST:FIRST + M].copy()


def issue(ix, entry, keys, init, r2=float("inf"), indices=None, n=N):
    """One call of `entry` about the window into `keys` (device uint64 [M][K])."""
    K = K_OF[entry]
    q, mask = dev_f32(queries()), dev_counts(max(pkg.mask_words(n), 1), fill=0xFFFFFFFF)
    ind = None if indices is None else indices.data_ptr()
    torch.cuda.synchronize()
    if entry == "query_topk_large":
        ix.query_topk_large(M, K, q.data_ptr(), keys.data_ptr(), max_dist2=r2, init_keys=init, indices_dev=ind)
    elif entry == "query_topk_masked":
        ix.query_topk_masked(M, K, q.data_ptr(), mask.data_ptr(), keys.data_ptr(), max_dist2=r2, init_keys=init, indices_dev=ind)
    elif entry == "query_topk_large_masked":
        ix.query_topk_large_masked(M, K, q.data_ptr(), mask.data_ptr(), keys.data_ptr(), max_dist2=r2, init_keys=init, indices_dev=ind)
    else:
        assert entry == "self_topk"
        ix.self_topk(FIRST, M, K, keys.data_ptr(), max_dist2=r2, init_keys=init, indices_dev=ind)
    torch.cuda.synchronize()


def held(entry, value):
    return dev_u64(np.full(M * K_OF[entry], value, dtype=np.uint64))


@pytest.fixture(scope="module")
def index():
    ix = pkg.KnnIndex(K_DIM, rows())
    yield ix
    ix.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_init_call_brackets_and_reports_what_it_did_before_the_front(index, entry):
    launches_want, s2_want = PARENT[entry]
    index.timing(1)
    try:
        for _ in range(2):
            issue(index, entry, held(entry, PAD), True)
            launches, total_ms = index.timing_read()
            stats = index.last_stats()
            print(f"{entry}: {launches} bracketed launches, {total_ms:.4f} ms, last_stats {stats}")
            assert launches == launches_want, (entry, launches)
            assert math.isfinite(total_ms) and total_ms > 0, (entry, total_ms)
            assert stats == [1, 0, s2_want, 0], (entry, stats)
    finally:
        index.timing(0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_fold_into_padding_is_the_init_call_and_the_indices_are_the_keys_low_words(index, entry):
    K = K_OF[entry]
    written, folded = held(entry, PAD), held(entry, KEY_INIT)
    ind = torch.full((M * K,), -7, dtype=torch.int32, device=written.device)
    issue(index, entry, written, True, indices=ind)
    assert index.last_stats()[0] == 1
    issue(index, entry, folded, False)
    want = host_u64(written).reshape(M, K)
    assert (want < KEY_INIT).all() and (want[:, 1:] > want[:, :-1]).all()      # 2000 rows: no padding, ascending
    np.testing.assert_array_equal(host_u64(folded).reshape(M, K), want)
    np.testing.assert_array_equal(ind.cpu().numpy().view(np.uint32), (host_u64(written) & np.uint64(0xFFFFFFFF)).astype(np.uint32))


@pytest.mark.parametrize("entry", ENTRIES)
def test_radius_minus_zero_is_radius_zero(index, entry):
    plus, minus = held(entry, PAD), held(entry, PAD)
    issue(index, entry, plus, True, r2=0.0)
    issue(index, entry, minus, True, r2=-0.0)
    got = host_u64(plus).reshape(M, K_OF[entry])
    np.testing.assert_array_equal(host_u64(minus).reshape(got.shape), got)
    # a query that is a row of the shard finds that row at distance 0 and nothing else; a self call's row is no candidate
    assert ((got < KEY_INIT).sum(axis=1) == (0 if entry == "self_topk" else 1)).all()


def test_an_empty_shard_fills_under_init_alone_and_fails_the_self_call_on_its_range():
    ix = pkg.KnnIndex(K_DIM, np.zeros((0, K_DIM), np.float32))
    try:
        for entry in ENTRIES[:3]:
            keys = held(entry, PAD)
            issue(ix, entry, keys, False, n=0)
            assert (host_u64(keys) == PAD).all() and ix.last_stats() == [1, 0, 0, 0], entry
            issue(ix, entry, keys, True, n=0)
            assert (host_u64(keys) == KEY_INIT).all() and ix.last_stats() == [1, 0, 0, 0], entry
        keys = held("self_topk", PAD)
        for init in (False, True):
            with pytest.raises(pkg.KnnError, match="knn_index_self_topk: row_first \\+ rows above the shard's rows"):
                ix.self_topk(0, 1, 5, keys.data_ptr(), init_keys=init)
        torch.cuda.synchronize()
        assert (host_u64(keys) == PAD).all()
        # the list host calls: offsets of zeroes and arrays with one element of room
        q, word = np.zeros((M, K_DIM), np.float32), np.zeros(0, np.uint32)      # (a mask over no rows: no words)
        for off, ind, d2 in (ix.list_within_host(q, R2), ix.list_within_masked_host(q, R2, word)):
            assert off.shape == (M + 1,) and not off.any() and ind.size == 0 and d2.size == 0
        for off, ind, d2 in (ix.self_list_within_host(R2), ix.self_list_within_routed_host(R2)):
            assert off.shape == (1,) and not off.any() and ind.size == 0 and d2.size == 0
        offsets = np.full(1, -1, dtype=np.int64)
        ind_p, d2_p = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
        assert pkg.self_list_within_host_c()(ix._h, R2, offsets.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ind_p), ctypes.byref(d2_p)) == 0
        assert offsets[0] == 0 and bool(ind_p) and bool(d2_p)
        free = ctypes.CDLL(None).free
        free.argtypes = [ctypes.c_void_p]
        free(ind_p)
        free(d2_p)
    finally:
        ix.close()


def unpacked(keys):
    """(indices int32, dist2 float32) of packed keys, as the host calls unpack them."""
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32), (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("entry", ENTRIES[:3])
def test_a_topk_host_call_returns_what_its_device_call_returns(index, entry):
    K = K_OF[entry]
    keys = held(entry, PAD)
    issue(index, entry, keys, True, r2=R2)
    want = host_u64(keys).reshape(M, K)
    mask = np.full(pkg.mask_words(N), 0xFFFFFFFF, dtype=np.uint32)
    if entry == "query_topk_large":
        ind, d2, counts = index.query_topk_large_host(queries(), K, max_dist2=R2)
    elif entry == "query_topk_masked":
        ind, d2, counts = index.query_topk_masked_host(queries(), K, mask, max_dist2=R2)
    else:
        ind, d2, counts = index.query_topk_large_masked_host(queries(), K, mask, max_dist2=R2)
    assert index.last_stats()[0] == 1
    want_ind, want_d2 = unpacked(want)
    np.testing.assert_array_equal(np.asarray(ind).reshape(M, K), want_ind)
    np.testing.assert_array_equal(np.asarray(d2).reshape(M, K).view(np.uint32), want_d2.view(np.uint32))
    np.testing.assert_array_equal(np.asarray(counts), (want < KEY_INIT).sum(axis=1))
    assert int(np.asarray(counts).min()) >= 1 and (np.asarray(counts) < K).any()      # the radius leaves real keys and padding


def device_lists(segments, count, lst):
    """count -> knn_counts_to_offsets -> list -> knn_keys_sort_segments from the device entries: (offsets uint64, keys uint64)."""
    counts, fill = dev_counts(segments, fill=0xDEADBEEF), dev_counts(segments, fill=0xDEADBEEF)
    off = dev_u64(np.zeros(segments + 1, dtype=np.uint64))
    torch.cuda.synchronize()
    count(counts.data_ptr())
    pkg.counts_to_offsets(counts.data_ptr(), segments, off.data_ptr())
    torch.cuda.synchronize()
    offsets = host_u64(off)
    keys = dev_u64(np.full(max(int(offsets[segments]), 1), PAD))
    torch.cuda.synchronize()
    lst(off.data_ptr(), fill.data_ptr(), keys.data_ptr())
    pkg.keys_sort_segments(segments, off.data_ptr(), fill.data_ptr(), keys.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_counts(fill), host_counts(counts))
    return offsets, host_u64(keys)[:int(offsets[segments])]


@pytest.mark.parametrize("form", ["list_within", "list_within_masked", "self_list_within", "self_list_within_routed"])
def test_a_list_host_call_returns_what_its_device_sequence_returns(index, form):
    q, mask_d = dev_f32(queries()), dev_counts(pkg.mask_words(N), fill=0xFFFFFFFF)
    mask = np.full(pkg.mask_words(N), 0xFFFFFFFF, dtype=np.uint32)
    radii = (np.float32(R2) * (np.float32(0.5) + np.float32(0.5) * np.random.default_rng(9108).random(N, dtype=np.float32))).astype(np.float32)
    radii_d = dev_f32(radii)
    if form == "list_within":
        got = index.list_within_host(queries(), R2)
        want = device_lists(M, lambda c: index.count_within(M, q.data_ptr(), R2, c, init=True),
                            lambda *lists: index.list_within(M, q.data_ptr(), R2, *lists, init=True))
    elif form == "list_within_masked":
        got = index.list_within_masked_host(queries(), R2, mask)
        want = device_lists(M, lambda c: index.count_within_masked(M, q.data_ptr(), R2, mask_d.data_ptr(), c, init=True),
                            lambda *lists: index.list_within_masked(M, q.data_ptr(), R2, mask_d.data_ptr(), *lists, init=True))
    elif form == "self_list_within":
        got = index.self_list_within_host(R2)
        want = device_lists(N, lambda c: index.self_count_within(0, N, R2, c, init=True),
                            lambda *lists: index.self_list_within(0, N, R2, *lists, init=True))
    else:
        got = index.self_list_within_routed_host(R2, max_dist2=radii)
        want = device_lists(N, lambda c: index.self_count_within_routed(0, N, c, cap=R2, max_dist2_dev=radii_d.data_ptr(), init=True),
                            lambda *lists: index.self_list_within_routed(0, N, *lists, cap=R2, max_dist2_dev=radii_d.data_ptr(), init=True))
    offsets, ind, d2 = got
    want_ind, want_d2 = unpacked(want[1])
    np.testing.assert_array_equal(offsets.astype(np.uint64), want[0])
    np.testing.assert_array_equal(ind, want_ind)
    np.testing.assert_array_equal(d2.view(np.uint32), want_d2.view(np.uint32))
    segments = len(want[0]) - 1
    assert segments <= int(want[0][segments]) <= 40 * segments      # a few hits per row, not none and not the shard
