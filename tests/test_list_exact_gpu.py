"""knn_index_list_within on the exact list scan (the default way) on the GPU against tests/list_oracle.py, on the batch of
tests/test_count_exact_gpu.py: every compiled form of knn_exact_list_kernel<KC>, several slices, a second (clamped) wave of
queries, rows that are NaN, +INF and 3e38, a boundary tie across slices, every radius; overflowing segments between guard words,
the init flag against appending, a fold of two shards, m = 1, non-finite queries, two slots, the host call, and list, count and
top-K calls in every order on one slot."""
import ctypes
import itertools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count, dev, dev_counts, host_counts
from tests.count_oracle import counts_of, radii
from tests.list_helper import PAD, assert_lists, check_list, dev_u64, host_u64, list_call, segments
from tests.list_oracle import holds_every_kind, kinds, lengths, lists_of, offsets_of
from tests.test_count_exact_gpu import KS, M, N, TIE_A, TIE_B, batch
from tests.topk_oracle import topk_keys, v0_dist2
from tests.within_helper import plain

pytestmark = pytest.mark.gpu
BASE = 9


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


def all_radii(d):
    tie = float(d[3, TIE_A])
    return radii(d) + [("tie", tie), ("tie_below", float(np.nextafter(np.float32(tie), np.float32(0))))]


@pytest.mark.parametrize("k", KS)
def test_every_compiled_form_at_every_radius(k):
    R, Q = batch(k, 7000 + k)
    d = v0_dist2(Q, R, k)
    assert d[3, TIE_A] == d[3, TIE_B] and np.isnan(d[:, 5]).all() and np.isinf(d[:, 6]).all() and np.isinf(d[:, 7]).all()
    want = {name: lists_of(d, r2, base=BASE) for name, r2 in all_radii(d)}
    assert holds_every_kind(want.values()) and all(kinds(want[n])[:2] == (True, True) for n in ("at", "below"))
    assert kinds(want["large"])[2]
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for name, r2 in all_radii(d):
            np.testing.assert_array_equal(lengths(want[name]), counts_of(d, r2))
            check_list(ix, Q, r2, want[name], msg=f"k={k} {name} r2={r2}")
            assert ix.last_stats()[:3] == [1, 0, 0], ix.last_stats()
        # both copies of the tied row enter and leave together
        both = {np.uint64(BASE + TIE_A), np.uint64(BASE + TIE_B)}
        low = np.uint64(0xFFFFFFFF)
        assert both <= set((want["tie"][3] & low).tolist()) and not (both & set((want["tie_below"][3] & low).tolist()))
        assert (lengths(want["inf"]) == N - 3).all()
        # a flag on an index without the structure changes nothing
        check_list(ix, Q, radii(d)[0][1], want["at"], grid=True, cells=True)
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


@pytest.mark.parametrize("k", [3, 17, 129])
def test_overflowing_segments_store_nothing_outside_them(k):
    """Segments one entry short wherever the count is above zero, and segments of no room at all, with guard words in front of the
    first segment and behind the last: fill still ends as the count, every stored key is a hit of its query, stored once, and no
    guard word changes.  (Guards between the segments: test_guard_words_between_the_segments_ends.)"""
    R, Q = batch(k, 7300 + k)
    d = v0_dist2(Q, R, k)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for name in ("at", "large", "inf"):
            r2 = dict(radii(d))[name]
            want = lists_of(d, r2, base=BASE)
            cnt = lengths(want)
            assert kinds(want)[1] or name == "inf"
            for rooms in (np.where(cnt > 0, cnt - 1, 0), np.zeros(M, dtype=np.uint32)):
                # a guard word in front of the first segment and two behind the last
                exact = np.zeros(M + 1, dtype=np.uint64)
                exact[0] = 1
                exact[1:] = 1 + np.cumsum(rooms.astype(np.uint64))
                buf = np.full(int(exact[-1]) + 2, PAD, dtype=np.uint64)
                fill, keys = list_call(ix, Q, r2, exact, keys=dev_u64(buf))
                np.testing.assert_array_equal(fill, cnt, err_msg=f"{name}: fill is the count whether or not a hit was stored")
                assert keys[0] == PAD and keys[int(exact[-1])] == PAD and keys[-1] == PAD, "a guard word changed"
                for j in range(M):
                    got = keys[int(exact[j]):int(exact[j + 1])]
                    assert got.size == rooms[j]
                    assert np.isin(got, want[j]).all() and np.unique(got).size == got.size, (name, j)
    finally:
        ix.close()


def test_guard_words_between_the_segments_ends():
    """Segment j ends where segment j + 1 begins, so a guard word BETWEEN two segments' ends is a segment of its own: every odd query
    is a non-finite one whose segment of one entry must keep its bytes while both neighbours overflow."""
    k = 17
    R, Q = batch(k, 7350)
    Q2 = np.repeat(Q, 2, axis=0)
    Q2[1::2, 0] = np.nan
    d = v0_dist2(Q, R, k)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        r2 = dict(radii(d))["large"]
        want = lists_of(d, r2, base=BASE)
        cnt = lengths(want)
        rooms = np.ones(2 * M, dtype=np.uint64)
        rooms[0::2] = np.where(cnt > 0, cnt - 1, 0)
        exact = np.zeros(2 * M + 1, dtype=np.uint64)
        exact[0] = 1
        exact[1:] = 1 + np.cumsum(rooms)
        buf = np.full(int(exact[-1]) + 1, PAD, dtype=np.uint64)
        fill, keys = list_call(ix, Q2, r2, exact, keys=dev_u64(buf))
        np.testing.assert_array_equal(fill[0::2], cnt)
        assert (fill[1::2] == 0).all()
        assert keys[0] == PAD and keys[-1] == PAD
        for j in range(M):
            assert keys[int(exact[2 * j + 1])] == PAD, f"the guard behind segment {j} changed"
            got = keys[int(exact[2 * j]):int(exact[2 * j + 1])]
            assert np.isin(got, want[j]).all() and np.unique(got).size == got.size
        assert (cnt > 64).any() and (cnt == 0).any()
    finally:
        ix.close()


def test_init_zeroes_the_cursor_appending_continues_and_two_shards_fold_to_the_whole_set():
    k = 17
    R, Q = batch(k, 7100)
    d = v0_dist2(Q, R, k)
    rs = dict(radii(d))
    whole = pkg.KnnIndex(k, R)
    a, b = pkg.KnnIndex(k, R[:1500]), pkg.KnnIndex(k, R[1500:], base_index=1500)
    try:
        seen = []
        for name in ("at", "large", "inf", "zero"):
            r2, want = rs[name], lists_of(d, rs[name])
            seen.append(want)
            cnt = lengths(want)
            # appending twice behind an init call: three copies of every list, fill three times the count
            off = offsets_of(3 * cnt.astype(np.uint64))
            fill_d = dev_counts(M, fill=0xDEADBEEF)
            keys_d = dev_u64(np.full(max(int(off[-1]), 1), PAD))
            for rnd, init in enumerate((True, False, False)):
                fill, keys = list_call(whole, Q, r2, off, fill=fill_d, keys=keys_d, init=init)
                np.testing.assert_array_equal(fill, (rnd + 1) * cnt, err_msg=name)
            assert_lists(segments(off, fill, keys), [np.sort(np.tile(w, 3)) for w in want], name)
            # a cursor that already stands somewhere: the hits go behind it, what is in front keeps its bytes
            held = (np.arange(M, dtype=np.uint32) % 3)
            off = offsets_of(cnt.astype(np.uint64) + held)
            fill, keys = list_call(whole, Q, r2, off, fill=dev_counts(M, fill=held), init=False)
            np.testing.assert_array_equal(fill, held + cnt)
            for j in range(M):
                assert (keys[int(off[j]):int(off[j]) + int(held[j])] == PAD).all()
                np.testing.assert_array_equal(np.sort(keys[int(off[j]) + int(held[j]):int(off[j + 1])]), want[j])
            # two index-range shards: the first starts the cursor, the second appends
            off = offsets_of(cnt)
            fill_d = dev_counts(M, fill=0xDEADBEEF)
            keys_d = dev_u64(np.full(max(int(off[-1]), 1), PAD))
            list_call(a, Q, r2, off, fill=fill_d, keys=keys_d, init=True)
            fill, keys = list_call(b, Q, r2, off, fill=fill_d, keys=keys_d, init=False)
            np.testing.assert_array_equal(fill, cnt, err_msg=f"two shards, {name}")
            assert_lists(segments(off, fill, keys), want, f"two shards, {name}")
        assert holds_every_kind(seen)
    finally:
        whole.close()
        a.close()
        b.close()


def test_one_query_non_finite_queries_two_slots_and_the_host_call():
    k = 16
    R, Q = batch(k, 7200)
    d = v0_dist2(Q, R, k)
    rs = dict(radii(d))
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        assert holds_every_kind([lists_of(d, rs[n], base=BASE) for n in ("at", "large")])
        for name in ("at", "large", "inf"):
            r2 = rs[name]
            want = lists_of(d, r2, base=BASE)
            for j in (0, 33, M - 1):   # m = 1
                check_list(ix, Q[j:j + 1], r2, want[j:j + 1], msg=f"m=1 {name} {j}")
            Qbad = Q.copy()
            Qbad[4, 2] = np.nan
            Qbad[9, 0] = np.inf
            Qbad[66, k - 1] = -np.inf
            wbad = list(want)
            for j in (4, 9, 66):
                wbad[j] = np.zeros(0, dtype=np.uint64)
            check_list(ix, Qbad, r2, wbad, msg=f"non-finite queries, {name}")
        # the host call: count, offsets, list, sort — the lists come back sorted
        for name in ("at", "large", "zero", "inf"):
            want = lists_of(d, rs[name], base=BASE)
            off, ind, d2 = ix.list_within_host(Q, rs[name])
            np.testing.assert_array_equal(off, offsets_of(lengths(want)).astype(np.int64), err_msg=name)
            flat = np.concatenate(want) if int(off[-1]) else np.zeros(0, dtype=np.uint64)
            np.testing.assert_array_equal(ind.view(np.uint32), (flat & np.uint64(0xFFFFFFFF)).astype(np.uint32), err_msg=name)
            np.testing.assert_array_equal(d2.view(np.uint32), (flat >> np.uint64(32)).astype(np.uint32), err_msg=name)
        off, ind, d2 = ix.list_within_host(Q, -0.0)
        assert off[-1] == 0 and ind.size == 0 and d2.size == 0 and (lengths(lists_of(d, 0.0)) == 0).all()
        with pytest.raises(pkg.KnnError, match="knn_index_list_within_host"):
            ix.list_within_host(Q, float("nan"))
        # two slots in flight on two streams
        want = lists_of(d, rs["at"], base=BASE)
        streams = [torch.cuda.Stream(device=dev()) for _ in range(2)]
        orders = [np.arange(M), np.arange(M)[::-1]]
        q_d = [torch.from_numpy(np.ascontiguousarray(Q[o]).reshape(-1)).to(dev()) for o in orders]
        offs = [offsets_of(lengths(want)[o]) for o in orders]
        off_d = [dev_u64(o) for o in offs]
        fill_d = [dev_counts(M, fill=7) for _ in range(2)]
        keys_d = [dev_u64(np.full(int(o[-1]), PAD)) for o in offs]
        torch.cuda.synchronize()
        for j in range(2):
            ix.list_within(M, q_d[j].data_ptr(), rs["at"], off_d[j].data_ptr(), fill_d[j].data_ptr(), keys_d[j].data_ptr(), init=True,
                           slot=j, stream=streams[j].cuda_stream)
        torch.cuda.synchronize()
        for j in range(2):
            assert_lists(segments(offs[j], host_counts(fill_d[j]), host_u64(keys_d[j])), [want[i] for i in orders[j]], f"slot {j}")
    finally:
        ix.close()


def test_the_device_sequence_count_offsets_list_sort():
    """The four calls as a caller chains them on one stream, no host step in between: the sorted segments are the oracle's lists."""
    k = 33
    R, Q = batch(k, 7400)
    d = v0_dist2(Q, R, k)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        r2 = dict(radii(d))["large"]
        want = lists_of(d, r2, base=BASE)
        assert kinds(want) == (True, True, True)
        total = int(lengths(want).sum())
        q_d = torch.from_numpy(Q.reshape(-1)).to(dev())
        c_d, fill_d = dev_counts(M, fill=1), dev_counts(M, fill=2)
        off_d = dev_u64(np.full(M + 1, 3))
        keys_d = dev_u64(np.full(total, PAD))
        torch.cuda.synchronize()
        ix.count_within(M, q_d.data_ptr(), r2, c_d.data_ptr(), init=True)
        pkg.counts_to_offsets(c_d.data_ptr(), M, off_d.data_ptr())
        ix.list_within(M, q_d.data_ptr(), r2, off_d.data_ptr(), fill_d.data_ptr(), keys_d.data_ptr(), init=True)
        pkg.keys_sort_segments(M, off_d.data_ptr(), fill_d.data_ptr(), keys_d.data_ptr())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host_u64(off_d), offsets_of(lengths(want)))
        np.testing.assert_array_equal(host_counts(fill_d), lengths(want))
        np.testing.assert_array_equal(host_u64(keys_d), np.concatenate(want))
    finally:
        ix.close()


def test_an_empty_shard_and_bad_arguments_launch_nothing():
    k = 3
    rng = np.random.default_rng(5)
    R = rng.random((2000, k), dtype=np.float32)
    Q = rng.random((12, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R)
    empty = pkg.KnnIndex(k, R[:0], n_local=0)
    try:
        off = offsets_of(np.full(12, 4))
        fill, keys = list_call(empty, Q, 0.5, off, fill=dev_counts(12, fill=5), init=False)
        assert (fill == 5).all() and (keys == PAD).all()
        fill, keys = list_call(empty, Q, 0.5, off, fill=dev_counts(12, fill=5), init=True)
        assert (fill == 0).all() and (keys == PAD).all()
        vp = ctypes.c_void_p
        q_d = torch.from_numpy(Q.reshape(-1)).to(dev())
        off_d, f_d, k_d = dev_u64(off), dev_counts(12, fill=123), dev_u64(np.full(48, PAD))
        for slot, m, r2, flags in ((0, 12, -1.0, 1), (0, 12, float("nan"), 1), (8, 12, 1.0, 1), (-1, 12, 1.0, 1), (0, 0, 1.0, 1),
                                   (0, 12, 1.0, 2), (0, 12, 1.0, 4), (0, 12, 1.0, 8), (0, 12, 1.0, 64)):
            assert pkg.list_within_c()(ix._h, slot, m, vp(q_d.data_ptr()), r2, vp(off_d.data_ptr()), vp(f_d.data_ptr()),
                                       vp(k_d.data_ptr()), None, flags) == -1, (slot, m, r2, flags)
        with pytest.raises(pkg.KnnError, match="knn_index_list_within"):
            ix.list_within(12, q_d.data_ptr(), -2.0, off_d.data_ptr(), f_d.data_ptr(), k_d.data_ptr(), init=True)
        torch.cuda.synchronize()
        assert (host_counts(f_d) == 123).all() and (host_u64(k_d) == PAD).all()   # nothing was launched
    finally:
        ix.close()
        empty.close()


def test_count_top_k_and_list_calls_in_every_order_on_one_slot():
    k, K, slot = 16, 8, 5
    R, Q = batch(k, 7500)
    d = v0_dist2(Q, R, k)
    r2 = dict(radii(d))["at"]
    want = lists_of(d, r2, base=BASE)
    want_keys = topk_keys(Q, R, k, K, base=BASE)
    ix = pkg.KnnIndex(k, R, base_index=BASE)

    def counted():
        np.testing.assert_array_equal(count(ix, Q, r2, slot=slot), lengths(want))

    def top_k():
        np.testing.assert_array_equal(plain(ix, Q, K, slot=slot), want_keys)

    def listed():
        check_list(ix, Q, r2, want, slot=slot)

    try:
        for order in itertools.permutations((counted, top_k, listed)):
            for call in order:
                call()
    finally:
        ix.close()
