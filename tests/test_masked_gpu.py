"""knn_index_query_topk_masked and knn_index_count_within_masked (include/knn_mi355x.h 2g; DESIGN §4.6 "Over a subset of the rows")
on the GPU.  The rows and queries are tests/test_count_exact_gpu.py's batch (several slices, a clamped second wave of queries, a
NaN, a +INF and a 3e38 row, one row held twice).  The oracle alone decides every expectation: tests/topk_oracle.py over the
admitted rows with their ORIGINAL numbers, clipped at the radius by tests/within_helper.py, and tests/count_oracle.py over the
admitted rows.  Bar: bit-exact keys and counts."""
import functools

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count, dev, dev_counts, host_counts
from tests.count_oracle import counts as oracle_counts
from tests.count_oracle import radii
from tests.shards_helper import Shards
from tests.test_count_exact_gpu import M, N, TIE_A, TIE_B, batch
from tests.topk_oracle import KEY_INIT, keys_index, topk_keys, v0_dist2
from tests.within_helper import clip, dev_keys, host_keys, within

pytestmark = pytest.mark.gpu
INF = float("inf")
BASE = 9


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in ("path", "cells"):
        pkg.set_option(name, 0)


def words_of(n, sel):
    """The uint32 mask words over n rows that admit the rows `sel` (indices or a boolean array)."""
    bits = np.zeros(pkg.mask_words(n) * 32, dtype=bool)
    bits[:n][sel] = True
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def words_to_bits(words, n):
    return np.unpackbits(np.asarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


def dev_words(words):
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32).copy()).to(dev())


def masked(ix, Q, K, r2, words, keys=None, init=True, slot=0):
    """One call of query_topk_masked: keys [m][K] (numpy uint64) after it; the indices it unpacked are those of the keys."""
    Qf = np.array(Q, dtype=np.float32).reshape(-1)            # (a copy: the shared batch is read-only)
    m = Qf.size // ix.k
    q_d, w_d = torch.from_numpy(Qf).to(dev()), dev_words(words)
    if keys is None:
        keys = dev_keys(m, K, fill=np.full((m, K), 0x1234567887654321, dtype=np.uint64) if init else np.full((m, K), KEY_INIT))
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    ix.query_topk_masked(m, K, q_d.data_ptr(), w_d.data_ptr(), keys.data_ptr(), max_dist2=r2, init_keys=init,
                         indices_dev=ind.data_ptr(), slot=slot)
    torch.cuda.synchronize()
    got = host_keys(keys, m, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return got


def mcount(ix, Q, r2, words, counts=None, init=True, slot=0):
    """One call of count_within_masked: the counts [m] (numpy uint32) after it."""
    Qf = np.array(Q, dtype=np.float32).reshape(-1)            # (a copy: the shared batch is read-only)
    m = Qf.size // ix.k
    q_d, w_d = torch.from_numpy(Qf).to(dev()), dev_words(words)
    if counts is None:
        counts = dev_counts(m, fill=0xDEADBEEF if init else 0)
    torch.cuda.synchronize()
    ix.count_within_masked(m, q_d.data_ptr(), r2, w_d.data_ptr(), counts.data_ptr(), init=init, slot=slot)
    torch.cuda.synchronize()
    return host_counts(counts)


def want_keys(Q, R, k, K, sel, r2, base=BASE, gids=None):
    """The oracle over the admitted rows sel (ascending local rows), numbered base + row or gids[row]."""
    sel = np.asarray(sel, dtype=np.int64)
    g = (sel + base) if gids is None else np.asarray(gids)[sel]
    return clip(topk_keys(Q, R[sel], k, K, gids=g), r2)


def want_counts(Q, R, k, sel, r2):
    return oracle_counts(Q, R[np.asarray(sel, dtype=np.int64)], k, r2)


def check(ix, Q, R, k, K, sel, r2, base=BASE, msg=""):
    n = R.shape[0]
    w = words_of(n, sel)
    sel = np.flatnonzero(words_to_bits(w, n))
    np.testing.assert_array_equal(masked(ix, Q, K, r2, w), want_keys(Q, R, k, K, sel, r2, base), err_msg=f"keys {msg} r2={r2}")
    assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()
    np.testing.assert_array_equal(mcount(ix, Q, r2, w), want_counts(Q, R, k, sel, r2), err_msg=f"counts {msg} r2={r2}")
    assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()


@functools.lru_cache(maxsize=None)
def data(k):
    R, Q = batch(k, 9000 + k)
    d = v0_dist2(Q, R, k)
    assert d[3, TIE_A] == d[3, TIE_B] and np.isnan(d[:, 5]).all() and np.isinf(d[:, 6]).all() and np.isinf(d[:, 7]).all()
    for a in (R, Q, d):
        a.setflags(write=False)
    return R, Q, d


@pytest.mark.parametrize("k", [1, 16, 17, 32, 33, 128, 129])
def test_every_compiled_form_with_a_random_half_mask(k):
    R, Q, d = data(k)
    half = np.random.default_rng(100 + k).random(N) < 0.5
    half[[5, 6, 7]] = True                       # the rows without a finite distance stay admitted: they must not get in
    finite = dict(radii(d[:, half]))["at"]       # a distance some admitted row holds: zero counts and counts of 1 .. 63 among the queries
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for K in (1, 17, 64):
            for r2 in (INF, finite):
                check(ix, Q, R, k, K, half, r2, msg=f"k={k} K={K}")
    finally:
        ix.close()


def shapes(rng):
    tail = words_of(N, [])
    tail[-1] = np.uint32(~((1 << (N % 32)) - 1) & 0xFFFFFFFF)      # only bits at and beyond N
    every_second_word = np.repeat(np.arange(pkg.mask_words(N)) % 2 == 0, 32)[:N]
    return [
        ("all_zeros", []),
        ("row_0", [0]),
        ("row_last", [N - 1]),
        ("only_nan_inf_overflow_rows", [5, 6, 7]),
        ("every_second_word_zero", every_second_word),
        ("density_1_64", rng.random(N) < 1 / 64),
        ("range_of_100_in_one_granule", np.arange(1100, 1200)),    # T < slices: most slices are empty
        ("range_across_a_granule_boundary", np.arange(2000, 2100)),
        ("fewer_than_K", [17, 1023, 1024, 2047, 3148]),
        ("only_the_last_granule", np.arange(3080, N)),                # three empty granules in front: the walk jumps over them
        ("first_and_last_granule", [3, 700, 3100, 3148]),            # ... and over the two in between
        ("half", rng.random(N) < 0.5),
    ], tail


@pytest.mark.parametrize("k", [3, 17])
def test_mask_shapes(k):
    R, Q, d = data(k)
    K = 8
    finite = dict(radii(d))["large"]             # more than 64 rows of the whole set within it for some query
    all_rows, tail = shapes(np.random.default_rng(200 + k))
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for r2 in (INF, finite):
            # all ones: the unmasked calls' keys and counts bit for bit (and the oracle's)
            ones = np.full(pkg.mask_words(N), 0xFFFFFFFF, dtype=np.uint32)
            got = masked(ix, Q, K, r2, ones)
            np.testing.assert_array_equal(got, within(ix, Q.copy(), K, r2))       # (copies: the shared batch is read-only)
            np.testing.assert_array_equal(got, want_keys(Q, R, k, K, np.arange(N), r2))
            np.testing.assert_array_equal(mcount(ix, Q, r2, ones), count(ix, Q.copy(), r2))
            np.testing.assert_array_equal(mcount(ix, Q, r2, ones), want_counts(Q, R, k, np.arange(N), r2))
            for name, sel in all_rows:
                check(ix, Q, R, k, K, sel, r2, msg=f"{name} k={k}")
            # padding where the oracle says so, whatever the call found in the buffers
            assert (masked(ix, Q, K, r2, words_of(N, [])) == KEY_INIT).all() and (mcount(ix, Q, r2, words_of(N, [])) == 0).all()
            assert (masked(ix, Q, K, r2, words_of(N, [5, 6, 7])) == KEY_INIT).all()
            assert (masked(ix, Q, K, INF, words_of(N, [17, 1023, 1024]))[:, 3:] == KEY_INIT).all()
            # the tail word's bits at and beyond N change nothing
            half = words_of(N, all_rows[-1][1])
            np.testing.assert_array_equal(masked(ix, Q, K, r2, half | tail), masked(ix, Q, K, r2, half))
            np.testing.assert_array_equal(mcount(ix, Q, r2, half | tail), mcount(ix, Q, r2, half))
            assert (masked(ix, Q, K, r2, tail) == KEY_INIT).all() and (mcount(ix, Q, r2, tail) == 0).all()
    finally:
        ix.close()
    # shards of exactly one granule and of one granule and a row
    rng = np.random.default_rng(300 + k)
    for n in (1024, 1025):
        ix = pkg.KnnIndex(k, R[:n], base_index=BASE)
        try:
            for name, sel in (("ones", np.arange(n)), ("half", rng.random(n) < 0.5), ("last", [n - 1]), ("none", [])):
                for r2 in (INF, finite):
                    check(ix, Q, R[:n], k, K, sel, r2, msg=f"n={n} {name} k={k}")
        finally:
            ix.close()


def test_ties_go_to_the_admitted_copy_and_to_the_lower_number_first():
    k, K = 17, 8
    R, Q, d = data(k)
    tie = float(d[3, TIE_A])
    below = float(np.nextafter(np.float32(tie), np.float32(0)))
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for sel in ([TIE_A], [TIE_B], [TIE_A, TIE_B], [TIE_A, TIE_B, 40, 2500]):
            for r2 in (tie, below, INF):
                check(ix, Q, R, k, K, sel, r2, msg=f"tie {sel}")
        at = masked(ix, Q, K, tie, words_of(N, [TIE_A, TIE_B]))[3]
        assert list(keys_index(at[:2])) == [BASE + TIE_A, BASE + TIE_B] and at[0] >> np.uint64(32) == at[1] >> np.uint64(32)
        assert (at[2:] == KEY_INIT).all()
        assert (masked(ix, Q, K, below, words_of(N, [TIE_A, TIE_B]))[3] == KEY_INIT).all()
        assert keys_index(masked(ix, Q, K, tie, words_of(N, [TIE_B]))[3])[0] == BASE + TIE_B
        assert mcount(ix, Q, tie, words_of(N, [TIE_A, TIE_B]))[3] == 2 and mcount(ix, Q, below, words_of(N, [TIE_A, TIE_B]))[3] == 0
    finally:
        ix.close()


def fold_of(held, lists):
    return np.sort(np.concatenate([held, lists], axis=1), axis=1)[:, :held.shape[1]]


def test_two_shards_with_their_own_masks_fold_and_an_init_call_writes():
    k, K, cut = 17, 8, 1500
    R, Q, d = data(k)
    sel = np.random.default_rng(400).random(N) < 0.3
    rows = np.flatnonzero(sel)
    finite = dict(radii(d[:, sel]))["at"]
    a, b = pkg.KnnIndex(k, R[:cut]), pkg.KnnIndex(k, R[cut:], base_index=cut)
    wa, wb = words_of(cut, sel[:cut]), words_of(N - cut, sel[cut:])
    try:
        for r2 in (INF, finite):
            want = want_keys(Q, R, k, K, rows, r2, base=0)
            keys = dev_keys(M, K, fill=np.full((M, K), 0xDEADBEEFDEADBEEF, dtype=np.uint64))      # poisoned: the init call writes
            masked(a, Q, K, r2, wa, keys=keys, init=True)
            np.testing.assert_array_equal(masked(b, Q, K, r2, wb, keys=keys, init=False), want, err_msg=f"fold r2={r2}")
            c = dev_counts(M, fill=0xDEADBEEF)
            mcount(a, Q, r2, wa, counts=c, init=True)
            np.testing.assert_array_equal(mcount(b, Q, r2, wb, counts=c, init=False), want_counts(Q, R, k, rows, r2))
            held = np.arange(M, dtype=np.uint32) * 1000
            np.testing.assert_array_equal(mcount(b, Q, r2, wb, counts=dev_counts(M, fill=held), init=False),
                                          held + want_counts(Q, R[cut:], k, np.flatnonzero(sel[cut:]), r2))
        # a fold into caller keys that lie beyond the radius: they are the caller's and are not clipped
        far = np.float32(finite) * np.float32(4.0)
        held = np.full((M, K), KEY_INIT, dtype=np.uint64)
        held[:, 0] = (np.uint64(far.view(np.uint32)) << np.uint64(32)) | np.uint64(77)
        held[:, 1] = (np.uint64(np.float32(far * 2).view(np.uint32)) << np.uint64(32)) | np.uint64(3)
        got = masked(b, Q, K, finite, wb, keys=dev_keys(M, K, fill=held), init=False)
        mine = want_keys(Q, R[cut:], k, K, np.flatnonzero(sel[cut:]), finite, base=cut)
        np.testing.assert_array_equal(got, fold_of(held, mine))
        assert (got == held[0, 0]).any() and (got == held[0, 1]).any()
    finally:
        a.close()
        b.close()


def test_a_cell_range_shard_pair_folds_with_gids_under_masks_in_local_row_order():
    rng = np.random.default_rng(500)
    k, n, m, K = 16, (1 << 19) + 5, 24, 8
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    sel = rng.random(n) < 1 / 16
    rows = np.flatnonzero(sel)
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=False)
    try:
        gids = [g.cpu().numpy().astype(np.int64) for g in sh.gids]
        local = [words_of(g.size, sel[g]) for g in gids]             # bit i = local row i = global row gids[i]
        d = v0_dist2(Q, R[rows], k)
        finite = float(np.sort(d, axis=1)[:, 3].min())                # some lists are cut short at it, some are not
        for r2 in (INF, finite):
            want = want_keys(Q, R, k, K, rows, r2, base=0)
            keys, c = dev_keys(m, K), dev_counts(m, fill=0xDEADBEEF)
            for r, ix in enumerate(sh.idx):
                got = masked(ix, Q, K, r2, local[r], keys=keys, init=(r == 0))
                assert ix.last_stats() == [1, 0, 0, 0]
                cnt = mcount(ix, Q, r2, local[r], counts=c, init=(r == 0))
            np.testing.assert_array_equal(got, want, err_msg=f"r2={r2}")
            np.testing.assert_array_equal(cnt, want_counts(Q, R, k, rows, r2))
        assert int(keys_index(want_keys(Q, R, k, K, rows, INF, base=0)).max()) >= sh.rows[0].shape[0]   # numbers no local row of rank 0 has
        # each rank alone: its own admitted rows under their gids
        for r, ix in enumerate(sh.idx):
            mine = np.flatnonzero(sel[gids[r]])
            np.testing.assert_array_equal(masked(ix, Q, K, INF, local[r]), want_keys(Q, R[gids[r]], k, K, mine, INF, gids=gids[r]))
    finally:
        sh.close()


def test_an_index_with_a_grid_and_one_with_a_cell_sorted_layout_answer_too():
    m, K = 70, 8
    for k, n, opt in ((3, 16384, None), (16, 1 << 17, "cells")):
        rng = np.random.default_rng(600 + k)
        R = rng.random((n, k), dtype=np.float32)
        Q = rng.random((m, k), dtype=np.float32)
        sel = np.flatnonzero(rng.random(n) < 1 / 16)
        finite = float(np.sort(v0_dist2(Q, R[sel], k), axis=1)[:, 3].min())
        try:
            if opt:
                pkg.set_option(opt, 1)
            ix = pkg.KnnIndex(k, R, base_index=BASE)
            try:
                # the index is what the case says: its 1-NN call takes the grid / the cell-pruned scan
                keys1 = torch.empty(m, dtype=torch.int64, device=dev())
                ix.query_keys(m, torch.from_numpy(Q.reshape(-1)).to(dev()).data_ptr(), keys1.data_ptr(), init_keys=True)
                torch.cuda.synchronize()
                assert ix.last_stats()[0] == (4 if opt else 3), ix.last_stats()
                for r2 in (INF, finite):
                    check(ix, Q, R, k, K, sel, r2, msg=f"k={k} n={n}")
                # one contiguous range far into the shard: many slices cut it row by row, the empty granules around it are jumped
                start = (2 * n // 3) | 1
                check(ix, Q, R, k, K, np.arange(start, start + n // 16), INF, msg=f"range k={k} n={n}")
            finally:
                ix.close()
        finally:
            if opt:
                pkg.set_option(opt, 0)


def test_one_query_a_non_finite_query_slot_reuse_and_the_host_call():
    k, K = 16, 8
    R, Q, d = data(k)
    rng = np.random.default_rng(700)
    sel, other = np.flatnonzero(rng.random(N) < 0.4), np.flatnonzero(rng.random(N) < 0.1)
    w, w2 = words_of(N, sel), words_of(N, other)
    finite = dict(radii(d[:, sel]))["at"]
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for r2 in (INF, finite):
            for j in (0, 33, M - 1):      # m = 1
                np.testing.assert_array_equal(masked(ix, Q[j:j + 1], K, r2, w), want_keys(Q[j:j + 1], R, k, K, sel, r2))
                np.testing.assert_array_equal(mcount(ix, Q[j:j + 1], r2, w), want_counts(Q[j:j + 1], R, k, sel, r2))
            Qbad = Q.copy()
            Qbad[4, 2] = np.nan
            Qbad[9, 0] = np.inf
            Qbad[66, k - 1] = -np.inf
            got, cnt = masked(ix, Qbad, K, r2, w), mcount(ix, Qbad, r2, w)
            np.testing.assert_array_equal(got, want_keys(Qbad, R, k, K, sel, r2))
            np.testing.assert_array_equal(cnt, want_counts(Qbad, R, k, sel, r2))
            assert (got[[4, 9, 66]] == KEY_INIT).all() and (cnt[[4, 9, 66]] == 0).all()
            # one slot: masked, unmasked top-K, masked count, masked with another mask
            for slot in (0, 5):
                np.testing.assert_array_equal(masked(ix, Q, K, r2, w, slot=slot), want_keys(Q, R, k, K, sel, r2))
                np.testing.assert_array_equal(within(ix, Q.copy(), 64, r2, slot=slot), want_keys(Q, R, k, 64, np.arange(N), r2))
                np.testing.assert_array_equal(mcount(ix, Q, r2, w, slot=slot), want_counts(Q, R, k, sel, r2))
                np.testing.assert_array_equal(masked(ix, Q, K, r2, w2, slot=slot), want_keys(Q, R, k, K, other, r2))
                np.testing.assert_array_equal(masked(ix, Q, 64, r2, w2, slot=slot), want_keys(Q, R, k, 64, other, r2))
            # the host call
            want = want_keys(Q, R, k, K, sel, r2)
            ind, d2, cnt = ix.query_topk_masked_host(Q, K, w, max_dist2=r2)
            np.testing.assert_array_equal(ind, keys_index(want))
            np.testing.assert_array_equal(d2.view(np.uint32), (want >> np.uint64(32)).astype(np.uint32))
            np.testing.assert_array_equal(cnt, (want != KEY_INIT).sum(axis=1))
        assert cnt.min() < K <= cnt.max()
        with pytest.raises(ValueError):
            ix.query_topk_masked_host(Q, K, w[:-1])
        with pytest.raises(pkg.KnnError, match="knn_index_query_topk_masked: unknown flag"):
            q_d = torch.from_numpy(Q.reshape(-1).copy()).to(dev())
            ix.query_topk_masked(M, K, q_d.data_ptr(), dev_words(w).data_ptr(), dev_keys(M, K).data_ptr(), flags=64)
    finally:
        ix.close()
    empty = pkg.KnnIndex(k, R[:0], n_local=0)
    try:
        none = np.zeros(1, dtype=np.uint32)       # (a mask of no words: the pointer is only checked)
        held = np.sort(np.random.default_rng(1).integers(1, 1 << 62, size=(M, K), dtype=np.uint64), axis=1)
        np.testing.assert_array_equal(masked(empty, Q, K, INF, none, keys=dev_keys(M, K, fill=held), init=False), held)
        assert (masked(empty, Q, K, INF, none) == KEY_INIT).all()
        np.testing.assert_array_equal(mcount(empty, Q, 0.5, none, counts=dev_counts(M, fill=5), init=False), np.full(M, 5, np.uint32))
        assert (mcount(empty, Q, 0.5, none) == 0).all()
        assert empty.last_stats() == [1, 0, 0, 0]
    finally:
        empty.close()


def test_mask_set_rows_against_a_numpy_bitmap():
    n = 5000
    rng = np.random.default_rng(800)
    ids = np.concatenate([rng.integers(0, n, size=3000), [0, n - 1, n - 1, 31, 32, 32, 32], [n, n + 1, 8191, 1 << 20, 0xFFFFFFFF]])
    clear = np.concatenate([ids[:1000], rng.integers(0, n, size=500), [n, 0xFFFFFFFF, n - 1]])
    nw = pkg.mask_words(n)

    def apply(mask_d, rows, value):
        r_d = torch.from_numpy(np.asarray(rows, dtype=np.uint32).view(np.int32).copy()).to(dev())
        pkg.mask_set_rows(n, r_d.data_ptr(), r_d.numel(), value, mask_d.data_ptr())
        torch.cuda.synchronize()
        return mask_d.cpu().numpy().view(np.uint32)

    # an allow-list: zeros, then set (duplicates and ids outside 0 .. n - 1 among them); then clear some
    mask_d = torch.zeros(nw + 2, dtype=torch.int32, device=dev())      # two words of margin: nothing may be written there
    bits = np.zeros(n, dtype=bool)
    bits[ids[ids < n]] = True
    got = apply(mask_d, ids, 1)
    np.testing.assert_array_equal(got[:nw], words_of(n, bits))
    assert (got[nw:] == 0).all()
    bits[clear[clear < n]] = False
    got = apply(mask_d, clear, 0)
    np.testing.assert_array_equal(got[:nw], words_of(n, bits))
    assert (got[nw:] == 0).all()
    # tombstones: ones, then clear
    mask_d = torch.full((nw + 2,), -1, dtype=torch.int32, device=dev())
    got = apply(mask_d, clear, 0)
    alive = np.ones(n, dtype=bool)
    alive[clear[clear < n]] = False
    np.testing.assert_array_equal(words_to_bits(got[:nw], n), alive)
    assert (got[nw:] == 0xFFFFFFFF).all()
    # nothing listed: nothing launched, nothing changed
    pkg.mask_set_rows(n, None, 0, 1, mask_d.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(mask_d.cpu().numpy().view(np.uint32), got)
    # the mask it made drives a query
    k, K = 3, 8
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((20, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        check(ix, Q, R, k, K, alive, INF, msg="tombstones")
        np.testing.assert_array_equal(masked(ix, Q, K, INF, got[:nw]), want_keys(Q, R, k, K, np.flatnonzero(alive), INF))
    finally:
        ix.close()
