"""knn_index_list_within_masked and knn_index_query_topk_large_masked (include/knn_mi355x.h 2h; DESIGN §4.6 "Lists and large K over
a subset of the rows") on the GPU.  The rows and queries are tests/test_count_exact_gpu.py's batch (several granules and slices, a
last mask word with bits beyond n, a clamped second wave of 6 queries, a NaN, a +INF and a 3e38 row, one row held twice).  The
oracle alone decides every expectation: tests/topk_oracle.v0_dist2 over the admitted rows with their ORIGINAL numbers, then
tests/list_oracle.lists_of and topk_keys (clipped at the radius) as tests/test_masked_gpu.want_keys does.  Every data-dependent
test first asserts, from the oracle alone (the prep_* functions: numpy, no GPU), that its batch holds the kinds it is meant to
exercise.  Bar: bit-exact keys, fills and counts."""
import functools

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count, dev, dev_counts, host_counts
from tests.count_oracle import counts_of, radii
from tests.list_helper import PAD, assert_lists, dev_u64, host_u64, list_call, segments
from tests.list_oracle import lengths, lists_of, offsets_of
from tests.shards_helper import Shards
from tests.test_count_exact_gpu import M, N, TIE_A, TIE_B, batch
from tests.test_masked_gpu import dev_words, masked, mcount, shapes, want_keys, words_of, words_to_bits
from tests.test_topk_large_gpu import large
from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index, topk_keys, v0_dist2
from tests.within_helper import dev_keys, host_keys, within

pytestmark = pytest.mark.gpu
INF = float("inf")
BASE = 9
KL = 100                                   # the large call's K where the case does not say: above 64, below the admitted rows
FORMS = [1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129]


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in ("path", "cells"):
        pkg.set_option(name, 0)


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def mlist(ix, Q, r2, words, offsets, fill=None, keys=None, init=True, slot=0):
    """One call of list_within_masked on segments `offsets` (numpy uint64 [m + 1]): (fill uint32 [m], keys uint64) after it.
    Without `fill` the cursor held 0xDEADBEEF (init) or zeros (appending); without `keys` the buffer held PAD."""
    Qf = np.array(Q, dtype=np.float32).reshape(-1)            # (a copy: the shared batch is read-only)
    m = Qf.size // ix.k
    q_d, w_d, off_d = torch.from_numpy(Qf).to(dev()), dev_words(words), dev_u64(offsets)
    if fill is None:
        fill = dev_counts(m, fill=0xDEADBEEF if init else 0)
    if keys is None:
        keys = dev_u64(np.full(max(int(offsets[m]), 1), PAD))
    torch.cuda.synchronize()
    ix.list_within_masked(m, q_d.data_ptr(), r2, w_d.data_ptr(), off_d.data_ptr(), fill.data_ptr(), keys.data_ptr(), init=init,
                          slot=slot)
    torch.cuda.synchronize()
    return host_counts(fill), host_u64(keys)


def mlarge(ix, Q, K, r2, words, keys=None, init=True, slot=0):
    """One call of query_topk_large_masked: keys [m][K] (numpy uint64) after it; the indices it unpacked are those of the keys."""
    Qf = np.array(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d, w_d = torch.from_numpy(Qf).to(dev()), dev_words(words)
    if keys is None:
        keys = dev_keys(m, K, fill=np.full(m * K, 0xDEADBEEFDEADBEEF if init else KEY_INIT, dtype=np.uint64))
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    ix.query_topk_large_masked(m, K, q_d.data_ptr(), w_d.data_ptr(), keys.data_ptr(), max_dist2=r2, init_keys=init,
                               indices_dev=ind.data_ptr(), slot=slot)
    torch.cuda.synchronize()
    got = host_keys(keys, m, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return got


def rows_of(n, sel):
    """The ascending local rows a selection (indices or a boolean array) admits, through the mask words themselves."""
    return np.flatnonzero(words_to_bits(words_of(n, sel), n))


def want_lists(d, rows, r2, base=BASE, gids=None):
    """The oracle's lists over the admitted rows (ascending local rows) of the distance matrix d [m][n], numbered base + row or
    gids[row]."""
    rows = np.asarray(rows, dtype=np.int64)
    g = (rows + base) if gids is None else np.asarray(gids)[rows]
    return lists_of(d[:, rows], r2, gids=g)


def check_list(ix, Q, d, sel, r2, base=BASE, msg=""):
    """An init call on segments of exactly the expected lengths: fill is the count, the segments hold the expected keys."""
    n = d.shape[1]
    want = want_lists(d, rows_of(n, sel), r2, base)
    off = offsets_of(lengths(want))
    fill, keys = mlist(ix, Q, r2, words_of(n, sel), off)
    np.testing.assert_array_equal(fill, lengths(want), err_msg=f"fill {msg} r2={r2}")
    assert_lists(segments(off, fill, keys), want, f"lists {msg} r2={r2}")
    assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()


def check_large(ix, Q, R, k, K, sel, r2, base=BASE, msg=""):
    n = R.shape[0]
    got = mlarge(ix, Q, K, r2, words_of(n, sel))
    np.testing.assert_array_equal(got, want_keys(Q, R, k, K, rows_of(n, sel), r2, base), err_msg=f"keys {msg} K={K} r2={r2}")
    st = ix.last_stats()
    assert st[0] == 1 and st[1] == 0 and st[2] in (0, 1) and st[3] == 0, st


@functools.lru_cache(maxsize=None)
def data(k):
    R, Q = batch(k, 9500 + k)
    d = v0_dist2(Q, R, k)
    assert d[3, TIE_A] == d[3, TIE_B] and np.isnan(d[:, 5]).all() and np.isinf(d[:, 6]).all() and np.isinf(d[:, 7]).all()
    for a in (R, Q, d):
        a.setflags(write=False)
    return R, Q, d


# ---- 1. every compiled form -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prep_forms(k):
    R, Q, d = data(k)
    half = np.random.default_rng(1100 + k).random(N) < 0.5
    half[[5, 6, 7]] = True                       # the rows without a finite distance stay admitted: they must not get in
    rows = np.flatnonzero(half)
    rs = radii(d[:, rows])                       # (asserts a zero count and counts of 1 .. 63 at `at` and `below`)
    at, big = dict(rs)["at"], dict(rs)["large"]
    assert (counts_of(d, at) > counts_of(d[:, rows], at)).any(), "no query has an excluded row inside the radius"
    assert (counts_of(d[:, rows], at) == 0).any(), "no query without a hit"
    cb = counts_of(d[:, rows], big)
    assert (cb < KL).any() and (counts_of(d[:, rows], INF) > KL).all(), "no query with fewer / more admitted candidates than K"
    return R, Q, d, half, [r for _, r in rs], big


@pytest.mark.parametrize("k", FORMS)
def test_every_compiled_form_with_a_random_half_mask(k):
    R, Q, d, half, rs, big = prep_forms(k)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for r2 in rs:                            # at, below, 0, +INF, under every distance, large
            check_list(ix, Q, d, half, r2, msg=f"k={k}")
        for r2 in (INF, big):
            check_large(ix, Q, R, k, KL, half, r2, msg=f"k={k}")
    finally:
        ix.close()


# ---- 2. mask shapes -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prep_shapes(k):
    R, Q, d = data(k)
    big = dict(radii(d))["large"]                # more than 64 rows of the whole set within it for some query, none for others
    all_rows, tail = shapes(np.random.default_rng(1200 + k))
    all_rows = all_rows + [("range_deep_in_the_shard", np.arange(2900, 3100)), ("runs_of_8", (np.arange(N) // 8) % 2 == 0)]
    half = rows_of(N, all_rows[-3][1])
    assert all_rows[-3][0] == "half"
    assert (counts_of(d, big) > counts_of(d[:, half], big)).any() and (counts_of(d[:, half], big) == 0).any()
    assert (counts_of(d[:, half], big) < KL).any() and (counts_of(d[:, half], INF) > KL).all()
    return R, Q, d, all_rows, tail, big


@pytest.mark.parametrize("k", [3, 17])
def test_mask_shapes(k):
    R, Q, d, all_rows, tail, big = prep_shapes(k)
    ones = np.full(pkg.mask_words(N), 0xFFFFFFFF, dtype=np.uint32)
    none = words_of(N, [])
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for r2 in (INF, big):
            check_list(ix, Q, d, np.arange(N), r2, msg=f"all_ones k={k}")
            check_large(ix, Q, R, k, KL, np.arange(N), r2, msg=f"all_ones k={k}")
            for name, sel in all_rows:
                check_list(ix, Q, d, sel, r2, msg=f"{name} k={k}")
                check_large(ix, Q, R, k, KL, sel, r2, msg=f"{name} k={k}")
            # all zero: nothing stored, the cursor at its entry value; padding
            off = offsets_of(np.full(M, 3))
            fill, keys = mlist(ix, Q, r2, none, off, fill=dev_counts(M, fill=5), init=False)
            assert (fill == 5).all() and (keys == PAD).all()
            fill, keys = mlist(ix, Q, r2, none, off)
            assert (fill == 0).all() and (keys == PAD).all()
            assert (mlarge(ix, Q, KL, r2, none) == KEY_INIT).all()
            assert (mlarge(ix, Q, KL, r2, words_of(N, [5, 6, 7])) == KEY_INIT).all()
            # garbage bits at and beyond N change nothing
            half = words_of(N, all_rows[-3][1])
            off_half = offsets_of(lengths(want_lists(d, rows_of(N, all_rows[-3][1]), r2)))
            fa, ka = mlist(ix, Q, r2, half | tail, off_half)
            fb, kb = mlist(ix, Q, r2, half, off_half)
            np.testing.assert_array_equal(fa, fb)
            assert_lists(segments(off_half, fa, ka), segments(off_half, fb, kb))
            np.testing.assert_array_equal(mlarge(ix, Q, KL, r2, half | tail), mlarge(ix, Q, KL, r2, half))
            assert (mlarge(ix, Q, KL, r2, tail) == KEY_INIT).all() and (mlist(ix, Q, r2, tail, off)[0] == 0).all()
    finally:
        ix.close()


# ---- 3. equalities --------------------------------------------------------------------------------------------------------------
def test_an_all_ones_mask_equals_the_unmasked_calls():
    k = 17
    R, Q, d = data(k)
    rs = dict(radii(d))
    ones = np.full(pkg.mask_words(N), 0xFFFFFFFF, dtype=np.uint32)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for r2 in (rs["at"], rs["large"], INF):
            off = offsets_of(counts_of(d, r2))
            f0, k0 = list_call(ix, Q.copy(), r2, off)
            f1, k1 = mlist(ix, Q, r2, ones, off)
            np.testing.assert_array_equal(f1, f0)
            assert_lists(segments(off, f1, k1), segments(off, f0, k0), f"r2={r2}")
        for K in (KL, 4096):
            for r2 in (rs["large"], INF):
                np.testing.assert_array_equal(mlarge(ix, Q, K, r2, ones), large(ix, Q.copy(), K, r2), err_msg=f"K={K} r2={r2}")
    finally:
        ix.close()


def test_k_up_to_64_equals_the_masked_top_k_bit_for_bit():
    k = 17
    R, Q, d = data(k)
    Qbad = np.concatenate([Q, Q[:3]])
    Qbad[-3, 4] = np.nan                                # a query with a NaN coordinate
    Qbad[-2] = 1e30                                     # one whose distances overflow
    Qbad[-1, 0] = np.inf
    half = np.random.default_rng(1300).random(N) < 0.5
    half[[5, 6, 7]] = True
    at = dict(radii(d[:, np.flatnonzero(half)]))["at"]
    w = words_of(N, half)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for K in (1, 8, 64):
            for r2 in (INF, at):
                ref = masked(ix, Qbad, K, r2, w)
                got = mlarge(ix, Qbad, K, r2, w)
                np.testing.assert_array_equal(got, ref, err_msg=f"K={K} r2={r2}")
                np.testing.assert_array_equal(got[:M], want_keys(Q, R, k, K, np.flatnonzero(half), r2))
                assert (got[M:] == KEY_INIT).all()
    finally:
        ix.close()


# ---- 4. ties --------------------------------------------------------------------------------------------------------------------
BLOCK0 = 500                                            # first row of the block of KL + 5 identical rows


@functools.lru_cache(maxsize=None)
def prep_ties():
    """Rows: the batch with a block of KL + 5 copies of one point.  Queries: a tight cloud around a point next to the block, so that
    for EVERY query the block is (all but) the nearest thing and the K-th place falls into it or behind it as the mask decides."""
    k = 3
    R, Q0 = batch(k, 9700)
    R = R.copy()
    rng = np.random.default_rng(9701)
    centre = np.array([0.4, 0.5, 0.6], dtype=np.float32)
    Q = (centre + rng.normal(0.0, 0.002, size=(M, k))).astype(np.float32)
    block = np.arange(BLOCK0, BLOCK0 + KL + 5)
    R[block] = centre + np.float32(0.01)
    d = v0_dist2(Q, R, k)
    assert (d[:, block] == d[:, block[:1]]).all()
    nearer = (d < d[:, BLOCK0:BLOCK0 + 1]).sum(axis=1)                   # rows nearer than the block, per query
    assert nearer.max() < 10, nearer.max()
    others = np.ones(N, dtype=bool)
    others[block] = False
    # part of the block, the lowest numbers excluded: more copies than places -> the cut falls inside the class
    part = others.copy()
    part[block[3:]] = True
    # fewer copies than KL - (nearer rows), for every query -> the class fits whole
    few = others.copy()
    few[block[5:5 + KL - 20]] = True
    out = {}
    for name, sel in (("part", part), ("few", few)):
        rows = np.flatnonzero(sel)
        more = want_keys(Q, R, k, KL + 1, rows, INF)
        tie = (keys_dist2(more[:, KL - 1]) == keys_dist2(more[:, KL])) & (more[:, KL] != KEY_INIT)
        out[name] = (sel, more[:, :KL], tie)
    assert out["part"][2].all(), "some query's cut is not inside the block"
    assert not out["few"][2].any(), "some query's cut falls inside a class although the block fits"
    # the lowest ADMITTED numbers win: rows block[3] .. of the block, not block[0 .. 2], and not the highest
    q0 = keys_index(out["part"][1][0])
    assert BASE + BLOCK0 + 3 in q0 and BASE + BLOCK0 not in q0 and BASE + BLOCK0 + KL + 4 not in q0
    # the pair of equal rows, for the batch's own queries
    d0 = v0_dist2(Q0, R, k)
    assert d0[3, TIE_A] == d0[3, TIE_B]
    return R, Q, Q0, d0, out


def test_ties_the_cut_inside_an_admitted_class_and_a_class_that_fits():
    k = 3
    R, Q, Q0, d0, cases = prep_ties()
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        sel, want, _ = cases["part"]
        np.testing.assert_array_equal(mlarge(ix, Q, KL, INF, words_of(N, sel)), want)
        assert ix.last_stats() == [1, 0, 1, 0], ix.last_stats()          # the index word's passes ran
        sel, want, _ = cases["few"]
        np.testing.assert_array_equal(mlarge(ix, Q, KL, INF, words_of(N, sel)), want)
        assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()          # ... and here they stayed gated off
        # the pair of equal rows: whichever copies the mask admits, at the tie's radius and just below it
        tie = float(d0[3, TIE_A])
        below = float(np.nextafter(np.float32(tie), np.float32(0)))
        for pick in ([TIE_A], [TIE_B], [TIE_A, TIE_B], [TIE_A, TIE_B, 40, 2500]):
            for r2 in (tie, below, INF):
                check_list(ix, Q0, d0, pick, r2, msg=f"tie {pick}")
                check_large(ix, Q0, R, k, KL, pick, r2, msg=f"tie {pick}")
    finally:
        ix.close()


# ---- 5. overflow of a segment ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prep_overflow(k):
    R, Q, d = data(k)
    half = np.random.default_rng(1500 + k).random(N) < 0.5
    rows = np.flatnonzero(half)
    r2 = dict(radii(d[:, rows]))["large"]
    # every query twice: the copy is non-finite and owns a segment of one entry — the canary BETWEEN two real segments
    Q2 = np.repeat(Q, 2, axis=0)
    Q2[1::2, 0] = np.nan
    want = want_lists(d, rows, r2)
    cnt = lengths(want)
    rooms = np.where(np.arange(M) % 3 == 0, cnt, np.maximum(cnt.astype(np.int64) - 2, 0)).astype(np.uint64)
    short = rooms < cnt
    assert short.any() and (~short & (cnt > 0)).any() and (cnt == 0).any() and (cnt > 64).any()
    assert (counts_of(d, r2) > cnt).any(), "no query has an excluded row inside the radius"
    return R, Q2, half, r2, want, cnt, rooms, short


@pytest.mark.parametrize("k", [3, 17, 129])
def test_overflowing_segments_store_nothing_outside_them(k):
    R, Q2, half, r2, want, cnt, rooms, short = prep_overflow(k)
    both = np.ones(2 * M, dtype=np.uint64)
    both[0::2] = rooms
    exact = np.zeros(2 * M + 1, dtype=np.uint64)
    exact[0] = 1                                                         # a canary in front of the first segment
    exact[1:] = 1 + np.cumsum(both)
    buf = np.full(int(exact[-1]) + 2, PAD, dtype=np.uint64)              # ... and two behind the last
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        fill, keys = mlist(ix, Q2, r2, words_of(N, half), exact, keys=dev_u64(buf))
        np.testing.assert_array_equal(fill[0::2], cnt, err_msg="fill is the admitted count whether or not a hit was stored")
        assert (fill[1::2] == 0).all()
        np.testing.assert_array_equal(fill[0::2] > rooms, short)         # fill > room for exactly the short segments
        assert keys[0] == PAD and (keys[int(exact[-1]):] == PAD).all(), "a canary in front of or behind the segments changed"
        for j in range(M):
            assert keys[int(exact[2 * j + 1])] == PAD, f"the canary behind segment {j} changed"
            got = keys[int(exact[2 * j]):int(exact[2 * j + 1])]
            assert got.size == rooms[j] and np.isin(got, want[j]).all() and np.unique(got).size == got.size
            if not short[j]:
                np.testing.assert_array_equal(np.sort(got), want[j])
    finally:
        ix.close()


# ---- 6. folds -------------------------------------------------------------------------------------------------------------------
def fold_of(held, lists):
    return np.sort(np.concatenate([held, lists], axis=1), axis=1)[:, :held.shape[1]]


def test_two_shards_with_their_own_masks_append_and_fold():
    k, cut = 17, 1500
    R, Q, d = data(k)
    sel = np.random.default_rng(1600).random(N) < 0.3
    rows = np.flatnonzero(sel)
    rs = dict(radii(d[:, rows]))
    a, b = pkg.KnnIndex(k, R[:cut]), pkg.KnnIndex(k, R[cut:], base_index=cut)
    wa, wb = words_of(cut, sel[:cut]), words_of(N - cut, sel[cut:])
    try:
        for r2 in (rs["at"], rs["large"], INF):
            want = want_lists(d, rows, r2, base=0)
            first = lengths(want_lists(d, rows[rows < cut], r2, base=0))     # both shards give some query a hit
            assert (first > 0).any() and (lengths(want) > first).any()
            off = offsets_of(lengths(want))
            # with the init flag on the first ...
            fill_d, keys_d = dev_counts(M, fill=0xDEADBEEF), dev_u64(np.full(max(int(off[-1]), 1), PAD))
            mlist(a, Q, r2, wa, off, fill=fill_d, keys=keys_d, init=True)
            fill, keys = mlist(b, Q, r2, wb, off, fill=fill_d, keys=keys_d, init=False)
            np.testing.assert_array_equal(fill, lengths(want))
            assert_lists(segments(off, fill, keys), want, f"two shards r2={r2}")
            # ... and without: both append behind a cursor the caller zeroed
            fill_d, keys_d = dev_counts(M, fill=0), dev_u64(np.full(max(int(off[-1]), 1), PAD))
            mlist(b, Q, r2, wb, off, fill=fill_d, keys=keys_d, init=False)
            fill, keys = mlist(a, Q, r2, wa, off, fill=fill_d, keys=keys_d, init=False)
            np.testing.assert_array_equal(fill, lengths(want))
            assert_lists(segments(off, fill, keys), want, f"two shards appending r2={r2}")
            # the large list: init on the first, and both folding into padding
            wantk = want_keys(Q, R, k, KL, rows, r2, base=0)
            keys = dev_keys(M, KL, fill=np.full(M * KL, 0xDEADBEEFDEADBEEF, dtype=np.uint64))
            mlarge(a, Q, KL, r2, wa, keys=keys, init=True)
            np.testing.assert_array_equal(mlarge(b, Q, KL, r2, wb, keys=keys, init=False), wantk, err_msg=f"fold r2={r2}")
            keys = dev_keys(M, KL, fill=np.full(M * KL, KEY_INIT, dtype=np.uint64))
            mlarge(b, Q, KL, r2, wb, keys=keys, init=False)
            np.testing.assert_array_equal(mlarge(a, Q, KL, r2, wa, keys=keys, init=False), wantk, err_msg=f"fold, no init r2={r2}")
        # a fold into caller keys that lie beyond the radius: they are the caller's and are not clipped
        finite = rs["large"]
        far = np.float32(finite) * np.float32(4.0)
        held = np.full((M, KL), KEY_INIT, dtype=np.uint64)
        held[:, 0] = (np.uint64(far.view(np.uint32)) << np.uint64(32)) | np.uint64(77)
        held[:, 1] = (np.uint64(np.float32(far * 2).view(np.uint32)) << np.uint64(32)) | np.uint64(3)
        got = mlarge(b, Q, KL, finite, wb, keys=dev_keys(M, KL, fill=held), init=False)
        mine = want_keys(Q, R[cut:], k, KL, np.flatnonzero(sel[cut:]), finite, base=cut)
        np.testing.assert_array_equal(got, fold_of(held, mine))
        assert (got == held[0, 0]).any() and (got == held[0, 1]).any()
    finally:
        a.close()
        b.close()


def test_a_cell_range_shard_pair_folds_with_gids_under_masks_in_local_row_order():
    rng = np.random.default_rng(1700)
    k, n, m = 16, (1 << 19) + 5, 24
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    sel = rng.random(n) < 1 / 16
    rows = np.flatnonzero(sel)
    d = v0_dist2(Q, R[rows], k)
    r2 = float(np.sort(d, axis=1)[:, 40].min())               # about 40 admitted rows for the nearest query, fewer for the others
    want = lists_of(d, r2, gids=rows)
    wantk = want_keys(Q, R, k, KL, rows, INF, base=0)
    assert (lengths(want) > 0).any() and (lengths(want) < 40).any()
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=False)
    try:
        gids = [g.cpu().numpy().astype(np.int64) for g in sh.gids]
        local = [words_of(g.size, sel[g]) for g in gids]             # bit i = local row i = global row gids[i]
        assert int(keys_index(wantk).max()) >= sh.rows[0].shape[0]   # numbers no local row of rank 0 has
        off = offsets_of(lengths(want))
        fill_d, keys_d = dev_counts(m, fill=0xDEADBEEF), dev_u64(np.full(max(int(off[-1]), 1), PAD))
        kd = dev_keys(m, KL)
        for r, ix in enumerate(sh.idx):
            fill, keys = mlist(ix, Q, r2, local[r], off, fill=fill_d, keys=keys_d, init=(r == 0))
            assert ix.last_stats() == [1, 0, 0, 0]
            got = mlarge(ix, Q, KL, INF, local[r], keys=kd, init=(r == 0))
        np.testing.assert_array_equal(fill, lengths(want))
        assert_lists(segments(off, fill, keys), want, "cell-range shards")
        np.testing.assert_array_equal(got, wantk)
    finally:
        sh.close()


# ---- 7. small ends --------------------------------------------------------------------------------------------------------------
def test_one_query_k_4096_beyond_the_admitted_rows_and_tiny_shards():
    k = 16
    R, Q, d = data(k)
    sel = np.flatnonzero(np.random.default_rng(1800).random(N) < 0.4)
    w = words_of(N, sel)
    at = dict(radii(d[:, sel]))["at"]
    assert sel.size < 4096
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for j in (0, 33, M - 1):                                   # m = 1
            for r2 in (INF, at):
                check_list(ix, Q[j:j + 1], d[j:j + 1], sel, r2, msg=f"m=1 j={j}")
                check_large(ix, Q[j:j + 1], R, k, KL, sel, r2, msg=f"m=1 j={j}")
        # K = 4096 with fewer admitted candidates: padding behind them, and the host call's counts
        want = want_keys(Q, R, k, 4096, sel, INF)
        n_fin = sel.size - np.isin([5, 6, 7], sel).sum()
        assert ((want != KEY_INIT).sum(axis=1) == n_fin).all()
        np.testing.assert_array_equal(mlarge(ix, Q, 4096, INF, w), want)
        ind, d2, cnt = ix.query_topk_large_masked_host(Q, 4096, w)
        np.testing.assert_array_equal(ind, keys_index(want))
        assert (cnt == n_fin).all()
    finally:
        ix.close()
    rng = np.random.default_rng(1801)
    for n in (31, 33):
        Rn = R[100:100 + n]
        dn = v0_dist2(Q, Rn, k)
        ix = pkg.KnnIndex(k, Rn, base_index=BASE)
        try:
            for name, pick in (("ones", np.arange(n)), ("half", rng.random(n) < 0.5), ("last", [n - 1]), ("none", [])):
                for r2 in (INF, float(np.median(dn))):
                    check_list(ix, Q, dn, pick, r2, msg=f"n={n} {name}")
                    check_large(ix, Q, Rn, k, 70, pick, r2, msg=f"n={n} {name}")
        finally:
            ix.close()
    empty = pkg.KnnIndex(k, R[:0], n_local=0)
    try:
        none = np.zeros(1, dtype=np.uint32)       # (a mask of no words: the pointer is only checked)
        held = np.sort(np.random.default_rng(1).integers(1, 1 << 62, size=(M, KL), dtype=np.uint64), axis=1)
        np.testing.assert_array_equal(mlarge(empty, Q, KL, INF, none, keys=dev_keys(M, KL, fill=held), init=False), held)
        assert (mlarge(empty, Q, KL, INF, none) == KEY_INIT).all()
        off = offsets_of(np.full(M, 4))
        fill, keys = mlist(empty, Q, 0.5, none, off, fill=dev_counts(M, fill=5), init=False)
        assert (fill == 5).all() and (keys == PAD).all()
        fill, keys = mlist(empty, Q, 0.5, none, off)
        assert (fill == 0).all() and (keys == PAD).all()
        assert empty.last_stats() == [1, 0, 0, 0]
    finally:
        empty.close()


# ---- 8. other index kinds -------------------------------------------------------------------------------------------------------
def test_an_index_with_a_grid_and_one_with_a_cell_sorted_layout_answer_with_a_plain_indexs_keys():
    m = 70
    for k, n, opt in ((3, 16384, None), (16, 1 << 17, "cells")):
        rng = np.random.default_rng(1900 + k)
        R = rng.random((n, k), dtype=np.float32)
        Q = rng.random((m, k), dtype=np.float32)
        sel = np.flatnonzero(rng.random(n) < 1 / 16)
        w = words_of(n, sel)
        d = v0_dist2(Q, R[sel], k)
        r2 = float(np.sort(d, axis=1)[:, 30].min())
        want = lists_of(d, r2, gids=sel + BASE)
        wantk = want_keys(Q, R, k, KL, sel, INF)
        assert (lengths(want) >= 30).any() and (lengths(want) < 30).any()
        off = offsets_of(lengths(want))
        pkg.set_option("path", 1)
        plain_ix = pkg.KnnIndex(k, R, base_index=BASE)             # exact kernels only: no grid, no layout
        pkg.set_option("path", 0)
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
                f0, k0 = mlist(plain_ix, Q, r2, w, off)
                f1, k1 = mlist(ix, Q, r2, w, off)
                assert ix.last_stats() == [1, 0, 0, 0]
                np.testing.assert_array_equal(f1, f0)
                np.testing.assert_array_equal(f1, lengths(want))
                assert_lists(segments(off, f1, k1), segments(off, f0, k0))
                assert_lists(segments(off, f1, k1), want)
                g1 = mlarge(ix, Q, KL, INF, w)
                np.testing.assert_array_equal(g1, mlarge(plain_ix, Q, KL, INF, w))
                np.testing.assert_array_equal(g1, wantk)
            finally:
                ix.close()
        finally:
            plain_ix.close()
            if opt:
                pkg.set_option(opt, 0)


# ---- 9. slot reuse and the host calls -------------------------------------------------------------------------------------------
def test_every_kind_of_call_in_turn_on_one_slot_and_the_host_calls():
    k = 16
    R, Q, d = data(k)
    rng = np.random.default_rng(2000)
    sel, other = np.flatnonzero(rng.random(N) < 0.4), np.flatnonzero(rng.random(N) < 0.1)
    w, w2 = words_of(N, sel), words_of(N, other)
    r2 = dict(radii(d[:, sel]))["large"]
    every = np.arange(N)
    assert (counts_of(d[:, sel], r2) == 0).any() and (counts_of(d, r2) > counts_of(d[:, sel], r2)).any()
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for slot in (0, 5):
            q_d = torch.from_numpy(Q.reshape(-1).copy()).to(dev())
            keys1 = torch.empty(M, dtype=torch.int64, device=dev())
            ix.query_keys(M, q_d.data_ptr(), keys1.data_ptr(), init_keys=True, slot=slot)                    # 1-NN
            torch.cuda.synchronize()
            np.testing.assert_array_equal(keys1.cpu().numpy().view(np.uint64), want_keys(Q, R, k, 1, every, INF)[:, 0])
            np.testing.assert_array_equal(within(ix, Q.copy(), 64, r2, slot=slot), want_keys(Q, R, k, 64, every, r2))   # top-K
            np.testing.assert_array_equal(count(ix, Q.copy(), r2, slot=slot), counts_of(d, r2))             # count
            wl = want_lists(d, every, r2)
            off = offsets_of(lengths(wl))
            f, kk = list_call(ix, Q.copy(), r2, off, slot=slot)                                             # list
            assert_lists(segments(off, f, kk), wl)
            np.testing.assert_array_equal(large(ix, Q.copy(), KL, r2, slot=slot), want_keys(Q, R, k, KL, every, r2))   # large
            np.testing.assert_array_equal(masked(ix, Q, 8, r2, w, slot=slot), want_keys(Q, R, k, 8, sel, r2))   # masked top-K
            wl = want_lists(d, sel, r2)
            off = offsets_of(lengths(wl))
            f, kk = mlist(ix, Q, r2, w, off, slot=slot)                                                     # masked list
            np.testing.assert_array_equal(f, lengths(wl))
            assert_lists(segments(off, f, kk), wl)
            np.testing.assert_array_equal(mlarge(ix, Q, KL, r2, w, slot=slot), want_keys(Q, R, k, KL, sel, r2))   # masked large
            np.testing.assert_array_equal(mcount(ix, Q, r2, w2, slot=slot), counts_of(d[:, other], r2))     # ... another mask
            np.testing.assert_array_equal(mlarge(ix, Q, 300, INF, w2, slot=slot), want_keys(Q, R, k, 300, other, INF))
            np.testing.assert_array_equal(large(ix, Q.copy(), KL, r2, slot=slot), want_keys(Q, R, k, KL, every, r2))
        # the host calls against the device calls (and the oracle)
        for rr in (r2, INF):
            wl = want_lists(d, sel, rr)
            off = offsets_of(lengths(wl))
            f, kk = mlist(ix, Q, rr, w, off)
            offs_h, ind_h, d2_h = ix.list_within_masked_host(Q, rr, w)
            np.testing.assert_array_equal(offs_h.astype(np.uint64), off)
            flat = np.concatenate(segments(off, f, kk)) if int(off[-1]) else np.zeros(0, dtype=np.uint64)
            np.testing.assert_array_equal(ind_h, keys_index(flat))
            np.testing.assert_array_equal(d2_h.view(np.uint32), (flat >> np.uint64(32)).astype(np.uint32))
            got = mlarge(ix, Q, KL, rr, w)
            ind, d2, cnt = ix.query_topk_large_masked_host(Q, KL, w, max_dist2=rr)
            np.testing.assert_array_equal(ind, keys_index(got))
            np.testing.assert_array_equal(d2.view(np.uint32), (got >> np.uint64(32)).astype(np.uint32))
            np.testing.assert_array_equal(cnt, (got != KEY_INIT).sum(axis=1))
        offs_h, ind_h, d2_h = ix.list_within_masked_host(Q, 0.0, w)           # a total of zero: empty arrays
        assert (offs_h == 0).all() and ind_h.size == 0 and d2_h.size == 0
        with pytest.raises(ValueError):
            ix.query_topk_large_masked_host(Q, KL, w[:-1])
        with pytest.raises(ValueError):
            ix.list_within_masked_host(Q, 1.0, w[:-1])
        q_d = torch.from_numpy(Q.reshape(-1).copy()).to(dev())
        with pytest.raises(pkg.KnnError, match="knn_index_query_topk_large_masked: unknown flag"):
            ix.query_topk_large_masked(M, KL, q_d.data_ptr(), dev_words(w).data_ptr(), dev_keys(M, KL).data_ptr(), flags=64)
        with pytest.raises(pkg.KnnError, match="knn_index_list_within_masked: unknown flag"):
            ix.list_within_masked(M, q_d.data_ptr(), 1.0, dev_words(w).data_ptr(), dev_u64(np.zeros(M + 1)).data_ptr(),
                                  dev_counts(M, fill=0).data_ptr(), dev_u64(np.zeros(1)).data_ptr(), flags=4)
    finally:
        ix.close()


# ---- 10. the chunk boundary -----------------------------------------------------------------------------------------------------
def test_a_batch_just_across_the_chunk_of_65536_queries():
    rng = np.random.default_rng(2100)
    k, n, m, K = 2, 300, 65536 + 3, 70
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    half = rng.random(n) < 0.5
    rows = np.flatnonzero(half)
    assert rows.size > K
    r2 = 0.01                                                  # a disc of about 0.03 of the unit square: ~4 of ~150 admitted rows
    wantk = want_keys(Q, R, k, K, rows, INF)
    cnt = counts_of_chunks(Q, R[rows], k, r2)
    assert (cnt == 0).any() and (cnt > 0).any() and cnt[-3:].sum() > 0, "the queries behind the boundary have no hit"
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        w = words_of(n, half)
        got = mlarge(ix, Q, K, INF, w)
        np.testing.assert_array_equal(got, wantk)
        off = offsets_of(cnt)
        fill, keys = mlist(ix, Q, r2, w, off)
        np.testing.assert_array_equal(fill, cnt)
        # the lists are the radius-clipped prefix of the top-K order (cnt < K for every query)
        assert int(cnt.max()) < K
        for j in (0, 1, 65535, 65536, 65537, m - 1) + tuple(np.flatnonzero(cnt == cnt.max())[:2]):
            np.testing.assert_array_equal(np.sort(keys[int(off[j]):int(off[j + 1])]), wantk[j, :int(cnt[j])], err_msg=f"query {j}")
        flat = np.concatenate([np.sort(keys[int(off[j]):int(off[j + 1])]) for j in range(65530, m)])
        np.testing.assert_array_equal(flat, np.concatenate([wantk[j, :int(cnt[j])] for j in range(65530, m)]))
    finally:
        ix.close()


def counts_of_chunks(Q, R, k, r2, chunk=8192):
    return np.concatenate([counts_of(v0_dist2(Q[c:c + chunk], R, k), r2) for c in range(0, Q.shape[0], chunk)])
