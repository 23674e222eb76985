"""Queries about the shard's own rows on the GPU (knn_index_self_topk, knn_index_self_count_within, knn_index_self_list_within and
the two host calls; include/knn_mi355x.h 2i): every result bit for bit against tests/self_oracle.py."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import dev, dev_counts, host_counts
from tests.list_helper import PAD, assert_lists, dev_u64, host_u64, segments
from tests.list_oracle import lengths, offsets_of
from tests.self_oracle import fold, self_counts, self_dist2, self_lists, self_topk
from tests.shards_helper import Shards
from tests.test_count_exact_gpu import N, TIE_A, TIE_B, batch
from tests.topk_oracle import KEY_INIT, keys_index, topk_keys, v0_dist2

pytestmark = pytest.mark.gpu
INF = float("inf")
BASE = 9
OPTIONS = ("path", "cells", "topk_cells", "cells_rows", "cells_centre")
WINDOWS = [(0, 70), (N - 70, 70), (2090, 20)]   # the shard's first rows, its last (a second window of 6), rows around TIE_B = 2100


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def dev_keys(rows, K, fill=None):
    """A key buffer [rows][K] on the device: PAD everywhere, or the given keys."""
    a = np.full((rows, K), PAD, dtype=np.uint64) if fill is None else np.asarray(fill, dtype=np.uint64)
    return dev_u64(a.reshape(-1))


def stopk(ix, first, rows, K, r2=INF, keys=None, init=True, slot=0, **kw):
    """One self_topk call: the keys [rows][K] after it; the int32 indices it also writes must be the keys' index halves."""
    if keys is None:
        keys = dev_keys(rows, K)
    ind = torch.full((rows * K,), -7, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    ix.self_topk(first, rows, K, keys.data_ptr(), max_dist2=r2, init_keys=init, indices_dev=ind.data_ptr(), slot=slot, **kw)
    torch.cuda.synchronize()
    got = host_u64(keys).reshape(rows, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(rows, K), keys_index(got))
    return got


def scount(ix, first, rows, r2, counts=None, init=True, slot=0):
    if counts is None:
        counts = dev_counts(rows, fill=0xDEADBEEF if init else 0)
    torch.cuda.synchronize()
    ix.self_count_within(first, rows, r2, counts.data_ptr(), init=init, slot=slot)
    torch.cuda.synchronize()
    return host_counts(counts)


def slist(ix, first, rows, r2, offsets, fill=None, keys=None, init=True, slot=0):
    off_d = dev_u64(offsets)
    if fill is None:
        fill = dev_counts(rows, fill=0xDEADBEEF if init else 0)
    if keys is None:
        keys = dev_u64(np.full(max(int(offsets[rows]), 1), PAD))
    torch.cuda.synchronize()
    ix.self_list_within(first, rows, r2, off_d.data_ptr(), fill.data_ptr(), keys.data_ptr(), init=init, slot=slot)
    torch.cuda.synchronize()
    return host_counts(fill), host_u64(keys)


def count_offsets_list_sort(ix, first, rows, r2):
    """The four steps a caller makes, all on the device: self count -> offsets -> self list -> sort; (counts, offsets, keys)."""
    counts = dev_counts(rows, fill=0xDEADBEEF)
    off_d = dev_u64(np.zeros(rows + 1))
    fill = dev_counts(rows, fill=0xDEADBEEF)
    ix.self_count_within(first, rows, r2, counts.data_ptr(), init=True)
    pkg.counts_to_offsets(counts.data_ptr(), rows, off_d.data_ptr())
    torch.cuda.synchronize()
    off = host_u64(off_d)
    keys = dev_u64(np.full(max(int(off[rows]), 1), PAD))
    ix.self_list_within(first, rows, r2, off_d.data_ptr(), fill.data_ptr(), keys.data_ptr(), init=True)
    pkg.keys_sort_segments(rows, off_d.data_ptr(), fill.data_ptr(), keys.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host_counts(fill), host_counts(counts))
    return host_counts(counts), off, host_u64(keys)


def check_all(ix, R, k, first, rows, Ks, radii, msg, base=BASE):
    d = self_dist2(R, k, first, rows)
    for r2 in radii:
        for K in Ks:
            got = stopk(ix, first, rows, K, r2)
            assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()
            np.testing.assert_array_equal(got, self_topk(d, K, r2, base=base), err_msg=f"{msg} top-{K} r2={r2}")
        want = self_lists(d, r2, base=base)
        counts, off, keys = count_offsets_list_sort(ix, first, rows, r2)
        assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()
        np.testing.assert_array_equal(counts, self_counts(d, r2), err_msg=f"{msg} count r2={r2}")
        np.testing.assert_array_equal(off, offsets_of(lengths(want)))
        assert_lists([keys[int(off[j]):int(off[j + 1])] for j in range(rows)], want, f"{msg} list r2={r2}")
    return d


# ---- 1. every compiled form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16, 17, 32, 33, 128, 129])
def test_every_compiled_form_in_three_windows(k):
    R, _ = batch(k, 7100 + k)
    d_all = v0_dist2(R[2090:2110], R, k)
    # a finite distance some pair of DIFFERENT rows holds: row 2095's 12th nearest other row
    held = np.sort(np.delete(d_all[5], 2095)[np.delete(d_all[5], 2095) < np.inf])[11]
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for first, rows in WINDOWS:
            d = check_all(ix, R, k, first, rows, (1, 17, 64), (INF, float(held)), f"k={k} window {first}+{rows}")
            if first == 0:   # the NaN, +INF and 3e38 rows (5, 6, 7) as QUERIES: no candidate at all; as rows: nobody's neighbour
                assert (self_counts(d)[5:8] == 0).all() and (self_counts(d)[:5] == N - 4).all()
            if first == 2090:   # the copy of row TIE_A at TIE_B: its twin is its nearest other row, at distance 0
                assert self_topk(d, 1, base=BASE)[TIE_B - 2090, 0] == np.uint64(TIE_A + BASE) and d[TIE_B - 2090, TIE_B] != 0
    finally:
        ix.close()


# ---- 2. the whole shard in one call; tiny shards ----------------------------------------------------------------------------------
def test_the_whole_shard_in_one_call():
    k = 16
    R, _ = batch(k, 7200)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        slices = pkg.debug_self_plan(k=k, rows=N, K=8, shard_rows=N, num_cu=256, init=1)["slices"]
        assert slices == 1 or ((N + slices - 1) // slices) % 64 != 0   # windows fall inside, across and outside slices
        check_all(ix, R, k, 0, N, (8,), (INF,), "whole shard")
    finally:
        ix.close()


@pytest.mark.parametrize("n", [1, 2, 64, 65])
def test_tiny_shards(n):
    k = 3
    R = np.random.default_rng(7300 + n).random((n, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        d = check_all(ix, R, k, 0, n, (1, 3), (INF, 0.25), f"n={n}")
        if n == 1:
            assert (self_topk(d, 3) == KEY_INIT).all() and self_counts(d)[0] == 0
        else:
            assert (self_counts(d) == n - 1).all()
    finally:
        ix.close()


# ---- 3. copies ---------------------------------------------------------------------------------------------------------------------
def copies_set(k, n, seed, lo, hi):
    """n random rows, twelve of them — at sorted places in [lo, hi) — copies of one."""
    rng = np.random.default_rng(seed)
    R = rng.random((n, k), dtype=np.float32)
    at = np.sort(rng.choice(np.arange(lo, hi), size=12, replace=False))
    R[at] = R[at[0]]
    return R, at


def check_copies(ix, R, k, at, grid):
    first, rows = int(at[0]), int(at[-1] - at[0] + 1)
    d = self_dist2(R, k, first, rows)
    want = self_topk(d, 8, base=BASE)
    got = stopk(ix, first, rows, 8, grid=grid)
    np.testing.assert_array_equal(got, want)
    for a in at:   # eight OTHER copies at distance 0, ascending numbers, itself absent
        others = [int(x) + BASE for x in at if x != a][:8]
        assert [int(x) for x in got[a - first]] == others, a
    np.testing.assert_array_equal(scount(ix, first, rows, 0.0)[at - first], np.full(12, 11, dtype=np.uint32))


def test_twelve_copies_of_one_row_on_the_self_scan():
    k = 16
    R, at = copies_set(k, N, 7400, 100, N - 100)   # the copies lie in several slices
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        check_copies(ix, R, k, at, grid=False)
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_twelve_copies_of_one_row_on_the_grid_way_where_the_drop_removes_the_last_entry():
    """Among K + 1 = 9 nearest of a later copy are the nine first copies: the copy itself is not in the list, so what goes is the
    list's last entry."""
    k = 3
    R, at = copies_set(k, 16384, 7401, 5000, 5400)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        first, rows = int(at[0]), int(at[-1] - at[0] + 1)
        stopk(ix, first, rows, 8, grid=True)
        assert ix.last_stats()[0] == 3, ix.last_stats()
        check_copies(ix, R, k, at, grid=True)
        q = torch.from_numpy(R[at[-1]:at[-1] + 1]).to(dev())
        k9 = dev_keys(1, 9)
        ix.query_topk(1, 9, q.data_ptr(), k9.data_ptr(), init_keys=True, grid=True)
        torch.cuda.synchronize()
        assert int(at[-1]) + BASE not in [int(x) for x in keys_index(host_u64(k9))]
    finally:
        ix.close()


# ---- 4. folding ------------------------------------------------------------------------------------------------------------------
def test_two_index_range_shards_fold_to_the_whole_set_in_both_orders():
    k, K, first, rows, r2 = 16, 8, 1500, 100, None
    R, _ = batch(k, 7500)
    cut = 1550                                        # the window straddles the two shards: each takes its own rows' self call
    d = self_dist2(R, k, first, rows)
    r2 = float(np.sort(d[3][d[3] < np.inf])[20])
    A = pkg.KnnIndex(k, R[:cut], base_index=BASE)
    B = pkg.KnnIndex(k, R[cut:], base_index=BASE + cut)
    R_d = torch.from_numpy(R).to(dev())
    try:
        parts = ((A, first, cut - first, B, 0), (B, 0, first + rows - cut, A, cut - first))   # (own shard, local first, rows, other, at)
        for order in ("self first", "plain first"):
            keys = dev_keys(rows, K)
            counts = dev_counts(rows, fill=0xDEADBEEF)
            want = self_lists(d, r2, base=BASE)
            off = offsets_of(lengths(want))
            off_d, fill, lk = dev_u64(off), dev_counts(rows, fill=0xDEADBEEF), dev_u64(np.full(int(off[rows]), PAD))
            for own, lf, lr, other, at in parts:
                q = R_d[first + at:first + at + lr]
                kp, cp, fp, op = (keys.data_ptr() + at * K * 8, counts.data_ptr() + at * 4, fill.data_ptr() + at * 4, off_d.data_ptr() + at * 8)
                calls = [
                    lambda init: (own.self_topk(lf, lr, K, kp, max_dist2=r2, init_keys=init),
                                  own.self_count_within(lf, lr, r2, cp, init=init),
                                  own.self_list_within(lf, lr, r2, op, fp, lk.data_ptr(), init=init)),
                    lambda init: (other.query_topk_within(lr, K, q.data_ptr(), r2, kp, init_keys=init),
                                  other.count_within(lr, q.data_ptr(), r2, cp, init=init),
                                  other.list_within(lr, q.data_ptr(), r2, op, fp, lk.data_ptr(), init=init))]
                if order == "plain first":
                    calls.reverse()
                calls[0](True)
                calls[1](False)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(host_u64(keys).reshape(rows, K), self_topk(d, K, r2, base=BASE), err_msg=order)
            np.testing.assert_array_equal(host_counts(counts), self_counts(d, r2), err_msg=order)
            np.testing.assert_array_equal(host_counts(fill), lengths(want), err_msg=order)
            assert_lists(segments(off, host_counts(fill), host_u64(lk)), want, order)
    finally:
        A.close()
        B.close()


def test_a_cell_range_pair_carries_gids_and_excludes_by_local_row():
    k, K, rows = 16, 8, 24
    n = (1 << 19) + 5
    R = np.random.default_rng(7600).random((n, k), dtype=np.float32)
    R_d = torch.from_numpy(R).to(dev())
    sh = Shards(k, R_d, 2, attach=False)
    try:
        for r, ix in enumerate(sh.idx):
            gids = sh.gids[r].cpu().numpy().astype(np.int64)
            first = gids.size // 2
            mine = gids[first:first + rows]                       # the window's global rows
            assert not np.array_equal(mine, np.arange(first, first + rows))   # a gid is not the local row number
            d = v0_dist2(R[mine], R[gids], k)
            d[np.arange(rows), first + np.arange(rows)] = np.nan    # exclusion is by LOCAL row
            r2 = float(np.sort(d[0][d[0] < np.inf])[30])
            got = stopk(ix, first, rows, K)
            assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()      # a cell-range shard takes the self-scan
            np.testing.assert_array_equal(got, self_topk(d, K, gids=gids))
            np.testing.assert_array_equal(scount(ix, first, rows, r2), self_counts(d, r2))
            want = self_lists(d, r2, gids=gids)
            off = offsets_of(lengths(want))
            fill, keys = slist(ix, first, rows, r2, off)
            assert_lists(segments(off, fill, keys), want, f"rank {r}")
            # the other rank folds in through the plain call: the K nearest others of the whole set
            other = sh.idx[1 - r]
            og = sh.gids[1 - r].cpu().numpy().astype(np.int64)
            kd = dev_keys(rows, K, fill=got)
            q = sh.rows[r][first:first + rows]
            other.query_topk(rows, K, q.data_ptr(), kd.data_ptr(), init_keys=False)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(host_u64(kd).reshape(rows, K), fold(got, topk_keys(R[mine], R[og], k, K, gids=og)))
    finally:
        sh.close()


# ---- 5. routes: the through way ----------------------------------------------------------------------------------------------------
def test_the_grid_way_answers_with_the_flag_and_k_64_takes_the_self_scan():
    k, n, first, rows = 3, 16384, 5000, 200
    R = np.random.default_rng(7700).random((n, k), dtype=np.float32)
    R[5100] = R[5003]
    d = self_dist2(R, k, first, rows)
    r2 = float(np.sort(d[7][d[7] < np.inf])[5])
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for K, radius in ((8, INF), (63, INF), (8, r2)):
            got = stopk(ix, first, rows, K, radius, grid=True)
            assert ix.last_stats()[0] == 3, ix.last_stats()
            np.testing.assert_array_equal(got, self_topk(d, K, radius, base=BASE), err_msg=f"K={K} r2={radius}")
        # folding on the through way: into the keys a first call on other rows' behalf left (here: the same shard's, shifted)
        held = self_topk(self_dist2(R, k, first + 1000, rows), 8, base=BASE)
        got = stopk(ix, first, rows, 8, keys=dev_keys(rows, 8, fill=held), init=False, grid=True)
        assert ix.last_stats()[0] == 3
        np.testing.assert_array_equal(got, fold(held, self_topk(d, 8, base=BASE)))
        got = stopk(ix, first, rows, 64, grid=True)
        assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()
        np.testing.assert_array_equal(got, self_topk(d, 64, base=BASE))
        got = stopk(ix, first, rows, 8)            # without the flag: the plain call's route is the exact scan
        assert ix.last_stats()[0] == 1
        np.testing.assert_array_equal(got, self_topk(d, 8, base=BASE))
    finally:
        ix.close()


def test_the_cell_pruned_scan_answers_under_topk_cells_1():
    k, n, first, rows, K = 16, 1 << 17, 70000, 40, 8
    R = np.random.default_rng(7800).random((n, k), dtype=np.float32)
    for name, v in (("cells", 1), ("cells_rows", 1), ("cells_centre", 2)):
        pkg.set_option(name, v)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        pkg.set_option("topk_cells", 1)
        d = self_dist2(R, k, first, rows)
        got = stopk(ix, first, rows, K)
        assert ix.last_stats()[0] == 4, ix.last_stats()
        np.testing.assert_array_equal(got, self_topk(d, K, base=BASE))
        pkg.set_option("topk_cells", 2)
        pkg.set_option("path", 1)
        got = stopk(ix, first, rows, K)
        assert ix.last_stats() == [1, 0, 0, 0]
        np.testing.assert_array_equal(got, self_topk(d, K, base=BASE))
    finally:
        ix.close()


def test_the_filter_answers_under_path_2():
    """The dense filter, at the smallest shard for which the route hook gives way 2 for (K + 1 = 9 neighbours, 64 queries) under
    path 2: the route needs filter layouts, and knn_debug_index_build_plan says from which size the library builds them (k 40; under
    path 2 from the first row on, so the smallest shard is the call's own 64 rows)."""
    k, rows, K = 40, 64, 8

    def way(n):
        built = pkg.debug_index_build_plan(k=k, n_local=n, refs_on_device=0, build_filter=-1, build_grid=-1, path=2, cells=0, ingest=0,
                                           cells_build=0)["want_layouts"]
        return pkg.debug_query_route(k=k, K=K + 1, m=rows, n=n, topk_cells=0, has_cells=0, centred=0, rows_u8=0, bins=0, sharded=0,
                                     n_outliers=0, ncells=0, nitems=0, cap=0, several_slots=0, scan_blocks=0, scan_deal=0, num_cu=256,
                                     rec_cap=1 << 22, cells=0, path=2, filter_usable=built, has_grid=0, filter_wanted=built,
                                     init_keys=1)["way"]

    n = next(n for n in range(rows, 1 << 16) if way(n) == 2)   # (a call's rows are rows of the shard: n >= rows)
    assert n == rows or way(n - 1) != 2
    first = n - rows
    R = np.random.default_rng(7900).random((n, k), dtype=np.float32)
    pkg.set_option("path", 2)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        d = self_dist2(R, k, first, rows)
        got = stopk(ix, first, rows, K)
        assert ix.last_stats()[0] == 2, (n, ix.last_stats())
        np.testing.assert_array_equal(got, self_topk(d, K, base=BASE))
    finally:
        ix.close()


# ---- 6. the rest -------------------------------------------------------------------------------------------------------------------
def test_a_list_overflow_shows_in_the_cursor_and_nothing_is_stored_outside():
    k, first, rows = 16, 2090, 20
    R, _ = batch(k, 7950)
    d = self_dist2(R, k, first, rows)
    r2 = float(np.sort(d[0][d[0] < np.inf])[40])
    want = self_lists(d, r2, base=BASE)
    room = np.minimum(lengths(want), 3)               # too small for most
    assert (lengths(want) > room).any()
    off = offsets_of(room)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        total = int(off[rows])
        keys = dev_u64(np.full(total + 16, PAD))
        fill, got = slist(ix, first, rows, r2, off, keys=keys)
        np.testing.assert_array_equal(fill, lengths(want))          # the cursor counts every hit, stored or not
        assert (got[total:] == PAD).all()
        for j in range(rows):
            seg = got[int(off[j]):int(off[j + 1])]
            assert (seg != PAD).all() and np.isin(seg, want[j]).all() and np.unique(seg).size == seg.size
    finally:
        ix.close()


def test_slot_reuse_between_self_calls_and_plain_calls_and_the_range_rule():
    k, first, rows, K = 16, 100, 130, 8
    R, Q = batch(k, 7960)
    d = self_dist2(R, k, first, rows)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        q = torch.from_numpy(Q).to(dev())
        m = Q.shape[0]
        for slot in (0, 3, 0):
            np.testing.assert_array_equal(stopk(ix, first, rows, 64, slot=slot), self_topk(d, 64, base=BASE))
            pk = dev_keys(m, 3)
            ix.query_topk(m, 3, q.data_ptr(), pk.data_ptr(), init_keys=True, slot=slot)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(host_u64(pk).reshape(m, 3), topk_keys(Q, R, k, 3, base=BASE))
            np.testing.assert_array_equal(stopk(ix, first, rows, K, slot=slot), self_topk(d, K, base=BASE))
            np.testing.assert_array_equal(scount(ix, first, rows, 0.5, slot=slot), self_counts(d, 0.5))
        # row_first + rows above the shard's rows: the one rule that needs the index
        kd, cd = dev_keys(8, 8), dev_counts(8, fill=7)
        for call, who in ((lambda: ix.self_topk(N - 7, 8, 8, kd.data_ptr(), init_keys=True), "knn_index_self_topk"),
                          (lambda: ix.self_count_within(N, 1, 1.0, cd.data_ptr(), init=True), "knn_index_self_count_within"),
                          (lambda: ix.self_list_within(N - 1, 2, 1.0, kd.data_ptr(), cd.data_ptr(), kd.data_ptr(), init=True),
                           "knn_index_self_list_within")):
            with pytest.raises(pkg.KnnError, match=who + ": row_first \\+ rows above the shard's rows"):
                call()
        torch.cuda.synchronize()
        assert (host_u64(kd) == PAD).all() and (host_counts(cd) == 7).all()      # nothing was launched
        empty = pkg.KnnIndex(k, np.empty(0, dtype=np.float32), n_local=0, base_index=BASE)
        try:
            with pytest.raises(pkg.KnnError, match="row_first \\+ rows above the shard's rows"):
                empty.self_count_within(0, 1, 1.0, cd.data_ptr(), init=True)
        finally:
            empty.close()
    finally:
        ix.close()


def test_both_host_calls_give_the_graph_of_the_whole_shard():
    k, K = 16, 8
    R, _ = batch(k, 7970)
    d = self_dist2(R, k, 0, N)
    r2 = float(np.sort(d[100][d[100] < np.inf])[6])
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        want = self_topk(d, K, r2, base=BASE)
        ind, d2, counts = ix.self_topk_host(K, r2)
        np.testing.assert_array_equal(ind, keys_index(want))
        np.testing.assert_array_equal(d2.view(np.uint32), (want >> np.uint64(32)).astype(np.uint32))
        np.testing.assert_array_equal(counts, (want != KEY_INIT).sum(axis=1))
        lists = self_lists(d, r2, base=BASE)
        off, lind, ld2 = ix.self_list_within_host(r2)
        np.testing.assert_array_equal(off, offsets_of(lengths(lists)).astype(np.int64))
        flat = np.concatenate(lists)
        np.testing.assert_array_equal(lind, keys_index(flat))
        np.testing.assert_array_equal(ld2.view(np.uint32), (flat >> np.uint64(32)).astype(np.uint32))
        off0, ind0, _ = ix.self_list_within_host(0.0)     # rows TIE_A and TIE_B alone have a neighbour at distance 0
        assert int(off0[-1]) == 2 and sorted(ind0) == [TIE_A + BASE, TIE_B + BASE]
    finally:
        ix.close()
