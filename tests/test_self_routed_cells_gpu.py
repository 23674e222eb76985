"""knn_index_self_count_within_routed and knn_index_self_list_within_routed on the cell-pruned scan (KNN_QUERY_COUNT_CELLS) on the
GPU against tests/each_oracle.py over tests/self_oracle.self_dist2, and against the existing self calls.  Bar: exact counts and
sorted lists, the own row never listed, another copy of it listed at distance 0; "pruned" means knn_index_last_stats()[0] == 4,
[2] != 0 a pass that fell back and was answered by the gated self-scan."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.count_helper import dev, dev_counts, host_counts
from tests.each_helper import assert_segments, dev_f32
from tests.list_helper import PAD, dev_u64, host_u64
from tests.list_oracle import offsets_of
from tests.self_oracle import self_dist2
from tests.self_routed_helper import (LOW, assert_own_row_absent, assert_same_answer, existing_pipeline, plant_duplicates,
                                      routed_pipeline, segment_numbers)
from tests.shards_helper import Shards
from tests.test_within_cells_gpu import BINS, FP16, MATRIX, N17, OPTIONS
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
BASE = 11
FIRST, ROWS = 2090, 96            # a window that starts inside a block of 64 rows
INF = float("inf")
NIF = [c for c in MATRIX if c[0] == "nif_k20_fixed"][0]
CASES = [
    ("fp16_k16_fixed", 16, dict(FP16, scan_deal=1)),
    ("fp16_k16_counter", 16, dict(FP16, scan_deal=2)),
    ("bins_k16_fixed", 16, dict(BINS, scan_deal=1)),
    ("bins_k16_counter", 16, dict(BINS, scan_deal=2)),
    ("fp16_k8", 8, FP16),
    NIF,
]


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


def kind_max(r, kind):
    return float(r[eo.KINDS.index(kind)::len(eo.KINDS)].max())


@functools.lru_cache(maxsize=None)
def data(k):
    """The shard of a dimension, its window's distances, a radius of every kind per row and the largest list-sized one: made once."""
    rng = np.random.default_rng(N17 + 7 * k)
    R = rng.random((N17, k), dtype=np.float32)
    dup = plant_duplicates(R, FIRST)
    d = self_dist2(R, k, FIRST, ROWS)
    r = eo.radii_of(d)
    for a in (R, d):                                  # shared among the tests: left unchanged
        a.setflags(write=False)
    return R, d, r, kind_max(r, "held"), dup


def rcount(ix, first, rows, cap, r=None, counts=None, init=True, **flags):
    r_d = dev_f32(r) if r is not None else None
    if counts is None:
        counts = dev_counts(rows, fill=0xDEADBEEF if init else 0)
    torch.cuda.synchronize()
    ix.self_count_within_routed(first, rows, counts.data_ptr(), cap=cap, max_dist2_dev=r_d.data_ptr() if r is not None else None,
                                init=init, **flags)
    torch.cuda.synchronize()
    return host_counts(counts)


def rlist(ix, first, rows, cap, offsets, r=None, fill=None, keys=None, total=None, init=True, **flags):
    r_d = dev_f32(r) if r is not None else None
    off_d = dev_u64(offsets)
    if fill is None:
        fill = dev_counts(rows, fill=0xDEADBEEF if init else 0)
    if keys is None:
        keys = dev_u64(np.full(max(int(offsets[rows]) if total is None else total, 1), PAD))
    torch.cuda.synchronize()
    ix.self_list_within_routed(first, rows, off_d.data_ptr(), fill.data_ptr(), keys.data_ptr(), cap=cap,
                               max_dist2_dev=r_d.data_ptr() if r is not None else None, init=init, **flags)
    torch.cuda.synchronize()
    return host_counts(fill), host_u64(keys)


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_every_layout_and_kind_of_radius_is_exact_pruned_and_never_lists_the_own_row(name, k, opts):
    R, d, r, cap, (src, twin, outside) = data(k)
    eo.assert_every_kind_of_count(eo.counts_of(d, r))
    eo.assert_no_shared_radius_passes(d, r, cap)
    own = BASE + FIRST + np.arange(ROWS)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for form, rr in (("scalar", None), ("each", r)):
            radii = np.full(ROWS, cap, np.float32) if rr is None else rr
            lists = eo.lists_of(d, radii, cap, base=BASE)
            r_d = dev_f32(rr) if rr is not None else None
            got = routed_pipeline(ix, FIRST, ROWS, cap, r_d, cells=True)
            assert all(st[0] == 4 and st[2] == 0 for st in got[4]), (name, form, got[4])
            ref = existing_pipeline(ix, FIRST, ROWS, cap, r_d)
            assert_same_answer(got, lists, ref, msg=f"{name} {form}")
            assert_own_row_absent(got, own, msg=f"{name} {form}")
            # the planted copies: for both window rows the other two are listed first, at distance 0, the own row is not
            for j, others in ((src - FIRST, {twin, outside}), (twin - FIRST, {src, outside})):
                numbers, bits = segment_numbers(got, j)
                assert set(numbers[:2]) == {BASE + o for o in others} and (bits[:2] == 0).all(), (name, form, j, numbers[:4])
                if rr is not None:
                    assert numbers.size == 2, (name, j)         # a "zero" radius lists the copies alone
    finally:
        ix.close()


def test_two_passes_advance_the_own_row_with_the_queries():
    """rows = 1024 + 96 from row 1000: the second pass's own rows start at 2024.  The oracle is evaluated for the first 64 rows and
    for the second pass; a second pass that dropped row 1000 + j would list every row's own row (distance 0)."""
    k, first, m1, m2 = 8, 1000, 1024, 96
    rng = np.random.default_rng(49)
    R = rng.random((N17, k), dtype=np.float32)
    d1, d2 = self_dist2(R, k, first, 64), self_dist2(R, k, first + m1, m2)
    r1, r2 = eo.radii_of(d1), eo.radii_of(d2, first_kind=4)
    cap = max(kind_max(r1, "held"), float(r2[(0 - 4) % 9::9].max()))
    r = np.concatenate([np.tile(r1, m1 // 64), r2])        # (rows 64 .. 1023 under the first 64 rows' radii: cap bounds them)
    eo.assert_no_shared_radius_passes(d2, r2, cap)
    eo.assert_a_stale_pointer_fails(d2, r2, r[:m2], cap)
    w1, w2 = eo.lists_of(d1, r1, cap, base=BASE), eo.lists_of(d2, r2, cap, base=BASE)
    assert (eo.lengths(w2) == 0).any()                       # rows a stale own-row base would give a hit: themselves
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for form, rr, a, b in (("each", r, w1, w2),
                               ("scalar", None, eo.lists_of(d1, np.full(64, cap, np.float32), cap, base=BASE),
                                eo.lists_of(d2, np.full(m2, cap, np.float32), cap, base=BASE))):
            r_d = dev_f32(rr) if rr is not None else None
            got = routed_pipeline(ix, first, m1 + m2, cap, r_d, cells=True)
            assert all(st[0] == 4 and st[2] == 0 for st in got[4]), (form, got[4])
            counts, off, fill, keys = got[:4]
            np.testing.assert_array_equal(counts[:64], eo.lengths(a), err_msg=form)
            np.testing.assert_array_equal(counts[m1:], eo.lengths(b), err_msg=form)
            assert_segments(off, keys, a, msg=f"{form} first pass")
            assert_segments(off[m1:], keys, b, msg=f"{form} second pass")
            assert_same_answer(got, None, existing_pipeline(ix, first, m1 + m2, cap, r_d), msg=form)
            assert_own_row_absent(got, BASE + first + np.arange(m1 + m2), msg=form)
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [FP16, BINS], ids=["fp16", "bins"])
def test_a_far_row_and_a_nan_row_fall_back_to_the_self_scan_and_the_next_call_is_pruned_again(opts):
    k = 16
    R0, d0, r, cap, _ = data(k)
    R = R0.copy()
    far, bad = FIRST + 0, FIRST + 9          # both of kind "held": a radius with candidates, so nothing bounds the far row
    assert eo.KINDS[0] == "held" and eo.KINDS[9 % 9] == "held"
    R[far] = 1e6
    R[bad, 3] = np.nan
    d = self_dist2(R, k, FIRST, ROWS)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for form, rr in (("scalar", None), ("each", r)):
            radii = np.full(ROWS, cap, np.float32) if rr is None else rr
            lists = eo.lists_of(d, radii, cap, base=BASE)
            r_d = dev_f32(rr) if rr is not None else None
            got = routed_pipeline(ix, FIRST, ROWS, cap, r_d, cells=True)
            assert all(st[0] == 4 and st[2] != 0 for st in got[4]), (form, got[4])
            assert_same_answer(got, lists, existing_pipeline(ix, FIRST, ROWS, cap, r_d), msg=f"fell back, {form}")
            assert_own_row_absent(got, BASE + FIRST + np.arange(ROWS), msg=form)
            assert got[0][bad - FIRST] == 0 and got[0][far - FIRST] == 0
            assert (got[0] > 0).any()
        # a window without the two rows: pruned again
        first2 = FIRST + 3000 + 5
        got = routed_pipeline(ix, first2, ROWS, cap, None, cells=True)
        assert all(st[0] == 4 and st[2] == 0 for st in got[4]), got[4]
        assert_same_answer(got, None, existing_pipeline(ix, first2, ROWS, cap, None), msg="the next call")
    finally:
        ix.close()


def test_folding_overflow_and_the_route():
    k = 8
    R, d, r, cap, _ = data(k)
    lists = eo.lists_of(d, r, cap, base=BASE)
    want = eo.lengths(lists)
    assert (want > 1).any()
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        # a folding count adds
        held = np.arange(ROWS, dtype=np.uint32) * 5
        np.testing.assert_array_equal(rcount(ix, FIRST, ROWS, cap, r, counts=dev_counts(ROWS, fill=held), init=False, cells=True),
                                      held + want)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0
        # a folding list appends behind a non-zero fill
        f0 = (np.arange(ROWS) % 3).astype(np.uint32)
        off = offsets_of(want + f0)
        fill, keys = rlist(ix, FIRST, ROWS, cap, off, r, fill=dev_counts(ROWS, fill=f0), init=False, cells=True)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0
        np.testing.assert_array_equal(fill, f0 + want)
        for j in range(ROWS):
            seg = keys[int(off[j]):int(off[j + 1])]
            assert (seg[:f0[j]] == PAD).all(), j
            np.testing.assert_array_equal(np.sort(seg[f0[j]:]), lists[j], err_msg=str(j))
        # less room than hits: fill > room, nothing outside the segments, the guard words on both sides untouched
        room = np.where((np.arange(ROWS) % 4 == 0) & (want > 0), want - 1, want).astype(np.uint32)
        assert (room < want).any()
        guard = 3
        off = offsets_of(room) + np.uint64(guard)
        fill, keys = rlist(ix, FIRST, ROWS, cap, off, r, total=int(off[ROWS]) + guard, cells=True)
        np.testing.assert_array_equal(fill, want)
        assert (fill > room).any()
        assert (keys[:guard] == PAD).all() and (keys[int(off[ROWS]):] == PAD).all()
        for j in range(ROWS):
            seg = keys[int(off[j]):int(off[j + 1])]
            assert seg.size == room[j] and np.isin(seg, lists[j]).all() and np.unique(seg).size == seg.size, j
        # the route: without the flag, with 4 rows, with cap = +INF and under `cells` 2 the exact self-scan answers
        ref = existing_pipeline(ix, FIRST, ROWS, cap, dev_f32(r))
        got = routed_pipeline(ix, FIRST, ROWS, cap, dev_f32(r))
        assert all(st == [1, 0, 0, 0] for st in got[4]), got[4]
        assert_same_answer(got, lists, ref, msg="no flag")
        np.testing.assert_array_equal(rcount(ix, FIRST, 4, cap, r[:4], cells=True), want[:4])
        assert ix.last_stats()[0] == 1
        every = eo.counts_of(d, np.full(ROWS, np.inf, np.float32))
        np.testing.assert_array_equal(rcount(ix, FIRST, ROWS, INF, cells=True), every)
        assert ix.last_stats()[0] == 1 and (every == N17 - 1).all()
        pkg.set_option("cells", 2)
        np.testing.assert_array_equal(rcount(ix, FIRST, ROWS, cap, r, cells=True), want)
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


def test_a_cell_range_shard_carries_gids_and_drops_by_local_row():
    k, rows = 16, 40
    n = (1 << 19) + 5
    R = np.random.default_rng(7600).random((n, k), dtype=np.float32)
    planted = 2000 + 4099 * np.arange(120)
    R[planted + 1] = R[planted]                    # pairs of copies: one place, so one cell and one rank
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=False)
    try:
        for rank, ix in enumerate(sh.idx):
            gids = sh.gids[rank].cpu().numpy().astype(np.int64)
            mine = np.flatnonzero(np.isin(gids, planted))
            p = int(mine[mine.size // 2])            # a planted row of this rank and, behind it, its copy
            assert gids[p + 1] == gids[p] + 1 and p > 64
            first = p - 7
            window = gids[first:first + rows]
            assert not np.array_equal(window, np.arange(first, first + rows))   # a gid is not the local row number
            d = v0_dist2(R[window], R[gids], k)
            d[np.arange(rows), first + np.arange(rows)] = np.nan                # exclusion is by LOCAL row
            r = eo.radii_of(d)
            cap = kind_max(r, "held")
            for form, rr in (("scalar", None), ("each", r)):
                radii = np.full(rows, cap, np.float32) if rr is None else rr
                lists = eo.lists_of(d, radii, cap, gids=gids)
                r_d = dev_f32(rr) if rr is not None else None
                got = routed_pipeline(ix, first, rows, cap, r_d, cells=True)
                assert all(st[0] == 4 and st[2] == 0 for st in got[4]), (rank, form, got[4])
                assert_same_answer(got, lists, existing_pipeline(ix, first, rows, cap, r_d), msg=f"rank {rank} {form}")
                assert_own_row_absent(got, window, msg=f"rank {rank} {form}")
                assert np.isin(got[3] & LOW, gids.astype(np.uint64)).all()
                for j, other in ((7, gids[p + 1]), (8, gids[p])):               # the copy in the same rank, at distance 0
                    numbers, bits = segment_numbers(got, j)
                    assert numbers[0] == other and bits[0] == 0, (rank, form, j, numbers[:3])
    finally:
        sh.close()


def test_the_host_call_returns_the_radius_graph_of_the_whole_shard():
    k = 8
    R, d, _, _, _ = data(k)
    finite = np.sort(np.where(np.isnan(d), np.inf, d), axis=1)
    cap = float(np.median(finite[:, 2]))             # about three neighbours a row: a small radius
    lists = eo.lists_of(d[:64], np.full(64, cap, np.float32), cap, base=BASE)
    assert (eo.lengths(lists) > 0).any() and (eo.lengths(lists) == 0).any()
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        off, ind, d2 = ix.self_list_within_routed_host(cap, cells=True)
        assert ix.last_stats()[0] == 4, ix.last_stats()
        ref_off, ref_ind, ref_d2 = ix.self_list_within_host(cap)
        np.testing.assert_array_equal(off, ref_off)
        np.testing.assert_array_equal(ind, ref_ind)
        np.testing.assert_array_equal(d2.view(np.uint32), ref_d2.view(np.uint32))
        assert off[0] == 0 and off[-1] == ind.size == d2.size and off.size == N17 + 1
        for j in range(64):
            a, b = int(off[FIRST + j]), int(off[FIRST + j + 1])
            keys = (d2[a:b].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ind[a:b].astype(np.uint32).astype(np.uint64)
            np.testing.assert_array_equal(keys, lists[j], err_msg=str(j))
    finally:
        ix.close()
