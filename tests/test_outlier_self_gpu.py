"""The out-of-box launches of the routed self calls — knn_count_self_outlier_kernel and knn_list_self_outlier_kernel behind
knn_index_self_count_within_routed / knn_index_self_list_within_routed with KNN_QUERY_COUNT_CELLS — on the GPU against
tests/each_oracle.py over tests/self_oracle.self_dist2 and against the existing self calls, on the rows of tests/outlier_rows.py:
own rows that are themselves outside the filter's robust box, whose neighbours (a copy at distance 0 among them) are too.  Bar:
tests/test_self_routed_cells_gpu.py's — exact counts and sorted lists, the own row never listed, its copy listed first — and every
call that claims the out-of-box path asserts knn_index_last_stats(): [0] == 4, [2] == 0 (in a pass that fell back the kernels
return at their first line) and [3] == the planted rows."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests import outlier_rows as orow
from tests.count_helper import dev
from tests.each_helper import assert_segments, dev_f32
from tests.self_routed_helper import (LOW, assert_own_row_absent, assert_same_answer, existing_pipeline, routed_pipeline,
                                      segment_numbers)
from tests.shards_helper import Shards
from tests.test_within_cells_gpu import BINS, FP16, N17, OPTIONS
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
BASE = orow.BASE
ROWS = orow.WINDOW
CASES = [
    ("fp16_k16_fixed", 16, dict(FP16, scan_deal=1)),
    ("fp16_k16_counter", 16, dict(FP16, scan_deal=2)),
    ("bins_k16", 16, BINS),
    ("fp16_k8", 8, FP16),
]
assert N17 == orow.N17 and BASE == 11


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


def on_the_outlier_path(st, planted=orow.P):
    return st[0] == 4 and st[2] == 0 and st[3] == planted


def forms(r, cap, rows=ROWS):
    """(name, the device radii or None, the radii the oracle uses) of the scalar form (radii null: the cap) and the each form."""
    return (("scalar", None, np.full(rows, cap, np.float32)), ("each", dev_f32(r), r))


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_windows_inside_and_across_the_end_of_the_planted_block_are_exact_and_never_list_the_own_row(name, k, opts):
    R = orow.rows(k)
    a, b = orow.planted_range()
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for where, first in (("inside", orow.INSIDE_FIRST), ("straddling", orow.STRADDLE_FIRST)):
            d = orow.own_dist2(k, first, ROWS)
            r = eo.radii_of(d)
            cap = orow.kind_max(r, "held", eo.KINDS)
            own = first + np.arange(ROWS)
            for form, r_d, radii in forms(r, cap):
                msg = f"{name} {where} {form}"
                lists = eo.lists_of(d, radii, cap, base=BASE)
                got = routed_pipeline(ix, first, ROWS, cap, r_d, cells=True)
                assert all(on_the_outlier_path(st) for st in got[4]), (msg, got[4])
                assert_same_answer(got, lists, existing_pipeline(ix, first, ROWS, cap, r_d), msg=msg)
                assert_own_row_absent(got, BASE + own, msg=msg)
                hit = eo.hits_of(d, radii, cap)
                outside = orow.is_planted(own)
                # own rows outside the box: every hit is a planted row (the out-of-box launch's); inside: none is (the re-rank's)
                assert hit[outside].sum() > 0 and hit[outside].sum() == hit[outside, a:b].sum(), msg
                if where == "straddling":
                    assert hit[~outside].sum() > 0 and hit[~outside, a:b].sum() == 0, msg
                    assert (got[0][outside] > 0).any() and (got[0][~outside] > 0).any(), msg       # neither kind is dropped
                # the exact copy of a pair is listed first, at distance 0, and the own row (distance 0 too) is not
                seen = 0
                for c in orow.copy_rows():
                    j = c - first
                    if 0 <= j < ROWS and lists[j].size:
                        numbers, bits = segment_numbers(got, j)
                        assert numbers[0] == BASE + orow.twin_of(c) and bits[0] == 0, (msg, j, numbers[:3])
                        assert numbers.size == 1 or bits[1] != 0, (msg, j)
                        seen += 1
                assert seen >= 2, (msg, seen)
    finally:
        ix.close()


def test_two_passes_advance_the_own_row_of_the_out_of_box_launch():
    """rows = 1024 + 96 from TWO_PASS_FIRST: the second pass's own rows lie inside the planted block, so their own row is in the
    outlier list, at distance 0.  An out-of-box launch whose `first` stayed at the first pass's would drop a cluster row nobody
    lists and list every second-pass row's own row.  The oracle is evaluated for the first 64 rows and for the second pass."""
    k, first, m1, m2 = 8, orow.TWO_PASS_FIRST, orow.PASS, ROWS
    R = orow.rows(k)
    d1, d2 = orow.own_dist2(k, first, 64), orow.own_dist2(k, first + m1, m2)
    r1, r2 = eo.radii_of(d1), eo.radii_of(d2, first_kind=4)
    cap = max(orow.kind_max(r1, "held", eo.KINDS), orow.kind_max(r2, "held", eo.KINDS, 4))
    r = np.concatenate([np.tile(r1, m1 // 64), r2])        # (rows 64 .. 1023 under the first 64 rows' radii: cap bounds them)
    eo.assert_a_stale_pointer_fails(d2, r2, r[:m2], cap)
    assert orow.is_planted(first + m1 + np.arange(m2)).all()
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for form, rr, ra, rb in (("each", r, r1, r2), ("scalar", None, np.full(64, cap, np.float32), np.full(m2, cap, np.float32))):
            wa, wb = eo.lists_of(d1, ra, cap, base=BASE), eo.lists_of(d2, rb, cap, base=BASE)
            assert eo.lengths(wb).sum() > 0 and (eo.lengths(wb) == orow.planted_hits(d2, orow.bound_of(rb, cap))).all()
            r_d = dev_f32(rr) if rr is not None else None
            got = routed_pipeline(ix, first, m1 + m2, cap, r_d, cells=True)
            assert all(on_the_outlier_path(st) for st in got[4]), (form, got[4])
            counts, off, fill, keys = got[:4]
            np.testing.assert_array_equal(counts[:64], eo.lengths(wa), err_msg=form)
            np.testing.assert_array_equal(counts[m1:], eo.lengths(wb), err_msg=form)
            assert_segments(off, keys, wa, msg=f"{form} first pass")
            assert_segments(off[m1:], keys, wb, msg=f"{form} second pass")
            assert_same_answer(got, None, existing_pipeline(ix, first, m1 + m2, cap, r_d), msg=form)
            assert_own_row_absent(got, BASE + first + np.arange(m1 + m2), msg=form)
    finally:
        ix.close()


def test_a_cell_range_shard_lists_its_out_of_box_rows_by_gid_and_drops_by_local_row():
    """tests/test_self_routed_cells_gpu.py's shard test with rows outside the box: two cell-range shards of uniform rows, and 120
    pairs of exact copies in a small cloud at coordinate 0 = 1.7 .. 1.72.  The shards' frame is the geometry's — the sample's range
    widened, half-width about 0.53, so sigma 1 and a box of [-0.5, 1.5] — and no planted row is in the strided sample it is made
    from: they are outside, [3] > 0 on the rank that holds them (asserted).  The window holds one planted pair; its neighbours within
    the "held" radius are planted rows of the same rank, listed by gids[row], and the own row is dropped by LOCAL row."""
    k, rows = 16, 40
    n = (1 << 19) + 5
    rng = np.random.default_rng(7600)
    R = rng.random((n, k), dtype=np.float32)
    planted = 2001 + 4096 * np.arange(120)              # never a row of Shards' sample (every 128th)
    cloud = (0.45 + 0.1 * rng.random((120, k))).astype(np.float32)
    cloud[:, 0] = (1.7 + 0.02 * rng.random(120)).astype(np.float32)
    R[planted] = cloud
    R[planted + 1] = cloud
    every = np.concatenate([planted, planted + 1])
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=False)
    try:
        tested = 0
        for rank, ix in enumerate(sh.idx):
            gids = sh.gids[rank].cpu().numpy().astype(np.int64)
            mine = np.flatnonzero(np.isin(gids, planted))
            if mine.size == 0:
                continue
            tested += 1
            here = int(np.isin(gids, every).sum())
            p = int(mine[mine.size // 2])            # a planted row of this rank and, behind it, its copy
            assert gids[p + 1] == gids[p] + 1 and p > 64
            first = p - 9                            # the pair at window rows 9 ("held") and 10 ("below")
            window = gids[first:first + rows]
            assert not np.array_equal(window, np.arange(first, first + rows))   # a gid is not the local row number
            d = v0_dist2(R[window], R[gids], k)
            d[np.arange(rows), first + np.arange(rows)] = np.nan                # exclusion is by LOCAL row
            r = eo.radii_of(d)
            cap = orow.kind_max(r, "held", eo.KINDS)
            local_planted = np.isin(gids, every)
            for form, r_d, radii in forms(r, cap, rows):
                lists = eo.lists_of(d, radii, cap, gids=gids)
                hit = eo.hits_of(d, radii, cap)
                assert hit[9:11].sum() >= 4 and hit[9:11].sum() == hit[9:11][:, local_planted].sum()   # the pair's hits: planted rows
                got = routed_pipeline(ix, first, rows, cap, r_d, cells=True)
                assert all(st[0] == 4 and st[2] == 0 for st in got[4]), (rank, form, got[4])
                assert all(st[3] > 0 for st in got[4]), (rank, form, got[4])
                assert all(st[3] == here for st in got[4]), (rank, form, got[4], here)
                assert_same_answer(got, lists, existing_pipeline(ix, first, rows, cap, r_d), msg=f"rank {rank} {form}")
                assert_own_row_absent(got, window, msg=f"rank {rank} {form}")
                assert np.isin(got[3] & LOW, gids.astype(np.uint64)).all()
                for j, other in ((9, gids[p + 1]), (10, gids[p])):               # the copy in the same rank, at distance 0
                    numbers, bits = segment_numbers(got, j)
                    assert numbers[0] == other and bits[0] == 0, (rank, form, j, numbers[:3])
                    assert np.isin(numbers, every).all() and numbers.size >= 2, (rank, form, j)
        assert tested >= 1
    finally:
        sh.close()
