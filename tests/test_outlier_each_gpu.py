"""The out-of-box launches of the calls with a radius per query — knn_count_each_outlier_kernel and knn_list_each_outlier_kernel
behind knn_index_count_within_each / knn_index_list_within_each with KNN_QUERY_COUNT_CELLS — on the GPU against tests/each_oracle.py,
on the rows of tests/outlier_rows.py: 640 rows outside the filter's robust box (3 blocks, 10 waves of the kernels), and queries
whose hits are such rows alone.  Bar: tests/test_each_cells_gpu.py's — exact counts, lists equal as sorted key arrays, fill ==
counts — and every call that claims the out-of-box path asserts knn_index_last_stats(): [0] == 4 (pruned), [2] == 0 (no pass fell
back: the kernels return at their first line in one that did) and [3] == 640 (the rows are where the filter lists them)."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests import outlier_rows as orow
from tests.count_helper import dev_counts
from tests.each_helper import assert_segments, count_each, dev_f32, list_each, pipeline
from tests.list_helper import PAD, dev_u64
from tests.list_oracle import offsets_of
from tests.test_within_cells_gpu import BINS, FP16, N17, OPTIONS

pytestmark = pytest.mark.gpu
BASE = orow.BASE
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


def on_the_outlier_path(st):
    return st[0] == 4 and st[2] == 0 and st[3] == orow.P


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_both_caps_folds_and_overflow_are_exact_with_hits_from_the_out_of_box_rows(name, k, opts):
    m = orow.M_EACH
    R = orow.rows(k)
    Q, d = orow.each_batch(k)
    r = eo.radii_of(d)
    cap_held, cap_low = orow.kind_max(r, "held", eo.KINDS), orow.low_cap(r)
    beside = np.arange(orow.M_BESIDE)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        # the cap at the largest "held" radius (radii[q] decides), then below some queries' radii (acc <= cap decides)
        for cap in (cap_held, cap_low):
            lists = eo.lists_of(d, r, cap, base=BASE)
            counts, off, fill, keys, stats = pipeline([ix], dev_f32(Q), dev_f32(r), m, cap=cap, cells=True)
            assert all(on_the_outlier_path(st) for st in stats), (name, cap, stats)
            np.testing.assert_array_equal(counts, eo.lengths(lists), err_msg=f"{name} cap={cap}")
            np.testing.assert_array_equal(fill, counts)
            assert_segments(off, keys, lists, msg=f"{name} cap={cap}")
        cap = cap_held
        lists = eo.lists_of(d, r, cap, base=BASE)
        want = eo.lengths(lists)
        assert (want[beside] == orow.planted_hits(d, orow.bound_of(r, cap))[beside]).all()   # beside: out-of-box hits alone
        # a fold adds to held counts
        held = np.arange(m, dtype=np.uint32) * 5
        np.testing.assert_array_equal(count_each(ix, Q, r, cap=cap, counts=dev_counts(m, fill=held), init=False, cells=True), held + want)
        assert on_the_outlier_path(ix.last_stats()), ix.last_stats()
        # a list behind a non-zero fill appends
        f0 = (np.arange(m) % 3).astype(np.uint32)
        off = offsets_of(want + f0)
        fill, keys = list_each(ix, Q, r, off, cap=cap, fill=dev_counts(m, fill=f0), init=False, cells=True)
        assert on_the_outlier_path(ix.last_stats()), ix.last_stats()
        np.testing.assert_array_equal(fill, f0 + want)
        for j in range(m):
            seg = keys[int(off[j]):int(off[j + 1])]
            assert (seg[:f0[j]] == PAD).all(), j
            np.testing.assert_array_equal(np.sort(seg[f0[j]:]), lists[j], err_msg=f"{name} appended, query {j}")
        # less room than hits for queries whose hits are all out-of-box rows: fill > room, nothing outside the segment, guards untouched
        short = (np.arange(m) % 4 == 0) & (want > 0)
        assert short[beside].any()
        room = np.where(short, want - 1, want).astype(np.uint32)
        guard = 3
        off = offsets_of(room) + np.uint64(guard)
        fill, keys = list_each(ix, Q, r, off, cap=cap, keys=dev_u64(np.full(int(off[m]) + guard, PAD)), cells=True)
        assert on_the_outlier_path(ix.last_stats()), ix.last_stats()
        np.testing.assert_array_equal(fill, want)
        assert (fill[short] > room[short]).all()
        assert (keys[:guard] == PAD).all() and (keys[int(off[m]):] == PAD).all()
        for j in range(m):
            seg = keys[int(off[j]):int(off[j + 1])]
            assert seg.size == room[j] and np.isin(seg, lists[j]).all() and np.unique(seg).size == seg.size, (name, j)
    finally:
        ix.close()


def test_two_passes_advance_the_radii_of_the_out_of_box_launch():
    """m = 1024 + 96: the first pass's queries are 16 copies of 64 (32 beside planted rows, 32 in the cluster), the second pass's 96
    all sit beside planted rows and their kinds start elsewhere in the cycle: an out-of-box launch that read the first pass's radii
    in the second would count differently (tests.each_oracle.assert_a_stale_pointer_fails)."""
    k, m1, m2 = 8, orow.PASS, 96
    R = orow.rows(k)
    Q1, d1, Q2, d2 = orow.two_pass_batches(k)
    r1, r2 = eo.radii_of(d1), eo.radii_of(d2, first_kind=4)
    cap = max(orow.kind_max(r1, "held", eo.KINDS), orow.kind_max(r2, "held", eo.KINDS, 4))
    Q = np.concatenate([np.tile(Q1, (m1 // 64, 1)), Q2])
    r = np.concatenate([np.tile(r1, m1 // 64), r2])
    eo.assert_a_stale_pointer_fails(d2, r2, r[:m2], cap)
    w1, w2 = eo.lists_of(d1, r1, cap, base=BASE), eo.lists_of(d2, r2, cap, base=BASE)
    assert (eo.lengths(w2) == orow.planted_hits(d2, orow.bound_of(r2, cap))).all() and eo.lengths(w2).sum() > 0
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        counts, off, fill, keys, stats = pipeline([ix], dev_f32(Q), dev_f32(r), m1 + m2, cap=cap, cells=True)
        assert all(on_the_outlier_path(st) for st in stats), stats
        np.testing.assert_array_equal(counts[:m1].reshape(-1, 64), np.tile(eo.lengths(w1), (m1 // 64, 1)))
        np.testing.assert_array_equal(counts[m1:], eo.lengths(w2))
        np.testing.assert_array_equal(fill, counts)
        assert_segments(off, keys, w1, msg="first pass")
        assert_segments(off[m1:], keys, w2, msg="second pass")
    finally:
        ix.close()
