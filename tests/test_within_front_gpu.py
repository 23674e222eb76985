"""The one call front of the radius family (knn_api.cpp: within_check, within_begin, within_run) on the GPU: what every one of the
twelve device entry points leaves behind besides its answer — the timing bracket (knn_index_timing_read: one bracketed launch per
timed call on every way, as the commit before the front reported, never two records of an event) and knn_index_last_stats()[0],
the way: 1 the exact scans, 3 the grid index, 4 the cell-pruned scan.  And the empty shard: an init call zeroes the counts and
returns, a self call fails its range check.  No result values here: tests/test_count_*_gpu.py, test_list_*_gpu.py,
test_each_*_gpu.py, test_self_gpu.py, test_self_routed_*_gpu.py, test_masked_gpu.py and test_masked_lists_gpu.py check those
against their oracles."""
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.count_helper import dev_counts, host_counts
from tests.each_helper import dev_f32
from tests.list_helper import PAD, dev_u64
from tests.list_oracle import offsets_of
from tests.self_oracle import self_dist2
from tests.test_self_routed_cells_gpu import data as cells_data, kind_max
from tests.test_self_routed_grid_gpu import FIRST, N, ROWS
from tests.test_within_cells_gpu import FP16, OPTIONS

pytestmark = pytest.mark.gpu
LAUNCHES = 1      # bracketed launches of one timed call, every entry and every way: what the commit before the front reports
ENTRIES = ("count_within", "list_within", "count_within_each", "list_within_each", "count_within_masked", "list_within_masked",
           "self_count_within", "self_list_within", "self_count_within_each", "self_list_within_each", "self_count_within_routed",
           "self_list_within_routed")
ROUTABLE = tuple(e for e in ENTRIES if e.startswith(("count_within", "list_within")) and not e.endswith("masked")) + ENTRIES[-2:]


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


@functools.lru_cache(maxsize=None)
def grid_rows():
    R = np.random.default_rng(8103).random((N, 3), dtype=np.float32)
    R.setflags(write=False)
    return R


def window(R, k):
    """The window's per-row radii of every kind, the list-sized cap (the largest "held" radius) and segments with room for every
    entry's hits at that cap: the other rows within it and the row itself."""
    d = self_dist2(R, k, FIRST, ROWS)
    r = eo.radii_of(d)
    cap = kind_max(r, "held")
    return r, cap, offsets_of(eo.counts_of(d, np.full(ROWS, cap, np.float32), cap) + np.uint32(1))


def issue(ix, entry, R, r, cap, off, **flags):
    """One init call of `entry` about the window — its rows as the queries of the plain entries — at `cap`."""
    q, r_d, mask = dev_f32(R[FIRST:FIRST + ROWS].copy()), dev_f32(r), dev_counts(pkg.mask_words(R.shape[0]), fill=0xFFFFFFFF)
    counts, fill = dev_counts(ROWS, fill=0xDEADBEEF), dev_counts(ROWS, fill=0xDEADBEEF)
    off_d, keys = dev_u64(off), dev_u64(np.full(max(int(off[ROWS]), 1), PAD))
    lists = (off_d.data_ptr(), fill.data_ptr(), keys.data_ptr())
    torch.cuda.synchronize()
    if entry == "count_within":
        ix.count_within(ROWS, q.data_ptr(), cap, counts.data_ptr(), init=True, **flags)
    elif entry == "list_within":
        ix.list_within(ROWS, q.data_ptr(), cap, *lists, init=True, **flags)
    elif entry == "count_within_each":
        ix.count_within_each(ROWS, q.data_ptr(), r_d.data_ptr(), counts.data_ptr(), cap=cap, init=True, **flags)
    elif entry == "list_within_each":
        ix.list_within_each(ROWS, q.data_ptr(), r_d.data_ptr(), *lists, cap=cap, init=True, **flags)
    elif entry == "count_within_masked":
        ix.count_within_masked(ROWS, q.data_ptr(), cap, mask.data_ptr(), counts.data_ptr(), init=True)
    elif entry == "list_within_masked":
        ix.list_within_masked(ROWS, q.data_ptr(), cap, mask.data_ptr(), *lists, init=True)
    elif entry == "self_count_within":
        ix.self_count_within(FIRST, ROWS, cap, counts.data_ptr(), init=True)
    elif entry == "self_list_within":
        ix.self_list_within(FIRST, ROWS, cap, *lists, init=True)
    elif entry == "self_count_within_each":
        ix.self_count_within_each(FIRST, ROWS, r_d.data_ptr(), counts.data_ptr(), cap=cap, init=True)
    elif entry == "self_list_within_each":
        ix.self_list_within_each(FIRST, ROWS, r_d.data_ptr(), *lists, cap=cap, init=True)
    elif entry == "self_count_within_routed":
        ix.self_count_within_routed(FIRST, ROWS, counts.data_ptr(), cap=cap, max_dist2_dev=r_d.data_ptr(), init=True, **flags)
    else:
        assert entry == "self_list_within_routed"
        ix.self_list_within_routed(FIRST, ROWS, *lists, cap=cap, max_dist2_dev=r_d.data_ptr(), init=True, **flags)
    torch.cuda.synchronize()


def check_bracket_and_way(ix, R, flag, way):
    r, cap, off = window(R, ix.k)
    ix.timing(1)
    try:
        for entry, flags, want in [(e, {}, 1) for e in ENTRIES] + [(e, {flag: True}, way) for e in ROUTABLE]:
            issue(ix, entry, R, r, cap, off, **flags)
            launches, total_ms = ix.timing_read()
            print(f"{entry} {flags}: {launches} bracketed launches, {total_ms:.4f} ms, last_stats {ix.last_stats()}")
            assert launches == LAUNCHES, (entry, flags, launches)
            assert math.isfinite(total_ms) and total_ms > 0, (entry, flags, total_ms)
            assert ix.last_stats()[0] == want, (entry, flags, ix.last_stats())
    finally:
        ix.timing(0)


def test_every_entry_brackets_one_launch_and_reports_its_way_on_the_exact_and_grid_ways():
    R = grid_rows()
    ix = pkg.KnnIndex(3, R)
    try:
        check_bracket_and_way(ix, R, "grid", 3)
    finally:
        ix.close()


def test_every_entry_brackets_one_launch_and_reports_its_way_on_the_exact_and_cell_ways():
    R = cells_data(8)[0]
    for o, v in FP16.items():
        pkg.set_option(o, v)
    ix = pkg.KnnIndex(8, R)
    try:
        check_bracket_and_way(ix, R, "cells", 4)
    finally:
        ix.close()


def test_an_empty_shard_zeroes_an_init_count_and_fails_a_self_call_on_its_range():
    k, m = 3, 5
    ix = pkg.KnnIndex(k, np.zeros((0, k), np.float32))
    try:
        q, counts = dev_f32(np.zeros((m, k), np.float32)), dev_counts(m, fill=0xDEADBEEF)
        torch.cuda.synchronize()
        ix.count_within(m, q.data_ptr(), 1.0, counts.data_ptr(), init=True)
        torch.cuda.synchronize()
        assert (host_counts(counts) == 0).all() and ix.last_stats()[0] == 1
        with pytest.raises(pkg.KnnError, match="knn_index_self_count_within: row_first \\+ rows above the shard's rows"):
            ix.self_count_within(0, 1, 1.0, counts.data_ptr(), init=True)
        assert (host_counts(counts) == 0).all()
    finally:
        ix.close()
