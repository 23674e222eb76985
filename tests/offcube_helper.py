"""The radius family off the unit cube — what its GPU tests share (test infrastructure): one index per (distribution, layout) with
the 1-NN call that says whether the build took the cell-sorted layout, the scalar pipeline count -> offsets -> list -> sort, and
the checks every call's knn_index_last_stats() gets.  Rows, radii and masks come from tests/offcube_rows.py, expectations from the
suite's numpy oracles."""
import contextlib

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import offcube_rows as oc
from tests.count_helper import dev
from tests.each_helper import dev_f32, pipeline

OPTIONS = ("path", "cells", "cells_rows", "cells_centre", "cells_u8_frame", "scan_deal", "topk_cells")
GATED = ("uniform", "offset")       # the distributions whose passes must not fall back ([2] == 0); the others' [2] is printed
MAX_SKIPPED = 4
_declined = {}                      # (distribution, layout) -> the 1-NN call's stats, for the pairs whose build declined the layout


@contextlib.contextmanager
def index_on_way_4(name, layout, topk_cells=False):
    """The index of a (distribution, layout) pair, base_index oc.BASE, after a 1-NN query_keys call of the batch on it: exact, and
    on way 4 — or the test is skipped with the call's stats as the reason (at most MAX_SKIPPED pairs, none of oc.NEVER_SKIPPED)."""
    lname, k, opts = layout
    R, Q, d = oc.batch(name, k)
    for o, v in opts.items():
        pkg.set_option(o, v)
    if topk_cells:
        pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=oc.BASE)
    try:
        keys = torch.empty(oc.M, dtype=torch.int64, device=dev())
        q_d = dev_f32(Q.copy())
        ix.query_keys(oc.M, q_d.data_ptr(), keys.data_ptr(), init_keys=True)
        torch.cuda.synchronize()
        st = ix.last_stats()
        row = np.argmin(d, axis=1)              # (the lowest row of the smallest distance: v0's answer; no distance here is NaN)
        want = (d[np.arange(oc.M), row].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (row + oc.BASE).astype(np.uint64)
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), want, err_msg=f"{name} {lname} 1-NN, stats {st}")
        if st[0] != 4:
            assert (name, lname) not in oc.NEVER_SKIPPED, (name, lname, st)
            _declined[(name, lname)] = st
            assert len(_declined) <= MAX_SKIPPED, _declined
            print(f"offcube {name} {lname}: SKIPPED, the build declined the cell-sorted layout: 1-NN last_stats {st}")
            pytest.skip(f"{name} on {lname}: the build declined the cell-sorted layout (1-NN last_stats {st})")
        yield ix
    finally:
        ix.close()


def check_stats(stats, name, lname, form):
    """Every call of a test: answered on way 4 (a pass that fell back is answered exactly under that way, and the next call is on
    it again); no pass of a GATED distribution fell back.  stats: one last_stats() or a list of them."""
    stats = [stats] if stats and not isinstance(stats[0], (list, tuple)) else stats
    print(f"offcube {name} {lname} {form}: last_stats {stats}")
    for st in stats:
        assert st[0] == 4, (name, lname, form, stats)
        if name in GATED:
            assert st[2] == 0, (name, lname, form, stats)


def scalar_pipeline(ix, q_d, m, r2, **flags):
    """(counts, offsets, fill, sorted keys, the stats after both calls) of count_within -> counts_to_offsets -> list_within ->
    keys_sort_segments at the scalar radius r2."""
    def count(ix, counts, init):
        ix.count_within(m, q_d.data_ptr(), r2, counts.data_ptr(), init=init, **flags)

    def lst(ix, off, fill, keys, init):
        ix.list_within(m, q_d.data_ptr(), r2, off.data_ptr(), fill.data_ptr(), keys.data_ptr(), init=init, **flags)

    return pipeline([ix], None, None, m, count=count, lst=lst)


def assert_base_carried(keys, k):
    """Every listed key's low word is a row number of the shard plus the non-zero base_index."""
    numbers = (np.asarray(keys, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert oc.BASE > 0 and ((numbers >= oc.BASE) & (numbers < oc.BASE + oc.N17)).all(), k
