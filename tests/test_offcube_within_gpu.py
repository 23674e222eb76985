"""knn_index_count_within, the pipeline count -> offsets -> knn_index_list_within -> sort, and knn_index_query_topk_within on the
cell-pruned scan (KNN_QUERY_COUNT_CELLS; way 4) off the unit cube: the batches of tests/offcube_rows.py — coordinates of 4096.x, rows
and queries on the cell cuts with radii that rows of several cells hold exactly, blobs, skewed cuts, per-dimension scales 2^10
apart, queries that are rows — at a radius some row holds exactly, the next float below it, 0 and (where rows have copies) the
smallest subnormal.  Against tests/count_oracle.py, tests/list_oracle.py and the K smallest of the oracle's lists clipped at the
radius.  Bar: exact counts, lists exact as sorted segments, fill == counts, keys carry base_index, bit-exact top-K keys;
knn_index_last_stats()[0] == 4 at every call, [2] == 0 (no pass fell back) on uniform and offset rows, printed for the others."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import offcube_rows as oc
from tests.count_helper import count
from tests.count_oracle import counts_of
from tests.each_helper import assert_segments, dev_f32
from tests.list_oracle import lengths, lists_of
from tests.offcube_helper import OPTIONS, assert_base_carried, check_stats, index_on_way_4, scalar_pipeline
from tests.self_oracle import self_topk
from tests.within_helper import clip, within

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


@pytest.mark.parametrize("name,layout", oc.PAIRS, ids=oc.PAIR_IDS)
def test_counts_lists_and_top_k_within_are_exact_on_the_pruned_way(name, layout):
    lname, k, _ = layout
    _, Q, d = oc.batch(name, k)
    Q = Q.copy()                # (read-only as handed out: torch wants a writable array)
    _, dn, gids = oc.near(name, k)
    with index_on_way_4(name, layout, topk_cells=True) as ix:
        q_d = dev_f32(Q)
        for rname, r2 in oc.radii(name, k):
            want = lists_of(dn, r2, gids=gids)
            np.testing.assert_array_equal(lengths(want), counts_of(d, r2))
            print(f"offcube {name} {lname}: radius {rname} = {r2!r}, largest count {lengths(want).max()}")
            got = count(ix, Q, r2, cells=True)
            check_stats(ix.last_stats(), name, lname, f"count {rname}")
            np.testing.assert_array_equal(got, lengths(want), err_msg=f"{name} {lname} {rname} r2={r2!r}")
            counts, off, fill, keys, stats = scalar_pipeline(ix, q_d, oc.M, r2, cells=True)
            check_stats(stats, name, lname, f"count+list {rname}")
            np.testing.assert_array_equal(counts, lengths(want), err_msg=f"{name} {lname} {rname} counts")
            np.testing.assert_array_equal(fill, counts, err_msg=f"{name} {lname} {rname} fill")
            assert_segments(off, keys, want, msg=f"{name} {lname} {rname} r2={r2!r}")
            assert_base_carried(keys, (name, lname, rname))
        rs = dict(oc.radii(name, k))
        for K in (8, 64):
            for rname in ("at", "below"):
                want = clip(self_topk(dn, K, r2=rs[rname], gids=gids), rs[rname])
                got = within(ix, Q, K, rs[rname])
                check_stats(ix.last_stats(), name, lname, f"top-{K} within {rname}")
                np.testing.assert_array_equal(got, want, err_msg=f"{name} {lname} K={K} {rname} r2={rs[rname]!r}")
