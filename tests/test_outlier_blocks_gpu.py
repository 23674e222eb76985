"""More than one block and one wave of the scalar out-of-box kernels — knn_count_outlier_kernel, knn_list_outlier_kernel
(knn_index_count_within / knn_index_list_within with KNN_QUERY_COUNT_CELLS) and knn_topk_outlier_kernel (top-K under `topk_cells`
1) — on the GPU against tests/count_oracle.py, tests/list_oracle.py and tests/topk_oracle.py, on the rows of tests/outlier_rows.py:
640 out-of-box rows are 3 blocks of 256 and 10 waves per query, and queries in the middle of them hold 300 and more within one
radius — so several waves of several blocks add to one query's count and race for one list cursor, on the fp16 and on the bin-frame
8-bit layout, at base_index 11.  Every call asserts knn_index_last_stats(): [0] == 4, [2] == 0, [3] == 640."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import outlier_rows as orow
from tests.count_helper import count, dev_counts
from tests.count_oracle import counts_of
from tests.list_helper import check_list
from tests.list_oracle import lengths, lists_of
from tests.test_cells_topk_gpu import _topk
from tests.test_within_cells_gpu import BINS, FP16, N17, OPTIONS
from tests.topk_oracle import keys_index, topk_keys

pytestmark = pytest.mark.gpu
BASE = orow.BASE
CASES = [("fp16_k16", 16, FP16), ("bins_k16", 16, BINS), ("fp16_k8", 8, FP16)]
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


def radii_of(k):
    """The radii of the count and list tests, from the oracle: the one that holds half the planted block for query 0 (and no
    cluster row for any query), the next float below it, query 0's 70th nearest distance (two waves' worth) and its nearest."""
    _, d = orow.centre_batch(k)
    big = orow.blocks_radius(k)
    near = np.sort(d[0])
    assert orow.planted_hits(d, big).max() >= 300 and (counts_of(d, big) == orow.planted_hits(d, big)).all()
    assert (counts_of(d, big) == 0).any() and ((counts_of(d, big) > 0) & (counts_of(d, big) < 64)).any()
    return [("half_the_block", big), ("below", float(np.nextafter(np.float32(big), np.float32(0)))), ("seventy", float(near[69])),
            ("nearest", float(near[0]))]


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_counts_add_up_over_the_blocks_and_waves_of_one_query(name, k, opts):
    Q, d = orow.centre_batch(k)
    m = Q.shape[0]
    _set(opts)
    ix = pkg.KnnIndex(k, orow.rows(k), base_index=BASE)
    try:
        for rname, r2 in radii_of(k):
            want = counts_of(d, r2)
            got = count(ix, Q, r2, cells=True)
            assert on_the_outlier_path(ix.last_stats()), (name, rname, ix.last_stats())
            np.testing.assert_array_equal(got, want, err_msg=f"{name} {rname} r2={r2}")
            held = np.arange(m, dtype=np.uint32) * 7
            got = count(ix, Q, r2, counts=dev_counts(m, fill=held), init=False, cells=True)
            assert on_the_outlier_path(ix.last_stats()), (name, rname, ix.last_stats())
            np.testing.assert_array_equal(got, held + want, err_msg=f"{name} {rname} folded")
    finally:
        ix.close()


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_lists_hold_every_hit_once_when_blocks_race_for_one_cursor(name, k, opts):
    Q, d = orow.centre_batch(k)
    _set(opts)
    ix = pkg.KnnIndex(k, orow.rows(k), base_index=BASE)
    try:
        for rname, r2 in radii_of(k):
            want = lists_of(d, r2, base=BASE)
            assert rname not in ("half_the_block", "below") or lengths(want).max() >= 300
            check_list(ix, Q, r2, want, msg=f"{name} {rname} r2={r2}", cells=True)
            assert on_the_outlier_path(ix.last_stats()), (name, rname, ix.last_stats())
    finally:
        ix.close()


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_top_k_takes_its_keys_from_every_block_of_out_of_box_rows(name, k, opts):
    """The K nearest of the queries in the middle of the planted block are planted rows (the cluster is 0.86 away), spread over the
    whole outlier list: K = 8 and K = 64.  640 rows are at most half a query's candidate room, so the call stays on the cell way."""
    Q, _ = orow.centre_batch(k)
    R = orow.rows(k)
    want = topk_keys(Q, R, k, 64, base=BASE)
    assert orow.is_planted(keys_index(want) - BASE).all()
    # (the 64 nearest of query 0 come from more than one block's worth of any order of the list: they span the block)
    span = keys_index(want[0]) - BASE
    assert span.max() - span.min() > 256
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for K in (8, 64):
            got = _topk(ix, Q, K)
            assert on_the_outlier_path(ix.last_stats()), (name, K, ix.last_stats())
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{name} K={K}")
    finally:
        ix.close()
