"""The exact slice scans across the boundary between two chunks of 65536 queries (csrc/knn_slice_launch.h), for the launchers no
other test takes there: the scalar count and list scans, the masked top-K and count, and the self top-K, count and list in
scalar form.  (The plain and large top-K, the masked lists, the each forms and the cluster sweeps have such a test of their own.)
The second chunk's launch starts at query 65536 with its own slices: queries, counts, offsets, cursors and keys all advance.

Query side: k 3, n 1100, m = 65536 + 70; the first chunk is 1024 copies of 64 queries (tests/test_each_exact_gpu.py's shape), so
the oracle is evaluated for 64 + 70 queries.  Self forms: rows 100 .. 100 + 65536 + 70 of n = 70000; the oracle runs on a few
hundred picked rows around both ends of both chunks.  Bar: equality with the oracle, bit for bit."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_oracle import counts_of
from tests.each_helper import assert_segments, dev_f32, pipeline
from tests.list_oracle import lengths, lists_of, offsets_of
from tests.self_oracle import self_counts, self_lists, self_topk
from tests.test_masked_gpu import masked, mcount, words_of
from tests.test_self_gpu import count_offsets_list_sort, stopk
from tests.topk_oracle import topk_keys, v0_dist2

pytestmark = pytest.mark.gpu
K_DIM, N, M1, M2, BASE = 3, 1100, 65536, 70, 11
R2 = 0.01          # a ball of ~0.4 % of the unit cube: a few hits per query, some queries with none


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


@functools.lru_cache(maxsize=None)
def queries():
    """R [N][3]; Q1 [64][3], Q2 [70][3]; Q = 1024 copies of Q1, then Q2; the two distance matrices."""
    rng = np.random.default_rng(6500)
    R = rng.random((N, K_DIM), dtype=np.float32)
    R[5, 0] = np.nan
    R[6, 2] = np.inf
    Q1, Q2 = rng.random((64, K_DIM), dtype=np.float32), rng.random((M2, K_DIM), dtype=np.float32)
    Q = np.concatenate([np.tile(Q1, (M1 // 64, 1)), Q2])
    d1, d2 = v0_dist2(Q1, R, K_DIM), v0_dist2(Q2, R, K_DIM)
    for a in (R, Q1, Q2, Q, d1, d2):
        a.setflags(write=False)
    return R, Q1, Q2, Q, d1, d2


def assert_two_chunks(got, w1, w2, msg):
    """got [M1 + M2][...] against the first chunk's 64 expected rows, repeated, and the second chunk's 70."""
    got = np.asarray(got)
    np.testing.assert_array_equal(got[:M1].reshape((M1 // 64, 64) + got.shape[1:]),
                                  np.broadcast_to(w1, (M1 // 64,) + np.asarray(w1).shape), err_msg=msg + ": first chunk")
    np.testing.assert_array_equal(got[M1:], w2, err_msg=msg + ": second chunk")


def test_scalar_count_and_list_scans():
    R, Q1, Q2, Q, d1, d2 = queries()
    w1, w2 = lists_of(d1, R2, base=BASE), lists_of(d2, R2, base=BASE)
    assert (lengths(w2) == 0).any() and (lengths(w2) > 1).any() and (lengths(w1) != lengths(w2)[:64]).any()
    m, q_d = M1 + M2, dev_f32(np.array(Q))                 # (a copy: the shared batch is read-only)
    ix = pkg.KnnIndex(K_DIM, R, base_index=BASE)
    try:
        counts, off, fill, keys, stats = pipeline(
            [ix], q_d, None, m,
            count=lambda ix, c, init: ix.count_within(m, q_d.data_ptr(), R2, c.data_ptr(), init=init),
            lst=lambda ix, o, f, kk, init: ix.list_within(m, q_d.data_ptr(), R2, o.data_ptr(), f.data_ptr(), kk.data_ptr(), init=init))
        assert all(st[0] == 1 for st in stats), stats
        assert_two_chunks(counts, counts_of(d1, R2), counts_of(d2, R2), "counts")
        np.testing.assert_array_equal(counts[M1:], lengths(w2))
        np.testing.assert_array_equal(fill, counts)
        np.testing.assert_array_equal(off, offsets_of(counts))
        assert_segments(off, keys, w1, msg="first chunk")
        assert_segments(off[M1 - 64:], keys, w1, msg="end of the first chunk")
        assert_segments(off[M1:], keys, w2, msg="second chunk")
    finally:
        ix.close()


def test_masked_topk_and_count():
    R, Q1, Q2, Q, d1, d2 = queries()
    K = 5
    half = np.random.default_rng(6501).random(N) < 0.5
    half[[5, 6]] = True                           # the rows without a finite distance stay admitted: they must not get in
    sel = np.flatnonzero(half)
    words = words_of(N, half)
    ix = pkg.KnnIndex(K_DIM, R, base_index=BASE)
    try:
        got = masked(ix, Q, K, float("inf"), words)
        assert ix.last_stats()[0] == 1, ix.last_stats()
        assert_two_chunks(got, topk_keys(Q1, R[sel], K_DIM, K, gids=sel + BASE), topk_keys(Q2, R[sel], K_DIM, K, gids=sel + BASE), "keys")
        c1, c2 = counts_of(d1[:, sel], R2), counts_of(d2[:, sel], R2)
        assert (c2 == 0).any() and (c2 > 1).any()
        assert_two_chunks(mcount(ix, Q, R2, words), c1, c2, "counts")
        assert ix.last_stats()[0] == 1, ix.last_stats()
    finally:
        ix.close()


def test_self_topk_count_and_list_in_scalar_form():
    k, n, first, rows, K = 3, 70000, 100, M1 + M2, 5
    r2 = 0.0009                                   # ~8 other rows within it
    R = np.random.default_rng(6502).random((n, k), dtype=np.float32)
    R[first + M1 + 3] = R[first + M1 - 2]         # a row of the second chunk and its copy in the first: nearest other rows at 0
    picked = np.unique(np.concatenate([np.arange(0, 70), np.arange(M1 - 70, M1 + 70), np.arange(rows - 70, rows),
                                       np.random.default_rng(6503).integers(0, rows, 40)]))
    assert {0, M1 - 1, M1, rows - 1} <= set(picked.tolist()) and 200 < picked.size < 400
    d = v0_dist2(R[first + picked], R, k)
    d[np.arange(picked.size), first + picked] = np.nan   # (tests/self_oracle.py's rule: a row never meets itself)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        got = stopk(ix, first, rows, K)
        assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()
        want = self_topk(d, K, base=BASE)
        np.testing.assert_array_equal(got[picked], want, err_msg="self top-K")
        assert want[picked.tolist().index(M1 + 3), 0] == np.uint64(first + M1 - 2 + BASE)   # (distance 0: the copy)
        counts, off, keys = count_offsets_list_sort(ix, first, rows, r2)
        assert ix.last_stats() == [1, 0, 0, 0], ix.last_stats()
        lists = self_lists(d, r2, base=BASE)
        np.testing.assert_array_equal(counts[picked], self_counts(d, r2), err_msg="self count")
        assert (counts[picked] > 1).any() and counts[picked].min() < counts[picked].max()
        np.testing.assert_array_equal(off, offsets_of(counts))
        for j, row in enumerate(picked):
            np.testing.assert_array_equal(keys[int(off[row]):int(off[row + 1])], lists[j], err_msg=f"self list of row {first + row}")
    finally:
        ix.close()
