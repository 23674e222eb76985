"""Radius-bounded top-K on the cell-pruned scan and on the ways that clip behind (knn_index_query_topk_within; DESIGN §4.6,
"Within a radius") on the GPU against the numpy restatement of v0 (tests/topk_oracle.py), clipped at the radius.  Bar: bit-exact
keys at every radius; "pruned" means knn_index_last_stats()[0] == 4, [2] != 0 a pass that fell back."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.shards_helper import Shards
from tests.topk_oracle import KEY_INIT, keys_dist2, topk_keys
from tests.within_helper import KS, clip, dev, dev_keys, host_keys, plain, radii, within

pytestmark = pytest.mark.gpu
OPTIONS = ("path", "cells", "cells_rows", "cells_centre", "cells_u8_frame", "scan_deal", "topk_cells")
N17 = (1 << 17) + 999          # the smallest shard that gets a cell-sorted layout under `cells` 1: 512 cells
FP16 = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2}
BINS = {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 2}
CENTRED = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 1}
DENSE = {"path": 2, "cells": 2}
# the one-frame layouts of tests/test_cells_topk_gpu.py's matrix the radius form of the prep kernel serves (PW x KT, both deals)
MATRIX = [
    ("fp16_k16_fixed", 16, dict(FP16, scan_deal=1)),
    ("fp16_k16_counter", 16, dict(FP16, scan_deal=2)),
    ("bins_k16", 16, BINS),
    ("nif_k20_fixed", 20, dict(FP16, scan_deal=1)),
    ("nif_k20_counter", 20, dict(FP16, scan_deal=2)),
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


def spread_queries(rng, m, k, reach=0.6):
    """Queries inside the rows' unit box and, one after the other, up to `reach` outside it along the first axis: their nearest
    distances span a range, so one radius leaves some lists full, some short and some empty."""
    Q = rng.random((m, k), dtype=np.float32)
    Q[:, 0] += np.linspace(0.0, reach, m, dtype=np.float32)
    return Q


@pytest.mark.parametrize("name,k,opts", MATRIX, ids=[c[0] for c in MATRIX])
def test_every_radius_is_bit_exact_pruned_and_a_small_radius_lists_less(name, k, opts):
    rng = np.random.default_rng(N17 + 7 * k)
    m = 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=11)
    try:
        want64 = topk_keys(Q, R, k, 64, base=11)
        for K in KS:
            want = want64[:, :K]
            for rname, r2 in radii(want):
                got = within(ix, Q, K, r2)
                st = ix.last_stats()
                assert st[0] == 4 and st[2] == 0, (name, K, rname, st)
                np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"{name} K={K} {rname} r2={r2}")
            np.testing.assert_array_equal(within(ix, Q, K, float("inf")), plain(ix, Q, K))
        # K = 64 under the batch's median 1-NN distance: the radius, not the 64-th seed score, bounds the candidates
        np.testing.assert_array_equal(plain(ix, Q, 64), want64)
        records_plain = ix.last_stats()[1]
        r2 = float(np.median(keys_dist2(want64[:, 0])))
        np.testing.assert_array_equal(within(ix, Q, 64, r2), clip(want64, r2))
        st = ix.last_stats()
        print(f"{name}: records re-ranked at K 64: plain {records_plain}, within the median 1-NN distance {st[1]}")
        assert st[0] == 4 and st[2] == 0 and st[1] < records_plain, (name, st, records_plain)
    finally:
        ix.close()


def test_fewer_real_rows_than_k_near_the_query_is_bounded_by_the_radius():
    """The data of test_empty_corner_query_and_fewer_real_rows_than_k (tests/test_cells_topk_gpu.py): a clustered set and queries
    in an empty corner, K = 64.  With a finite radius every query has a bound — the radius — and the pass does not fall back.
    (On an MI355X the plain call does not fall back on this batch either — its wide sample finds 64 rows: last_stats
    [4, 19874, 0, 51] — so what the radius shows here is the record count: it must not exceed the plain call's.)"""
    rng = np.random.default_rng(48)
    k, m, K = 16, 48, 64
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    R[:64] = rng.random((64, k), dtype=np.float32)          # a few rows spread over the unit box: the cuts see a box
    Q = rng.random((m, k), dtype=np.float32)
    Q[:24] = (0.97 + 0.03 * rng.random((24, k))).astype(np.float32)
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        want = topk_keys(Q, R, k, K)
        np.testing.assert_array_equal(plain(ix, Q, K), want)
        st_plain = ix.last_stats()
        print("plain call on the empty-corner batch:", st_plain)
        for rname, r2 in radii(want):
            if r2 == float("inf"):
                continue
            got = within(ix, Q, K, r2)
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0 and st[1] <= st_plain[1], (rname, st, st_plain)
            np.testing.assert_array_equal(got, clip(want, r2), err_msg=rname)
        assert st_plain[0] == 4, st_plain
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [FP16, BINS], ids=["fp16", "bins"])
def test_a_far_away_query_falls_back_clipped_and_the_next_batch_is_pruned_again(opts):
    rng = np.random.default_rng(45)
    k, m = 16, 70
    R = rng.random((N17, k), dtype=np.float32)
    R[10, 3] = np.nan
    R[20, 0] = np.inf
    R[30] = 3e38
    Q = spread_queries(rng, m, k)
    Qfar = Q.copy()
    Qfar[1] = 1e6
    Qfar[2, 5] = np.nan
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=4)
    try:
        for K in (1, 8, 64):
            want = topk_keys(Q, R, k, K, base=4)
            want_far = topk_keys(Qfar, R, k, K, base=4)
            r2 = radii(want)[0][1]
            np.testing.assert_array_equal(within(ix, Qfar, K, r2), clip(want_far, r2), err_msg=f"far K={K}")
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 1, st
            np.testing.assert_array_equal(within(ix, Q, K, r2), clip(want, r2), err_msg=f"K={K}")
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, st
    finally:
        ix.close()


def test_two_passes_as_a_fold():
    """m = 1024 + 7: two passes of the pruned top-K; the call folds into keys another shard left — keys beyond the radius among
    them, which stay.  (The batch repeats 96 queries: the oracle is computed once for them.)"""
    rng = np.random.default_rng(49)
    k, m, m0 = 16, 1024 + 7, 96
    R = rng.random((N17, k), dtype=np.float32)
    Q0 = spread_queries(rng, m0, k)
    rep = np.arange(m) % m0
    Q = Q0[rep]
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=N17)
    try:
        for K in (8, 64):
            want = topk_keys(Q0, R, k, K, base=N17)
            held = topk_keys(Q0, rng.random((400, k), dtype=np.float32), k, K, base=0)
            r2 = radii(want)[0][1]
            assert (keys_dist2(held) > np.float32(r2)).any()
            got = within(ix, Q, K, r2, init=False, keys=dev_keys(m, K, fill=held[rep]))
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, st
            exp = np.sort(np.concatenate([held, clip(want, r2)], axis=1), axis=1)[:, :K]
            np.testing.assert_array_equal(got, exp[rep], err_msg=f"K={K}")
            np.testing.assert_array_equal(within(ix, Q, K, r2), clip(want, r2)[rep])
    finally:
        ix.close()


@pytest.mark.parametrize("name,opts,flags,way", [("per_cell_frames", CENTRED, dict(frames=True), 4), ("dense_filter", DENSE, {}, 2)],
                         ids=["per_cell_frames", "dense_filter"])
def test_the_ways_without_a_radius_in_their_kernels_are_exact_and_clipped(name, opts, flags, way):
    rng = np.random.default_rng(52)
    k, m = 16, 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=6)
    try:
        want64 = topk_keys(Q, R, k, 64, base=6)
        for K in (1, 17, 64):
            want = want64[:, :K]
            for rname, r2 in radii(want):
                got = within(ix, Q, K, r2, **flags)
                assert ix.last_stats()[0] == way, (name, ix.last_stats())
                np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"{name} K={K} {rname}")
        # a fold: the held keys stay, the clipped list joins them
        K = 8
        want = want64[:, :K]
        r2 = radii(want)[0][1]
        held = topk_keys(Q, rng.random((400, k), dtype=np.float32), k, K, base=6 + N17)
        got = within(ix, Q, K, r2, init=False, keys=dev_keys(m, K, fill=held), **flags)
        np.testing.assert_array_equal(got, np.sort(np.concatenate([held, clip(want, r2)], axis=1), axis=1)[:, :K])
    finally:
        ix.close()


def test_a_cell_range_shard_pair_merges_to_the_clipped_global_topk():
    rng = np.random.default_rng(26)
    k, n, m = 16, (1 << 19) + 5, 40
    R = rng.random((n, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    pkg.set_option("topk_cells", 1)
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2)
    try:
        want64 = topk_keys(Q, R, k, 64, chunk=16)
        for K in (8, 64):
            want = want64[:, :K]
            for rname, r2 in radii(want):
                lists = []
                for r, ix in enumerate(sh.idx):
                    lists.append(within(ix, Q, K, r2, partial=True))
                    st = ix.last_stats()
                    assert st[0] == 4, (r, K, rname, st)
                    assert (keys_dist2(lists[r])[lists[r] != KEY_INIT] <= np.float32(r2)).all()
                acc, other = dev_keys(m, K, fill=lists[0]), dev_keys(m, K, fill=lists[1])
                pkg.keys_topk_merge(other.data_ptr(), acc.data_ptr(), m, K)
                torch.cuda.synchronize()
                np.testing.assert_array_equal(host_keys(acc, m, K), clip(want, r2), err_msg=f"K={K} {rname}")
    finally:
        sh.close()
