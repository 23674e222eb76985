"""Top-K queries (knn_index_query_topk, include/knn_mi355x.h section 2c) on the GPU against the numpy restatement of v0
(tests/topk_oracle.py).  Bar: bit-exact keys, in order — distance first, then the lowest global number — on every kind of
index, across shard folds and merges, cell-range shards' gids, and two batches in flight."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index, topk_keys

pytestmark = pytest.mark.gpu
KS = (1, 2, 8, 17, 64)
OPTIONS = ("path", "cells", "cells_rows", "cells_centre")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _dev():
    return torch.device("cuda:0")


def _keys(m, K, fill=None):
    t = torch.empty(m * K, dtype=torch.int64, device=_dev())
    if fill is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.uint64).reshape(-1).view(np.int64)))
    return t


def _host(keys, m, K):
    return keys.cpu().numpy().view(np.uint64).reshape(m, K)


def _topk(ix, Q, K, keys=None, init=True, slot=0, stream=0):
    """One batch: keys [m][K] (numpy uint64) after the call; the indices it unpacked are checked against the keys."""
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    if keys is None:
        keys = _keys(m, K)
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=_dev())
    ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=init, indices_dev=ind.data_ptr(), slot=slot,
                  stream=stream)
    torch.cuda.synchronize()
    got = _host(keys, m, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return got


def _one_nn(ix, Q):
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    keys = torch.empty(m, dtype=torch.int64, device=_dev())
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), init_keys=True)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


# (name, k, rows, options set before the index is built, whether the 1-NN path must be the one named)
LAYOUTS = [
    ("exact", 16, 5000, {"path": 1}),
    ("filter_k3", 3, 70000, {"path": 2, "cells": 2}),
    ("filter_k16", 16, 70000, {"path": 2, "cells": 2}),
    ("filter_k32", 32, 70000, {"path": 2, "cells": 2}),
    ("filter_k128", 128, 66000, {"path": 2, "cells": 2}),
    ("chunked_k600", 600, 65600, {"path": 2, "cells": 2}),
    ("cells_fp16", 16, (1 << 17) + 999, {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2}),
    ("cells_u8", 16, (1 << 17) + 999, {"path": 2, "cells": 1, "cells_rows": 2}),
    ("cells_centred", 8, (1 << 17) + 999, {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 1}),
    ("grid_k3", 3, 40000, {}),
]
# the path a top-K call takes on each (knn_index_last_stats()[0]): 2 the MFMA filter (dense layouts, and a cell-sorted layout in
# the shard's frame scanned in full), 1 the exact top-K scan (per-cell frames: centred or u8, grid indexes, small shards)
TOPK_PATH = {"exact": 1, "filter_k3": 2, "filter_k16": 2, "filter_k32": 2, "filter_k128": 2, "chunked_k600": 2,
             "cells_fp16": 2, "cells_u8": 1, "cells_centred": 1, "grid_k3": 1}
ONE_NN_PATH = {"exact": 1, "filter_k3": 2, "filter_k16": 2, "filter_k32": 2, "filter_k128": 2, "chunked_k600": 2,
               "cells_fp16": 4, "cells_u8": 4, "cells_centred": 4, "grid_k3": 3}


@pytest.mark.parametrize("name,k,n,opts", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_topk_is_bit_exact_on_every_index_layout(name, k, n, opts):
    rng = np.random.default_rng(n + k)
    m = 96 if k <= 32 else 40
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    base = 11
    for o, v in opts.items():
        pkg.set_option(o, v)
    ix = pkg.KnnIndex(k, R, base_index=base)
    try:
        want = topk_keys(Q, R, k, 64, base=base)
        for K in KS:
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            # the deep-K scans (k > 32) sample with their scan's grid: on a shard this small it has fewer blocks than K = 64,
            # so the batch falls back to the exact top-K by design (still bit-exact)
            deep_fallback = K == 64 and name in ("filter_k128", "chunked_k600")
            assert st[0] == TOPK_PATH[name] and (st[2] == 0 or deep_fallback), (name, K, st)
            assert (st[1] > 0) == (st[0] == 2) or deep_fallback, st   # records the filter handed to the top-K re-rank
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{name} K={K}")
        # K = 1 is knn_index_query on whatever path the index serves 1-NN by
        one = _one_nn(ix, Q)
        assert ix.last_stats()[0] == ONE_NN_PATH[name], ix.last_stats()
        np.testing.assert_array_equal(_topk(ix, Q, 1)[:, 0], one)
    finally:
        ix.close()


def test_duplicates_and_ties_straddling_the_kth_place():
    """A lattice of few values: dozens of rows share every distance, the K-th place cuts through runs of equal distances
    and duplicate rows; the lowest indices win."""
    rng = np.random.default_rng(21)
    k, n, m = 3, 4000, 130
    R = rng.integers(0, 3, (n, k)).astype(np.float32)
    R[1000:1100] = R[5]
    Q = rng.integers(0, 3, (m, k)).astype(np.float32)
    Q[0] = R[5]
    ix = pkg.KnnIndex(k, R, base_index=3)
    try:
        want = topk_keys(Q, R, k, 64, base=3)
        for K in KS:
            np.testing.assert_array_equal(_topk(ix, Q, K), want[:, :K], err_msg=f"K={K}")
        assert (keys_dist2(want[0]) == 0).all()   # 101 copies of query 0: only the first 64 of them
    finally:
        ix.close()


def test_non_finite_rows_and_a_far_away_query():
    rng = np.random.default_rng(22)
    k, n, m = 16, 3000, 70
    R = rng.random((n, k), dtype=np.float32)
    R[10, 3] = np.nan
    R[20, 0] = np.inf
    R[30] = 3e38
    Q = rng.random((m, k), dtype=np.float32)
    Q[1] = 1e6            # far outside the rows' box
    Q[2, 5] = np.nan      # no finite distance at all: every slot stays (+INF, 0)
    ix = pkg.KnnIndex(k, R, base_index=0)
    try:
        want = topk_keys(Q, R, k, 64)
        for K in KS:
            got = _topk(ix, Q, K)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"K={K}")
            assert (got[2] == KEY_INIT).all()
    finally:
        ix.close()


@pytest.mark.parametrize("cells", [2, 1])
def test_far_away_query_raises_the_fallback_on_the_filter_path(cells):
    """A query far outside the rows' box cannot be bounded by the filter: the batch raises FALLBACK, the gated exact top-K
    answers it, bit-exact; the next batch is back on the filter."""
    rng = np.random.default_rng(31 + cells)
    k, n, m = 16, (1 << 17) + 77, 64
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Qfar = Q.copy()
    Qfar[1] = 1e6
    pkg.set_option("path", 2)
    pkg.set_option("cells", cells)
    pkg.set_option("cells_centre", 2)
    pkg.set_option("cells_rows", 1)
    ix = pkg.KnnIndex(k, R, base_index=4)
    try:
        for K in (1, 8, 64):
            np.testing.assert_array_equal(_topk(ix, Qfar, K), topk_keys(Qfar, R, k, K, base=4), err_msg=f"K={K}")
            st = ix.last_stats()
            assert st[0] == 2 and st[2] == 1, st
            np.testing.assert_array_equal(_topk(ix, Q, K), topk_keys(Q, R, k, K, base=4))
            st = ix.last_stats()
            assert st[0] == 2 and st[2] == 0, st
    finally:
        ix.close()


def test_tight_clusters_overflow_the_candidates_and_fall_back_exactly():
    """Two clusters tighter than the fp16 step: every row of a query's cluster passes the threshold, far more than the
    candidate room; the batch falls back to the exact top-K, bit-exact, ties to the lowest index."""
    rng = np.random.default_rng(33)
    k, n, m = 16, 70000, 40
    c = rng.random((2, k), dtype=np.float32)
    R = (c[rng.integers(0, 2, n)] + rng.normal(0, 1e-6, (n, k))).astype(np.float32)
    Q = (c[rng.integers(0, 2, m)] + rng.normal(0, 1e-6, (m, k))).astype(np.float32)
    pkg.set_option("path", 2)
    pkg.set_option("cells", 2)
    ix = pkg.KnnIndex(k, R)
    try:
        want = topk_keys(Q, R, k, 64)
        for K in (1, 17, 64):
            np.testing.assert_array_equal(_topk(ix, Q, K), want[:, :K], err_msg=f"K={K}")
            st = ix.last_stats()
            assert st[0] == 2 and st[2] == 1, st
    finally:
        ix.close()


def test_fewer_rows_than_k():
    rng = np.random.default_rng(23)
    k, m = 4, 9
    R = rng.random((6, k), dtype=np.float32)
    R[4, 1] = np.nan
    Q = rng.random((m, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R, base_index=100)
    try:
        for K in (5, 8, 64):
            got = _topk(ix, Q, K)
            np.testing.assert_array_equal(got, topk_keys(Q, R, k, K, base=100))
            assert (got[:, 5:] == KEY_INIT).all() and (got[:, :5] < KEY_INIT).all()
        idx, d2 = ix.query_topk_host(Q, 8)
        want = topk_keys(Q, R, k, 8, base=100)
        np.testing.assert_array_equal(idx, keys_index(want))
        np.testing.assert_array_equal(d2.view(np.uint32), keys_dist2(want).view(np.uint32))
    finally:
        ix.close()


def test_more_queries_than_one_scan_launch_takes():
    rng = np.random.default_rng(24)
    k, n, m, K = 3, 1500, 65536 + 333, 4
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R)
    try:
        np.testing.assert_array_equal(_topk(ix, Q, K), topk_keys(Q, R, k, K, chunk=4096))
    finally:
        ix.close()


def test_two_index_range_shards_fold_and_merge_to_one_index():
    rng = np.random.default_rng(25)
    k, n, m = 16, 9000, 100
    R = rng.random((n, k), dtype=np.float32)
    R[7000:7050] = R[100:150]            # equal distances across the two shards: the lower global number wins
    Q = rng.random((m, k), dtype=np.float32)
    Q[:5] = R[100:105]
    cut = 4321
    a = pkg.KnnIndex(k, R[:cut], base_index=0)
    b = pkg.KnnIndex(k, R[cut:], base_index=cut)
    whole = pkg.KnnIndex(k, R)
    try:
        for K in KS:
            want = topk_keys(Q, R, k, K)
            np.testing.assert_array_equal(_topk(whole, Q, K), want)
            # fold: shard b writes fresh, shard a folds into b's keys (and the other way round)
            keys = _keys(m, K)
            _topk(b, Q, K, keys=keys, init=True)
            np.testing.assert_array_equal(_topk(a, Q, K, keys=keys, init=False), want, err_msg=f"fold K={K}")
            keys = _keys(m, K, fill=np.full((m, K), KEY_INIT, dtype=np.uint64))
            _topk(a, Q, K, keys=keys, init=False)
            np.testing.assert_array_equal(_topk(b, Q, K, keys=keys, init=False), want)
            # merge: each shard answers alone, knn_keys_topk_merge combines
            ka, kb = _keys(m, K), _keys(m, K)
            _topk(a, Q, K, keys=ka)
            _topk(b, Q, K, keys=kb)
            pkg.keys_topk_merge(ka.data_ptr(), kb.data_ptr(), m, K)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_host(kb, m, K), want, err_msg=f"merge K={K}")
    finally:
        for ix in (a, b, whole):
            ix.close()


def test_cell_range_shards_carry_gids():
    """Two cell-range shards (knn_geom_* / knn_index_create_sharded, the flow of test_shards_gpu.py): the keys carry the
    rows' global numbers, and the two ranks' lists merge to the top-K of the whole set."""
    rng = np.random.default_rng(26)
    k, n, m, nranks = 16, (1 << 19) + 5, 80, 2
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    dev = _dev()
    R_d = torch.from_numpy(R).to(dev)
    geom = pkg.KnnGeom(k, n, nranks, R[:: n // 4096][:4096])
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    geom.assign(R_d.data_ptr(), n, owner.data_ptr())
    torch.cuda.synchronize()
    rows, gids, idx = [], [], []
    try:
        for r in range(nranks):
            g = torch.nonzero(owner == r).reshape(-1)
            rows.append(R_d[g].contiguous())
            gids.append(g.to(torch.int32))
            idx.append(pkg.KnnIndex.sharded(geom, r, rows[r].data_ptr(), gids[r].data_ptr(), rows[r].shape[0],
                                            owners=(rows[r], gids[r])))
        layer = torch.zeros(geom.layer_bytes, dtype=torch.uint8, device=dev)
        for ix in idx:
            ix.seed_export(layer.data_ptr())
        torch.cuda.synchronize()
        for ix in idx:
            ix.seed_attach(layer.data_ptr(), owner=layer)
        want64 = topk_keys(Q, R, k, 64, chunk=16)
        rank64 = [topk_keys(Q, rows[r].cpu().numpy(), k, 64, gids=gids[r].cpu().numpy(), chunk=16) for r in range(nranks)]
        assert all(r.shape[0] > 1000 for r in rows)
        for K in (1, 8, 64):
            want = want64[:, :K]
            lists = []
            for r in range(nranks):
                got = _topk(idx[r], Q, K)
                np.testing.assert_array_equal(got, rank64[r][:, :K], err_msg=f"rank {r} K={K}")
                lists.append(got)
            # fold rank 1 into rank 0's keys on the device
            keys = _keys(m, K, fill=lists[0])
            np.testing.assert_array_equal(_topk(idx[1], Q, K, keys=keys, init=False), want, err_msg=f"K={K}")
    finally:
        for ix in idx:
            ix.close()
        geom.close()


def test_two_slots_in_flight_on_two_streams():
    rng = np.random.default_rng(27)
    k, n, m, K = 16, 20000, 200, 17
    R = rng.random((n, k), dtype=np.float32)
    Qs = [rng.random((m, k), dtype=np.float32) for _ in range(2)]
    ix = pkg.KnnIndex(k, R, base_index=5)
    dev = _dev()
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        q_d = [torch.from_numpy(Q.reshape(-1)).to(dev) for Q in Qs]
        keys = [_keys(m, K) for _ in range(2)]
        torch.cuda.synchronize()
        for s in range(2):
            ix.query_topk(m, K, q_d[s].data_ptr(), keys[s].data_ptr(), stream=streams[s].cuda_stream, slot=s,
                          init_keys=True)
        torch.cuda.synchronize()
        for s in range(2):
            np.testing.assert_array_equal(_host(keys[s], m, K), topk_keys(Qs[s], R, k, K, base=5))
    finally:
        ix.close()


def test_k_out_of_range_is_einval():
    rng = np.random.default_rng(28)
    R = rng.random((100, 3), dtype=np.float32)
    ix = pkg.KnnIndex(3, R)
    q = torch.zeros(3 * 4, dtype=torch.float32, device=_dev())
    keys = torch.zeros(4 * 65, dtype=torch.int64, device=_dev())
    try:
        for K in (0, 65):
            with pytest.raises(pkg.KnnError, match="1 <= K <= 64"):
                ix.query_topk(4, K, q.data_ptr(), keys.data_ptr(), init_keys=True)
            with pytest.raises(pkg.KnnError):
                pkg.keys_topk_merge(keys.data_ptr(), keys.data_ptr(), 4, K)
        with pytest.raises(pkg.KnnError):
            ix.query_topk(0, 4, q.data_ptr(), keys.data_ptr(), init_keys=True)
        torch.cuda.synchronize()
        assert (keys.cpu() == 0).all()     # nothing was launched
    finally:
        ix.close()
