"""Top-K on cell-range shards with KNN_QUERY_TOPK_PARTIAL (include/knn_mi355x.h §2c) on the GPU, option
`topk_cells` = 1: every rank takes the cell-pruned top-K (knn_index_last_stats()[0] == 4), bounded by the K-th smallest seed score
over rows of the GLOBAL set that the seed layer reaches, and reports what the global top-K needs of it.  Shards are built with the
flow of tests/test_topk_gpu.py::test_cell_range_shards_carry_gids; all ranks of a set live on the one GPU a test box has.

The oracle is tests/topk_oracle.py (v0's arithmetic restated in numpy), applied per query to a candidate set that provably holds
the query's 64 nearest rows: the 256 rows a float32 distance on the GPU ranks first, accepted only when the oracle's 64th distance
lies below the 256th of that ranking by more than the ranking's rounding error could be (asserted in _oracle_topk) — every row left
out then has a larger v0 distance than 64 candidates.  A query with a coordinate that is not finite goes through the oracle whole.
Bar: bit-exact keys."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index, topk_keys, v0_dist2

pytestmark = pytest.mark.gpu
OPTIONS = ("path", "cells", "topk_cells")
KNN_EINVAL = -1


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    pkg.set_option("topk_cells", 1)
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


def _topk(ix, Q, K, keys=None, init=True, partial=True, slot=0):
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    if keys is None:
        keys = _keys(m, K)
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=_dev())
    ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=init, indices_dev=ind.data_ptr(), slot=slot, partial=partial)
    torch.cuda.synchronize()
    got = _host(keys, m, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return got


def _oracle_topk(Q, R, R_d, k, K=64, gids=None):
    """uint64 [m][K]: tests/topk_oracle.topk_keys of every query over its candidates (see the module's docstring)."""
    Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, k)
    n, C = R.shape[0], 4 * K
    g = np.arange(n, dtype=np.int64) if gids is None else np.asarray(gids).astype(np.int64)
    out = np.empty((Q.shape[0], K), dtype=np.uint64)
    finite = np.isfinite(Q).all(axis=1)
    if n <= C:
        return topk_keys(Q, R, k, K, gids=g)
    for c0 in range(0, Q.shape[0], 128):
        Qc = torch.from_numpy(Q[c0:c0 + 128]).to(_dev())
        d = torch.zeros((Qc.shape[0], n), dtype=torch.float32, device=_dev())
        for j in range(k):
            d += (Qc[:, j:j + 1] - R_d[:, j][None, :]) ** 2
        d = torch.nan_to_num(d, nan=float("inf"))
        vals, idx = torch.topk(d, C, dim=1, largest=False)
        vals, idx = vals.cpu().numpy(), idx.cpu().numpy()
        for i in range(Qc.shape[0]):
            q = c0 + i
            if not finite[q]:
                out[q] = topk_keys(Q[q], R, k, K, gids=g)[0]
                continue
            cand = np.sort(idx[i])
            out[q] = topk_keys(Q[q], R[cand], k, K, gids=g[cand])[0]
            # the ranking's float32 sums differ from v0's by a few ulps per term (k <= 16 terms: < 1e-5 relative)
            assert out[q, K - 1] != KEY_INIT and keys_dist2(out[q, K - 1:K])[0] < vals[i, C - 1] * np.float32(1 - 1e-4), q
    return out


class Shards:
    """N cell-range shards of one reference set on one GPU, every rank's part of the seed layer exported."""

    def __init__(self, k, R, nranks, seed_tiles=0, attach=True):
        n = R.shape[0]
        self.k, self.n, self.nranks, self.R = k, n, nranks, R
        self.R_d = torch.from_numpy(R).to(_dev())
        self.geom = pkg.KnnGeom(k, n, nranks, R[:: n // 4096][:4096], seed_tiles)
        owner = torch.empty(n, dtype=torch.int32, device=_dev())
        self.geom.assign(self.R_d.data_ptr(), n, owner.data_ptr())
        torch.cuda.synchronize()
        self.owner = owner.cpu().numpy()
        self.rows, self.gids, self.idx = [], [], []
        for r in range(nranks):
            g = torch.nonzero(owner == r).reshape(-1)
            self.rows.append(self.R_d[g].contiguous())
            self.gids.append(g.to(torch.int32))
            self.idx.append(pkg.KnnIndex.sharded(self.geom, r, self.rows[r].data_ptr(), self.gids[r].data_ptr(),
                                                 self.rows[r].shape[0], owners=(self.rows[r], self.gids[r])))
        self.layer = torch.zeros(self.geom.layer_bytes, dtype=torch.uint8, device=_dev())
        for ix in self.idx:
            ix.seed_export(self.layer.data_ptr())
        torch.cuda.synchronize()
        if attach:
            for ix in self.idx:
                ix.seed_attach(self.layer.data_ptr(), owner=self.layer)

    def close(self):
        for ix in self.idx:
            ix.close()
        self.geom.close()


def _check(sh, Q, K, want, expect_fallback=None):
    """One flagged call per rank, every clause of the contract, the merge and the fold.  want: the global oracle [m][>= K].
    Returns the ranks' lists and statistics."""
    Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, sh.k)
    m = Q.shape[0]
    want = want[:, :K]
    lists, stats = [], []
    for r, ix in enumerate(sh.idx):
        got = _topk(ix, Q, K)
        st = ix.last_stats()
        assert st[0] == 4, (r, K, st)
        if expect_fallback is not None:
            assert st[2] == expect_fallback, (r, K, st)
        real = got != KEY_INIT
        for j in range(m):
            row = got[j][real[j]]
            assert real[j][:row.size].all(), (r, j)                                   # padding only behind the real keys
            assert (row[1:] > row[:-1]).all(), (r, j, row)                            # strictly ascending
            gid = keys_index(row).astype(np.int64)
            assert (sh.owner[gid] == r).all(), (r, j, gid)                            # rows of THIS rank ...
            d = v0_dist2(Q[j], sh.R[gid], sh.k)[0]                                    # ... with the oracle's bit-exact keys
            np.testing.assert_array_equal(row >> np.uint64(32), d.view(np.uint32).astype(np.uint64), err_msg=f"rank {r} query {j}")
            mine = want[j][(want[j] != KEY_INIT)]
            mine = mine[sh.owner[keys_index(mine).astype(np.int64)] == r]
            assert np.isin(mine, row).all(), (r, j, K)                                # its share of the global top-K is there
        lists.append(got)
        stats.append(st)
    # knn_keys_topk_merge over the ranks
    acc, others = _keys(m, K, fill=lists[0]), [_keys(m, K, fill=lists[r]) for r in range(1, sh.nranks)]
    for other in others:
        pkg.keys_topk_merge(other.data_ptr(), acc.data_ptr(), m, K)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_host(acc, m, K), want, err_msg=f"merge K={K}")
    # folding the other ranks into rank 0's keys (no INIT_KEYS): the candidates carry gids before the select
    keys = _keys(m, K, fill=lists[0])
    for r in range(1, sh.nranks):
        folded = _topk(sh.idx[r], Q, K, keys=keys, init=False)
    np.testing.assert_array_equal(folded, want, err_msg=f"fold K={K}")
    return lists, stats


# ---- 1. uniform rows, two ranks (shared by the cases below that need no other data) --------------------------------------------

@pytest.fixture(scope="module")
def uniform():
    rng = np.random.default_rng(26)
    k, n, m = 16, (1 << 19) + 5, 80
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    R_d = torch.from_numpy(R).to(_dev())
    return dict(k=k, n=n, m=m, R=R, Q=Q, want=_oracle_topk(Q, R, R_d, k))


def test_two_ranks_of_uniform_rows(uniform):
    sh = Shards(uniform["k"], uniform["R"], 2)
    try:
        assert all(r.shape[0] > 1000 for r in sh.rows)
        for K in (1, 8, 64):
            # K 8: nothing may fall back — a pass that fell back says nothing about the pruned path
            _check(sh, uniform["Q"], K, uniform["want"], expect_fallback=0 if K == 8 else None)
    finally:
        sh.close()


# ---- 2. other shapes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,nranks,n,m", [(16, 4, 1 << 20, 500), (8, 3, (1 << 19) + 4099, 200)], ids=["k16_4ranks", "k8_3ranks"])
def test_other_shapes(k, nranks, n, m):
    rng = np.random.default_rng(k * 131 + nranks)
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    sh = Shards(k, R, nranks)
    try:
        want = _oracle_topk(Q, R, sh.R_d, k)
        # most queries are foreign to each rank: their bound can only come from the other ranks' rows in the layer
        assert nranks < 4 or (np.bincount(sh.owner[keys_index(want[:, 0]).astype(np.int64)], minlength=nranks) < 0.6 * m).all()
        for K in (8, 33):      # 33 crosses the 32-lane half of the selection network
            _check(sh, Q, K, want)
    finally:
        sh.close()


# ---- 3. no layer attached, other layer depths ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(attach=False), dict(seed_tiles=1), dict(seed_tiles=4)], ids=["no_layer", "T1", "T4"])
def test_without_the_layer_and_with_other_layer_depths(uniform, kw):
    sh = Shards(uniform["k"], uniform["R"], 2, **kw)
    try:
        for K in (8, 64):
            lists, _ = _check(sh, uniform["Q"], K, uniform["want"])
            if not kw.get("attach", True):      # the bound comes from the rank's own rows: its list is its own complete top-K
                for r in range(2):
                    own = _oracle_topk(uniform["Q"], sh.rows[r].cpu().numpy(), sh.rows[r], uniform["k"], K=K,
                                       gids=sh.gids[r].cpu().numpy())
                    np.testing.assert_array_equal(lists[r], own, err_msg=f"rank {r} K={K}")
    finally:
        sh.close()


# ---- 4. a tie across two ranks at the K-th place --------------------------------------------------------------------------------

def test_a_tie_across_two_ranks_at_the_kth_place(uniform):
    """Twelve copies of two rows at exactly the same distance (0.25^2, one non-zero term) from query 0, the two on either side of the
    cut that decides the rank, their global numbers interleaved; five rows nearer.  K 8 cuts through the tie: the merged answer takes
    the three lowest-numbered copies, which two ranks own."""
    k, n = uniform["k"], uniform["n"]
    R, Q = uniform["R"].copy(), uniform["Q"].copy()
    # the dimension whose central cut separates the two ranks: ask the geometry (the construction of tests/test_shards_gpu.py's tie
    # test, without relying on which dimension carries the top code bit at this size)
    probe = np.full((2 * k, k), 0.5, dtype=np.float32)
    for d in range(k):
        probe[2 * d, d], probe[2 * d + 1, d] = 0.25, 0.75
    geom = pkg.KnnGeom(k, n, 2, R[:: n // 4096][:4096])
    p_d, own = torch.from_numpy(probe).to(_dev()), torch.empty(2 * k, dtype=torch.int32, device=_dev())
    geom.assign(p_d.data_ptr(), 2 * k, own.data_ptr())
    torch.cuda.synchronize()
    geom.close()
    own = own.cpu().numpy()
    dims = [d for d in range(k) if own[2 * d] != own[2 * d + 1]]
    assert dims, own
    d = dims[0]
    q = Q[0]
    q[d] = 0.5
    near = 2000 + 11 * np.arange(5)
    for t, i in enumerate(near):
        R[i] = q
        R[i, (d + 1) % k] += np.float32(0.01 * (t + 1))
    tie = 5000 + 13 * np.arange(12)
    for t, i in enumerate(tie):
        R[i] = q
        R[i, d] = 0.25 if t % 2 == 0 else 0.75
    sh = Shards(k, R, 2)
    try:
        assert sh.owner[tie[0]] != sh.owner[tie[1]] and (sh.owner[tie[::2]] == sh.owner[tie[0]]).all()
        want = _oracle_topk(Q, R, sh.R_d, k)
        assert list(keys_index(want[0, :8])) == list(near) + list(tie[:3])                    # the case is what it says
        assert len(set(want[0, 5:17] >> np.uint64(32))) == 1
        for K in (8, 6, 17):        # the K-th place inside the tie, at its first row, at its last
            _check(sh, Q, K, want)
    finally:
        sh.close()


# ---- 5. fallback, out-of-box rows ----------------------------------------------------------------------------------------------

def test_a_non_finite_query_falls_back_once_with_gids(uniform):
    Qbad = uniform["Q"].copy()
    Qbad[3, 2] = np.nan
    sh = Shards(uniform["k"], uniform["R"], 2)
    try:
        want_bad = uniform["want"].copy()
        want_bad[3] = KEY_INIT                  # no finite distance: (+INF, 0) in every slot
        _check(sh, Qbad, 8, want_bad, expect_fallback=1)     # the gated exact top-K answers, with gids
        _check(sh, uniform["Q"], 8, uniform["want"], expect_fallback=0)     # and the next call is pruned again
    finally:
        sh.close()


def test_out_of_box_rows_appear_once_with_their_gids():
    """tests/test_cells_topk_gpu.py's construction on two ranks: a tight cluster, 64 rows spread over the unit box, 8 rows planted
    beyond every other row in every coordinate (outside the robust box whenever any row is), queries in the corner beside them."""
    rng = np.random.default_rng(48)
    k, n, m = 16, (1 << 19) + 5, 48
    R = (0.45 + 0.1 * rng.random((n, k))).astype(np.float32)
    spread = 7 + 8191 * np.arange(64)
    R[spread] = rng.random((64, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Q[:24] = (0.97 + 0.03 * rng.random((24, k))).astype(np.float32)
    planted = spread[:8]
    R[planted] = (1.2 + 0.1 * rng.random((8, k))).astype(np.float32)
    sh = Shards(k, R, 2)
    try:
        want = _oracle_topk(Q, R, sh.R_d, k)
        assert all(set(planted) <= set(keys_index(want[q])) for q in range(24))
        for K in (8, 64):
            lists, stats = _check(sh, Q, K, want)
            assert sum(st[3] for st in stats) > 0, stats              # some rank holds rows outside the box
            for q in range(24):
                both = np.concatenate([keys_index(l[q][l[q] != KEY_INIT]) for l in lists])
                assert len(set(both)) == both.size                    # no row twice, on a rank or across ranks
                assert K < 64 or set(planted) <= set(both)
                assert np.isin(both, planted).any()
    finally:
        sh.close()


# ---- 6. two passes; 1-NN and top-K alternating on one slot ---------------------------------------------------------------------

def test_two_passes_and_alternating_calls_on_one_slot(uniform):
    rng = np.random.default_rng(61)
    k, m, K = uniform["k"], 1500, 8
    Q = rng.random((m, k), dtype=np.float32)
    sh = Shards(k, uniform["R"], 2)
    try:
        want = _oracle_topk(Q, uniform["R"], sh.R_d, k, K=K)
        q_d = torch.from_numpy(Q.reshape(-1)).to(_dev())
        one = torch.empty((2, 2, m), dtype=torch.int64, device=_dev())
        top = [[_keys(m, K) for _ in range(2)] for _ in range(2)]
        for r, ix in enumerate(sh.idx):          # 1-NN, top-K, 1-NN, top-K on slot 3 of each shard, no synchronisation between
            for rep in range(2):
                ix.query_keys(m, q_d.data_ptr(), one[r, rep].data_ptr(), init_keys=True, slot=3)
                ix.query_topk(m, K, q_d.data_ptr(), top[r][rep].data_ptr(), init_keys=True, slot=3, partial=True)
            assert ix.last_stats()[0] == 4
        torch.cuda.synchronize()
        for rep in range(2):
            acc = top[0][rep]
            pkg.keys_topk_merge(top[1][rep].data_ptr(), acc.data_ptr(), m, K)
            torch.cuda.synchronize()
            merged = _host(acc, m, K)
            np.testing.assert_array_equal(merged, want)
            nn = one[:, rep].min(dim=0).values.cpu().numpy().view(np.uint64)      # keys < 2^63: int64 min == unsigned min
            np.testing.assert_array_equal(nn, merged[:, 0])                        # 1-NN translated once, top-K not again
    finally:
        sh.close()


# ---- 7. the flag elsewhere -----------------------------------------------------------------------------------------------------

def test_the_flag_changes_nothing_on_other_indexes_and_is_rejected_by_1nn():
    rng = np.random.default_rng(71)
    k, n, m, K = 16, (1 << 17) + 999, 96, 17
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    for opts in ({"path": 1}, {"path": 2, "cells": 2}, {"path": 2, "cells": 1}):
        for o, v in opts.items():
            pkg.set_option(o, v)
        ix = pkg.KnnIndex(k, R, base_index=11)
        try:
            plain = _topk(ix, Q, K, partial=False)
            st = ix.last_stats()
            flagged = _topk(ix, Q, K, partial=True)
            assert ix.last_stats()[0] == st[0]
            np.testing.assert_array_equal(flagged, plain)
            np.testing.assert_array_equal(plain, topk_keys(Q, R, k, K, base=11))
            q_d = torch.from_numpy(Q.reshape(-1)).to(_dev())
            keys = torch.empty(m, dtype=torch.int64, device=_dev())
            for flags in (pkg.QUERY_TOPK_PARTIAL, pkg.QUERY_TOPK_PARTIAL | pkg.QUERY_INIT_KEYS):
                assert pkg.lib().knn_index_query(ix._h, 0, m, q_d.data_ptr(), keys.data_ptr(), None, None, flags) == KNN_EINVAL
                assert pkg.lib().knn_index_query_keys_ex(ix._h, 0, m, q_d.data_ptr(), keys.data_ptr(), None, flags) == KNN_EINVAL
        finally:
            ix.close()
