"""Top-K on cell-range shards with KNN_QUERY_TOPK_PARTIAL (include/knn_mi355x.h §2c), the parts that need no GPU:
the plan (knn_debug_cells_topk_plan, input `sharded` = 2: a cell-range shard whose call carries the flag) and a numpy restatement
of the contract — why lists cut at a bound drawn from K rows of the GLOBAL set merge to the global top-K."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_INIT = np.uint64(0x7F80000000000000)


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import multicore_hw2_amd as p
    if not os.path.exists(p.lib_path):
        import __graft_entry__ as g
        g.build()
    return p


# ---- the plan ---------------------------------------------------------------------------------------------------------------

def _inputs(**change):
    # a rank of 8 of a 2^24-row set: 2^13 cells (a cell-range shard is always fp16, not centred, k <= 16)
    base = dict(k=16, K=8, m=256, n=1 << 21, topk_cells=1, has_cells=1, centred=0, rows_u8=0, bins=0, sharded=0, n_outliers=0,
                ncells=8192, nitems=8192, cap=1024, several_slots=0, scan_blocks=0, scan_deal=0, num_cu=256, rec_cap=1 << 22, cells=0)
    return dict(base, **change)


@pytest.mark.parametrize("k", [3, 8, 16])
@pytest.mark.parametrize("K", [1, 8, 33, 64])
@pytest.mark.parametrize("m", [5, 80, 1024, 1500])
def test_a_shard_call_with_the_flag_is_planned_like_an_unsharded_layout(pkg, k, K, m):
    """sharded = 2 under topk_cells 1: served, with exactly the launch shapes of the same inputs without a shard.  (This is the
    case that is declined before the flag exists.)"""
    for change in (dict(), dict(scan_deal=1), dict(scan_deal=2, several_slots=1), dict(n_outliers=50), dict(ncells=2048, nitems=3000)):
        plain = pkg.debug_cells_topk_plan(**_inputs(k=k, K=K, m=m, sharded=0, **change))
        shard = pkg.debug_cells_topk_plan(**_inputs(k=k, K=K, m=m, sharded=2, **change))
        assert plain["use"] == 1 and shard["use"] == 1, (change, plain, shard)
        assert shard == plain, (change, plain, shard)
        assert shard["prep_kt"] == 1 and shard["scan_kt"] == 1 and shard["scan_self"] == 0 and shard["scan_ctr"] == 0
        assert shard["passes"] == -(-m // 1024)


def test_a_shard_is_pruned_on_request_only(pkg):
    for K in (1, 8, 64):
        for opt in (0, 2):       # the policy declines (nothing is measured on a shard yet), and "never" is never
            assert pkg.debug_cells_topk_plan(**_inputs(K=K, sharded=2, topk_cells=opt))["use"] == 0, (K, opt)
        for opt in (0, 1, 2):    # without the flag a cell-range shard keeps the exact top-K under every option
            assert pkg.debug_cells_topk_plan(**_inputs(K=K, sharded=1, topk_cells=opt))["use"] == 0, (K, opt)
        assert pkg.debug_cells_topk_plan(**_inputs(K=K, sharded=2, topk_cells=1))["use"] == 1


def test_a_flagged_shard_call_is_declined_where_an_unsharded_layout_is(pkg):
    for change in (dict(has_cells=0), dict(m=4), dict(n_outliers=(4096 + 128 * 8) // 2 + 1), dict(K=65), dict(centred=1),
                   dict(rows_u8=1, bins=0)):
        assert pkg.debug_cells_topk_plan(**_inputs(sharded=2, **change))["use"] == 0, change


# ---- the contract, restated ---------------------------------------------------------------------------------------------------

def _keys(d, gid):
    return (np.asarray(d, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(gid, dtype=np.uint64)


def _partial_lists(keys, owner, nranks, K, rng, extra):
    """What the flag guarantees of every rank, for one query.  The bound: the largest of K keys of K DISTINCT rows drawn from any
    ranks — so at least K rows of the global set have a key <= it, which is all the argument needs.  A rank keeps every row of its
    own with a key <= the bound, may add up to `extra` rows beyond it (rows between the bound and the gate), and reports the K
    smallest of what it kept, ascending, padded with KEY_INIT."""
    drawn = rng.choice(keys.size, size=K, replace=False)
    bound = keys[drawn].max()
    lists = np.full((nranks, K), KEY_INIT, dtype=np.uint64)
    for r in range(nranks):
        mine = keys[owner == r]
        kept = mine[mine <= bound]
        beyond = mine[mine > bound]
        if extra and beyond.size:
            kept = np.concatenate([kept, rng.choice(beyond, size=min(extra, beyond.size), replace=False)])
        kept = np.sort(kept)[:K]
        lists[r, :kept.size] = kept
    return bound, lists


def _merge(lists, K):
    allk = np.sort(lists.reshape(-1))
    allk = allk[allk != KEY_INIT][:K]
    out = np.full(K, KEY_INIT, dtype=np.uint64)
    out[:allk.size] = allk
    return out


@pytest.mark.parametrize("K", [1, 8, 33, 64])
@pytest.mark.parametrize("nranks", [2, 4, 8])
def test_lists_cut_at_a_bound_from_k_global_rows_merge_to_the_global_topk(K, nranks):
    rng = np.random.default_rng(100 * K + nranks)
    for trial in range(60):
        n = int(rng.integers(K, 40 * K + 2))
        d = rng.random(n, dtype=np.float32)
        if trial % 2:
            d = (np.round(d * 6) / 6).astype(np.float32)          # few distinct distances: ties everywhere, the K-th place included
        owner = rng.integers(0, nranks, n)
        if trial % 5 == 0:
            owner[:] = np.where(rng.random(n) < 0.9, 0, owner)    # most queries are foreign to most ranks
        keys = _keys(d, rng.permutation(n) + 7)
        want = np.sort(keys)[:K]
        bound, lists = _partial_lists(keys, owner, nranks, K, rng, extra=trial % 3)
        assert bound >= want[-1]                                  # K distinct rows: the bound is never below the global K-th key
        np.testing.assert_array_equal(_merge(lists, K), want)
        for r in range(nranks):
            real = lists[r][lists[r] != KEY_INIT]
            assert (real[1:] > real[:-1]).all()                       # strictly ascending
            assert np.isin(want[np.isin(want, keys[owner == r])], real).all()     # the rank's share of the global answer is there


def test_a_tie_at_the_kth_place_that_straddles_two_ranks():
    """Equal distances across the K-th place, the copies owned by two ranks: the merged answer takes the lower global numbers, and
    each rank must report ITS tied rows that are in — a rank that cut at the K-th DISTANCE exclusive would lose them."""
    rng = np.random.default_rng(5)
    K, n = 8, 200
    d = (0.5 + rng.random(n)).astype(np.float32)
    d[:5] = 0.1                                   # five rows nearer than the tie
    tie = np.arange(5, 17)                        # twelve rows at one distance: places 6 .. 17, the K-th (8) among them
    d[tie] = 0.25
    owner = rng.integers(0, 2, n)
    owner[tie] = np.arange(tie.size) % 2          # alternating owners: ranks 0 and 1 both hold tied rows inside AND outside the top 8
    gid = np.arange(n) + 100
    keys = _keys(d, gid)
    want = np.sort(keys)[:K]
    assert set((want & np.uint64(0xFFFFFFFF)).astype(int)) == set(range(100, 108))          # 5 near rows + the 3 lowest-numbered ties
    for extra in (0, 2):
        bound, lists = _partial_lists(keys, owner, 2, K, rng, extra)
        np.testing.assert_array_equal(_merge(lists, K), want)
        for r in range(2):
            inside = want[np.isin(want, keys[owner == r])]
            assert inside.size and np.isin(inside, lists[r]).all()
