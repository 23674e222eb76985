"""knn_index_count_within on the cell-pruned scan (KNN_QUERY_COUNT_CELLS; DESIGN §4.6, "Counts within a radius") on the GPU against
tests/count_oracle.py.  Bar: exact counts at every radius; "pruned" means knn_index_last_stats()[0] == 4, [2] != 0 a pass that fell
back and was answered by the exact count."""
import itertools

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count, dev, dev_counts
from tests.count_oracle import counts, counts_of, radii
from tests.shards_helper import Shards
from tests.test_within_cells_gpu import BINS, CENTRED, FP16, MATRIX, N17, OPTIONS, spread_queries
from tests.topk_oracle import topk_keys, v0_dist2
from tests.within_helper import plain

pytestmark = pytest.mark.gpu
PRUNED = ("at", "below", "zero", "under_all")     # the radii a K <= 64 list could be taken at: the pass must stay pruned there


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


@pytest.mark.parametrize("name,k,opts", MATRIX, ids=[c[0] for c in MATRIX])
def test_every_radius_is_exact_and_the_list_radii_stay_pruned(name, k, opts):
    rng = np.random.default_rng(N17 + 7 * k)
    m = 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=11)
    try:
        for rname, r2 in radii(d):
            want = counts_of(d, r2)
            got = count(ix, Q, r2, cells=True)
            st = ix.last_stats()
            if rname in PRUNED:
                assert st[0] == 4 and st[2] == 0, (name, rname, st)
            elif rname == "inf":
                assert st[0] == 1, (name, st)          # +INF under the cell flag: no cap to prune with
            else:
                print(f"{name}: large radius r2={r2}: last_stats {st}, largest count {want.max()}")   # pruned or not: unmeasured, not gated
            np.testing.assert_array_equal(got, want, err_msg=f"{name} {rname} r2={r2}")
        # without the flag the exact count answers; a fold on the pruned way adds
        r2 = radii(d)[0][1]
        want = counts_of(d, r2)
        np.testing.assert_array_equal(count(ix, Q, r2), want)
        assert ix.last_stats()[0] == 1
        held = np.arange(m, dtype=np.uint32) * 5
        np.testing.assert_array_equal(count(ix, Q, r2, counts=dev_counts(m, fill=held), init=False, cells=True), held + want)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0
        np.testing.assert_array_equal(count(ix, Q[:4], r2, cells=True), want[:4])       # m < 5: the exact count
        assert ix.last_stats()[0] == 1
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [FP16, BINS], ids=["fp16", "bins"])
def test_a_far_away_query_falls_back_exact_and_the_next_batch_is_pruned_again(opts):
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
    d, dfar = v0_dist2(Q, R, k), v0_dist2(Qfar, R, k)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=4)
    try:
        r2 = radii(d)[0][1]
        for init in (True, False):
            held = np.full(m, 40, np.uint32)
            got = count(ix, Qfar, r2, cells=True, init=init, counts=dev_counts(m, fill=held))
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 1, st
            np.testing.assert_array_equal(got, counts_of(dfar, r2) + (0 if init else held), err_msg=f"far, init={init}")
            got = count(ix, Q, r2, cells=True, init=init, counts=dev_counts(m, fill=held))
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, st
            np.testing.assert_array_equal(got, counts_of(d, r2) + (0 if init else held), err_msg=f"init={init}")
        assert counts_of(dfar, r2)[1] == 0 and counts_of(dfar, r2)[2] == 0
    finally:
        ix.close()


def test_two_passes():
    """m = 1024 + 6: two passes of the pruned count.  (The batch repeats 96 queries: the oracle is computed once for them.)"""
    rng = np.random.default_rng(49)
    k, m, m0 = 16, 1024 + 6, 96
    R = rng.random((N17, k), dtype=np.float32)
    Q0 = spread_queries(rng, m0, k)
    rep = np.arange(m) % m0
    d = v0_dist2(Q0, R, k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        for rname, r2 in radii(d)[:2]:
            want = counts_of(d, r2)[rep]
            got = count(ix, Q0[rep], r2, cells=True)
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, st
            np.testing.assert_array_equal(got, want, err_msg=rname)
            held = (np.arange(m, dtype=np.uint32) % 7) * 100
            np.testing.assert_array_equal(count(ix, Q0[rep], r2, cells=True, init=False, counts=dev_counts(m, fill=held)), held + want)
    finally:
        ix.close()


def test_rows_outside_the_robust_box_are_counted_exactly_once():
    """The rows of test_empty_corner_query_and_fewer_real_rows_than_k (tests/test_cells_topk_gpu.py): a tight cluster and 64 rows
    spread over the unit box, 51 of them outside the filter's robust box ([3]) — they sit in the layout (norm +INF: the re-rank
    skips them) and in the outlier list (the outlier kernel counts them).  Queries right beside each of the 64: a radius that holds
    just that row must count 1, not 0 and not 2."""
    rng = np.random.default_rng(48)
    k = 16
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    R[:64] = rng.random((64, k), dtype=np.float32)
    Q = (R[:64] + np.float32(1e-3) * rng.random((64, k), dtype=np.float32)).astype(np.float32)
    d = v0_dist2(Q, R, k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        own = float(d[np.arange(64), np.arange(64)].max())
        for r2 in (own, 10.0 * own):
            want = counts_of(d, r2)
            got = count(ix, Q, r2, cells=True)
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0 and st[3] == 51, st
            np.testing.assert_array_equal(got, want, err_msg=f"r2={r2}")
        assert (counts_of(d, own) == 1).sum() >= 51
    finally:
        ix.close()


def test_per_cell_frames_take_the_exact_count():
    rng = np.random.default_rng(52)
    k, m = 16, 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    _set(CENTRED)
    ix = pkg.KnnIndex(k, R, base_index=6)
    try:
        for rname, r2 in radii(d):
            got = count(ix, Q, r2, cells=True)
            assert ix.last_stats()[0] == 1, (rname, ix.last_stats())
            np.testing.assert_array_equal(got, counts_of(d, r2), err_msg=rname)
    finally:
        ix.close()


def test_one_nn_top_k_and_count_calls_in_every_order_on_one_slot():
    rng = np.random.default_rng(53)
    k, m, K, slot = 16, 96, 8, 3
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    want_keys = topk_keys(Q, R, k, K)
    r2 = radii(d)[0][1]
    want = counts_of(d, r2)
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    q_d = torch.from_numpy(Q.reshape(-1)).to(dev())

    def one_nn():
        keys = torch.empty(m, dtype=torch.int64, device=dev())
        ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), slot=slot, init_keys=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[0] == 4, ix.last_stats()
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), want_keys[:, 0])

    def top_k():
        np.testing.assert_array_equal(plain(ix, Q, K, slot=slot), want_keys)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0, ix.last_stats()

    def counted():
        np.testing.assert_array_equal(count(ix, Q, r2, cells=True, slot=slot), want)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0, ix.last_stats()

    try:
        for order in itertools.permutations((one_nn, top_k, counted)):
            for call in order:
                call()
    finally:
        ix.close()


@pytest.mark.parametrize("attach", [True, False], ids=["seed_layer_attached", "no_seed_layer"])
def test_a_cell_range_shard_pair_folds_to_the_global_count(attach):
    rng = np.random.default_rng(26)
    k, n, m = 16, (1 << 19) + 5, 40
    R = rng.random((n, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q[:m], R, k)
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=attach)
    try:
        for rname, r2 in radii(d):
            if r2 == float("inf"):
                continue
            c = dev_counts(m, fill=0xDEADBEEF)
            for r, ix in enumerate(sh.idx):
                got = count(ix, Q, r2, cells=True, counts=c, init=(r == 0))
                st = ix.last_stats()
                assert st[0] == 4, (r, rname, st)
                if rname != "large":
                    assert st[2] == 0, (r, rname, st)
            np.testing.assert_array_equal(got, counts_of(d, r2), err_msg=rname)
        # each rank's count is its own rows'
        r2 = radii(d)[0][1]
        for r, ix in enumerate(sh.idx):
            np.testing.assert_array_equal(count(ix, Q, r2, cells=True), counts(Q, sh.rows[r].cpu().numpy(), k, r2))
    finally:
        sh.close()


def test_the_top_k_within_lists_are_as_long_as_the_count_allows():
    """Secondary cross-check (the product against itself, never the primary bar): at K = 64 the list lengths of
    knn_index_query_topk_within_host equal min(count, 64) on the same index and radius."""
    rng = np.random.default_rng(54)
    k, m = 16, 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        for rname, r2 in radii(d):
            got = count(ix, Q, r2, cells=True)
            _, _, lengths = ix.query_topk_within_host(Q, 64, r2)
            np.testing.assert_array_equal(lengths, np.minimum(got, 64).astype(np.int32), err_msg=rname)
            np.testing.assert_array_equal(got, counts_of(d, r2), err_msg=rname)
    finally:
        ix.close()
