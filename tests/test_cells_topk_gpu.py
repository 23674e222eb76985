"""Top-K queries on the cell-pruned scan (option `topk_cells`) on the GPU against the numpy restatement of v0
(tests/topk_oracle.py).  Bar: bit-exact keys, in order.  "Pruned" means knn_index_last_stats()[0] == 4."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import KEY_INIT, keys_index, topk_keys

pytestmark = pytest.mark.gpu
KS = (1, 2, 8, 17, 64)
OPTIONS = ("path", "cells", "cells_rows", "cells_centre", "cells_u8_frame", "scan_deal", "topk_cells")


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
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    if keys is None:
        keys = _keys(m, K)
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=_dev())
    ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=init, indices_dev=ind.data_ptr(), slot=slot, stream=stream)
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


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


FP16 = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2}
BINS = {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 2}
N17 = (1 << 17) + 999
# (name, k, options before the build): every compiled form of the record-only scan and of the top-K prep kernel
MATRIX = [
    ("fp16_k16_fixed", 16, dict(FP16, scan_deal=1)),
    ("fp16_k16_counter", 16, dict(FP16, scan_deal=2)),
    ("fp16_k8", 8, FP16),
    ("bins_k16", 16, BINS),
    ("nif_k20_fixed", 20, dict(FP16, scan_deal=1)),
    ("nif_k20_counter", 20, dict(FP16, scan_deal=2)),
    ("window_k32_fixed", 32, dict(FP16, scan_deal=1)),
    ("window_k32_counter", 32, dict(FP16, scan_deal=2)),
]


@pytest.mark.parametrize("name,k,opts", MATRIX, ids=[c[0] for c in MATRIX])
def test_pruned_topk_is_bit_exact_on_every_served_layout(name, k, opts):
    """Uniform rows, 512 cells of ~256 rows: pruned, records handed on, and NO fallback — on uniform data at this size a fallback
    means the K-th seed bound or a room is wrong."""
    rng = np.random.default_rng(N17 + k)
    m = 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=11)
    try:
        want = topk_keys(Q, R, k, 64, base=11)
        for K in KS:
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 4 and st[1] > 0 and st[2] == 0, (name, K, st)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{name} K={K}")
        one = _one_nn(ix, Q)
        assert ix.last_stats()[0] == 4
        np.testing.assert_array_equal(_topk(ix, Q, 1)[:, 0], one)
    finally:
        ix.close()


def test_policy_declines_and_the_option_serves_an_index_at_the_size_rule():
    """k 16 at 2^20 + 999 rows (the 1-NN size rule: the library builds the cell-sorted layout on its own).  Default options: the
    policy declines every K for now (no measured win to rest on yet) — the excluded path, the filter's full scan (2);
    `topk_cells` = 1: pruned, bit-exact, no fallback.  And a 2^17-row index whose layout exists because `cells` = 1 forced it is
    not pruned under the policy either (path 2, as tests/test_topk_gpu.py asserts)."""
    rng = np.random.default_rng(41)
    k, m = 16, 64
    n = (1 << 20) + 999
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R, base_index=2)
    try:
        want = topk_keys(Q, R, k, 64, base=2, chunk=16)
        for K in (1, 8, 64):
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 2, (K, st)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"policy K={K}")
        pkg.set_option("topk_cells", 1)
        for K in (1, 8, 64):
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, (K, st)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"K={K}")
        pkg.set_option("topk_cells", 0)
    finally:
        ix.close()
    _set(FP16)
    ix = pkg.KnnIndex(k, R[:N17], base_index=2)
    try:
        want = topk_keys(Q, R[:N17], k, 8, base=2)
        np.testing.assert_array_equal(_topk(ix, Q, 8), want)
        assert ix.last_stats()[0] == 2, ix.last_stats()
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [dict(FP16, cells_centre=1), {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 1}],
                         ids=["centred_fp16", "per_cell_u8"])
def test_per_cell_frames_keep_the_exact_topk(opts):
    rng = np.random.default_rng(42)
    k, m = 8, 40
    R = rng.random((N17, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        np.testing.assert_array_equal(_topk(ix, Q, 8), topk_keys(Q, R, k, 8))
        assert ix.last_stats()[0] == 1, ix.last_stats()
    finally:
        ix.close()


def test_cell_range_shard_keeps_the_exact_topk():
    rng = np.random.default_rng(43)
    k, n, m, nranks = 16, (1 << 19) + 5, 40, 2
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    dev = _dev()
    R_d = torch.from_numpy(R).to(dev)
    geom = pkg.KnnGeom(k, n, nranks, R[:: n // 4096][:4096])
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    geom.assign(R_d.data_ptr(), n, owner.data_ptr())
    torch.cuda.synchronize()
    g = torch.nonzero(owner == 0).reshape(-1)
    rows, gids = R_d[g].contiguous(), g.to(torch.int32)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex.sharded(geom, 0, rows.data_ptr(), gids.data_ptr(), rows.shape[0], owners=(rows, gids))
    try:
        got = _topk(ix, Q, 8)
        assert ix.last_stats()[0] == 1, ix.last_stats()
        np.testing.assert_array_equal(got, topk_keys(Q, rows.cpu().numpy(), k, 8, gids=gids.cpu().numpy(), chunk=16))
    finally:
        ix.close()
        geom.close()


def test_ties_and_duplicates_straddling_the_kth_place():
    """A lattice of few values with planted copies: the K-th place cuts through runs of equal distances; the lowest index wins."""
    rng = np.random.default_rng(44)
    k, m = 16, 64
    R = (rng.integers(0, 4, (N17, k)) / 4.0).astype(np.float32)
    R[90000:90100] = R[5]
    Q = (rng.integers(0, 4, (m, k)) / 4.0).astype(np.float32)
    Q[0] = R[5]
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=3)
    try:
        want = topk_keys(Q, R, k, 64, base=3)
        for K in KS:
            np.testing.assert_array_equal(_topk(ix, Q, K), want[:, :K], err_msg=f"K={K}")
            assert ix.last_stats()[0] == 4
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [FP16, BINS], ids=["fp16", "bins"])
def test_non_finite_rows_and_a_far_away_query_fall_back_once(opts):
    """NaN / +INF / 3e38 rows never enter; a far-away query raises FALLBACK (the exact top-K answers, st[2] == 1) and the next
    batch is pruned again."""
    rng = np.random.default_rng(45)
    k, m = 16, 70
    R = rng.random((N17, k), dtype=np.float32)
    R[10, 3] = np.nan
    R[20, 0] = np.inf
    R[30] = 3e38
    Q = rng.random((m, k), dtype=np.float32)
    Qfar = Q.copy()
    Qfar[1] = 1e6
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=4)
    try:
        for K in (1, 8, 64):
            np.testing.assert_array_equal(_topk(ix, Qfar, K), topk_keys(Qfar, R, k, K, base=4), err_msg=f"far K={K}")
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 1, st
            np.testing.assert_array_equal(_topk(ix, Q, K), topk_keys(Q, R, k, K, base=4), err_msg=f"K={K}")
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, st
    finally:
        ix.close()


def test_tight_clusters_overflow_and_fall_back_exactly():
    """Two clusters tighter than the fp16 step: every row of a query's cluster is a candidate — over-full, FALLBACK, bit-exact."""
    rng = np.random.default_rng(46)
    k, m = 16, 40
    c = rng.random((2, k), dtype=np.float32)
    R = (c[rng.integers(0, 2, N17)] + rng.normal(0, 1e-6, (N17, k))).astype(np.float32)
    Q = (c[rng.integers(0, 2, m)] + rng.normal(0, 1e-6, (m, k))).astype(np.float32)
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        want = topk_keys(Q, R, k, 64)
        for K in (1, 17, 64):
            np.testing.assert_array_equal(_topk(ix, Q, K), want[:, :K], err_msg=f"K={K}")
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 1, st
    finally:
        ix.close()


def test_out_of_box_rows_appear_in_the_answer_once():
    """Rows outside the filter's robust box on the pruned path: they sit in the layout with a +INF norm, never pass the scan, and
    reach the candidates through knn_topk_outlier_kernel — once (the re-rank skips their positions; pushed there as well they stood
    in a list twice and displaced the K-th key).  A tight cluster, 64 rows spread over the unit box and 8 rows planted beyond every
    other row in every coordinate: per coordinate the box is an interval around the centre, so if ANY row is outside it
    (st[3] > 0) the planted ones are.  Queries in the corner beside them: all 8 planted rows are among their 64 nearest."""
    rng = np.random.default_rng(48)
    k, m = 16, 48
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    R[:64] = rng.random((64, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Q[:24] = (0.97 + 0.03 * rng.random((24, k))).astype(np.float32)
    planted = np.arange(8)
    R[planted] = (1.2 + 0.1 * rng.random((8, k))).astype(np.float32)
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=9)
    try:
        want = topk_keys(Q, R, k, 64, base=9)
        assert all(set(planted + 9) <= set(keys_index(want[q])) for q in range(24))     # the case is what it says
        for K in (8, 64):
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 4 and st[3] > 0, st
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"K={K}")
            for q in range(24):
                row = keys_index(got[q])
                assert len(set(row)) == K                                            # no row twice
                assert K < 64 or set(planted + 9) <= set(row)
                assert np.isin(row, planted + 9).any()
    finally:
        ix.close()


def test_empty_corner_query_and_fewer_real_rows_than_k():
    """A clustered set and queries in an empty corner: the seed cells hold fewer than K rows (the wide sample is merged in).  And a
    shard with fewer finite rows than K: the list ends in KEY_INIT.  That second case cannot reach the pruned path and is asserted
    on the path it takes (1): a cell-sorted layout needs 2^17 rows, and the filter is ruled out when more than n / 32 of them lie
    outside its box or are not finite — a shard with a layout always holds more than K rows that can be candidates, so on the
    pruned path neither the select's KEY_INIT padding nor a +INF K-th seed score over the WHOLE shard can be constructed."""
    rng = np.random.default_rng(48)
    k, m = 16, 48
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    R[:64] = rng.random((64, k), dtype=np.float32)          # a few rows spread over the unit box: the cuts see a box
    Q = rng.random((m, k), dtype=np.float32)
    Q[:24] = (0.97 + 0.03 * rng.random((24, k))).astype(np.float32)
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        got = _topk(ix, Q, 64)
        st = ix.last_stats()
        assert st[0] == 4, st
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, 64))
    finally:
        ix.close()
    R2 = np.full((N17, k), np.nan, dtype=np.float32)
    R2[:40] = rng.random((40, k), dtype=np.float32)
    for name in ("path", "cells", "cells_rows", "cells_centre"):      # library policy for this build; topk_cells stays 1
        pkg.set_option(name, 0)
    ix = pkg.KnnIndex(k, R2)
    try:
        got = _topk(ix, Q, 64)
        assert ix.last_stats()[0] == 1, ix.last_stats()
        np.testing.assert_array_equal(got, topk_keys(Q, R2, k, 64))
        assert (got[:, 40:] == KEY_INIT).all() and (got[:, :40] < KEY_INIT).all()
    finally:
        ix.close()


def test_folds_merges_two_passes_and_alternating_calls():
    rng = np.random.default_rng(49)
    k = 16
    n = 2 * N17
    R = rng.random((n, k), dtype=np.float32)
    R[N17 + 500:N17 + 550] = R[100:150]          # equal distances across the two shards: the lower global number wins
    m = 1024 + 333
    Q = rng.random((m, k), dtype=np.float32)
    Q[:5] = R[100:105]
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    a = pkg.KnnIndex(k, R[:N17], base_index=0)
    b = pkg.KnnIndex(k, R[N17:], base_index=N17)
    try:
        want_a = topk_keys(Q, R[:N17], k, 64, base=0)
        want_b = topk_keys(Q, R[N17:], k, 64, base=N17)
        want_all = np.sort(np.concatenate([want_a, want_b], axis=1), axis=1)[:, :64]   # the union's K smallest
        for K in (8, 64):
            want = want_all[:, :K]
            keys = _keys(m, K)
            _topk(b, Q, K, keys=keys, init=True)
            assert b.last_stats()[0] == 4
            got = _topk(a, Q, K, keys=keys, init=False)
            st = a.last_stats()
            assert st[0] == 4 and st[2] == 0, st
            np.testing.assert_array_equal(got, want, err_msg=f"fold K={K}")
            ka, kb = _keys(m, K), _keys(m, K)
            _topk(a, Q, K, keys=ka)
            _topk(b, Q, K, keys=kb)
            pkg.keys_topk_merge(ka.data_ptr(), kb.data_ptr(), m, K)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_host(kb, m, K), want, err_msg=f"merge K={K}")
        # two passes, a far-away query in the second only: the first pass stays pruned-exact, the second falls back
        Qfar = Q.copy()
        Qfar[1024 + 7] = 1e6
        got = _topk(a, Qfar, 8)
        st = a.last_stats()
        assert st[0] == 4 and st[2] == 1, st
        want_far = want_a[:, :8].copy()
        want_far[1024 + 7] = topk_keys(Qfar[1024 + 7], R[:N17], k, 8)[0]
        np.testing.assert_array_equal(got, want_far)
        # 1-NN and top-K alternating on one slot
        Qs = Q[:200]
        want8 = want_a[:200, :8]
        for _ in range(3):
            one = _one_nn(a, Qs)
            assert a.last_stats()[0] == 4
            np.testing.assert_array_equal(one, want8[:, 0])
            np.testing.assert_array_equal(_topk(a, Qs, 8), want8)
            st = a.last_stats()
            assert st[0] == 4 and st[2] == 0, st
    finally:
        a.close()
        b.close()


def test_two_slots_in_flight_on_two_streams():
    rng = np.random.default_rng(50)
    k, m, K = 16, 200, 17
    R = rng.random((N17, k), dtype=np.float32)
    Qs = [rng.random((m, k), dtype=np.float32) for _ in range(2)]
    _set(BINS)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=5)
    dev = _dev()
    try:
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        q_d = [torch.from_numpy(Q.reshape(-1)).to(dev) for Q in Qs]
        keys = [_keys(m, K) for _ in range(2)]
        torch.cuda.synchronize()
        for s in range(2):
            ix.query_topk(m, K, q_d[s].data_ptr(), keys[s].data_ptr(), stream=streams[s].cuda_stream, slot=s, init_keys=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[0] == 4
        for s in range(2):
            np.testing.assert_array_equal(_host(keys[s], m, K), topk_keys(Qs[s], R, k, K, base=5))
    finally:
        ix.close()


def _torch_topk_keys(q_d, r_d, k, K, chunk=1 << 20):
    """tests/topk_oracle.py's arithmetic with torch's element-wise float32 kernels (one rounding per operation, never fused), the
    rows in chunks: int64 keys [m][K] ascending.  Checked against topk_keys itself on a sample of the queries by the caller."""
    m, n = q_d.shape[0], r_d.shape[0]
    best = torch.full((m, K), int(KEY_INIT), dtype=torch.int64, device=q_d.device)
    inf_bits = 0x7F800000
    for r0 in range(0, n, chunk):
        rc = r_d[r0:r0 + chunk]
        d = torch.zeros((m, rc.shape[0]), dtype=torch.float32, device=q_d.device)
        for j in range(k):
            diff = q_d[:, j:j + 1] - rc[None, :, j]
            sq = diff * diff
            d = d + sq
        bits = d.view(torch.int32).to(torch.int64)
        keys = (bits << 32) | torch.arange(r0, r0 + rc.shape[0], dtype=torch.int64, device=q_d.device)[None, :]
        keys[~(d < float("inf"))] = (inf_bits << 32) | 0xFFFFFFFF   # never below a real candidate of the oracle's form
        part = torch.topk(keys, K, dim=1, largest=False).values
        best = torch.sort(torch.cat([best, part], dim=1), dim=1).values[:, :K]
        del d, bits, keys
    best[best >= (inf_bits << 32)] = int(KEY_INIT)
    return best


def test_c3_full_shape_default_index_every_query_against_the_oracle():
    """C3's shape (k 16, m 1024, n 2^24) on the index a user gets by default (8-bit rows in bin frames), K 8, `topk_cells` = 1 (the
    policy declines for now): pruned, no fallback, every query's keys against v0's arithmetic."""
    k, m, n, K = 16, 1024, 1 << 24, 8
    dev = _dev()
    r_d = torch.empty(n * k, dtype=torch.float32, device=dev)
    q_d = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(r_d.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(q_d.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    try:
        keys = _keys(m, K)
        ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=True)
        torch.cuda.synchronize()
        st = ix.last_stats()
        assert st[0] == 4 and st[2] == 0, st
        want = _torch_topk_keys(q_d.view(m, k), r_d.view(n, k), k, K)
        got = keys.view(m, K)
        assert torch.equal(got, want), torch.nonzero((got != want).any(dim=1)).reshape(-1)[:8]
        # the torch restatement against tests/topk_oracle.py on a few queries and the rows of the first 2^20
        sub = topk_keys(q_d.view(m, k)[:4].cpu().numpy(), r_d.view(n, k)[: 1 << 20].cpu().numpy(), k, K)
        mine = _torch_topk_keys(q_d.view(m, k)[:4], r_d.view(n, k)[: 1 << 20], k, K)
        np.testing.assert_array_equal(mine.cpu().numpy().view(np.uint64), sub)
    finally:
        ix.close()
