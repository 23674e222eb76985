"""knn_index_list_within on the cell-pruned scan (KNN_QUERY_COUNT_CELLS; DESIGN §4.6, "Lists within a radius") on the GPU against
tests/list_oracle.py, on the shapes and option sets of tests/test_count_cells_gpu.py.  Bar: exact lists and fill at every radius;
"pruned" means knn_index_last_stats()[0] == 4, [2] != 0 a pass that fell back and was answered by the exact list."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import dev, dev_counts
from tests.count_oracle import radii
from tests.list_helper import PAD, assert_lists, check_list, dev_u64, list_call, segments
from tests.list_oracle import holds_every_kind, kinds, lengths, lists_of, offsets_of
from tests.shards_helper import Shards
from tests.test_within_cells_gpu import BINS, CENTRED, FP16, MATRIX, N17, OPTIONS, spread_queries
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
PRUNED = ("at", "below", "zero", "under_all")     # the radii the pruned count stays pruned at: so must the list


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
def test_every_radius_is_exact_and_the_pruned_radii_stay_pruned(name, k, opts):
    rng = np.random.default_rng(N17 + 7 * k)
    m = 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    want = {rname: lists_of(d, r2, base=11) for rname, r2 in radii(d)}
    assert holds_every_kind(want.values()) and kinds(want["at"])[:2] == (True, True) and kinds(want["large"])[2]
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=11)
    try:
        for rname, r2 in radii(d):
            check_list(ix, Q, r2, want[rname], msg=f"{name} {rname} r2={r2}", cells=True)
            st = ix.last_stats()
            if rname in PRUNED:
                assert st[0] == 4 and st[2] == 0, (name, rname, st)
            elif rname == "inf":
                assert st[0] == 1, (name, st)          # +INF under the cell flag: no cap to prune with
            else:
                print(f"{name}: large radius r2={r2}: last_stats {st}, longest list {lengths(want[rname]).max()}")
        # without the flag the exact list answers; appending on the pruned way goes behind the cursor
        r2, w = radii(d)[0][1], want["at"]
        cnt = lengths(w)
        check_list(ix, Q, r2, w)
        assert ix.last_stats()[0] == 1
        held = (np.arange(m, dtype=np.uint32) % 5)
        off = offsets_of(cnt.astype(np.uint64) + held)
        fill, keys = list_call(ix, Q, r2, off, fill=dev_counts(m, fill=held), init=False, cells=True)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0
        np.testing.assert_array_equal(fill, held + cnt)
        for j in range(m):
            assert (keys[int(off[j]):int(off[j]) + int(held[j])] == PAD).all()
            np.testing.assert_array_equal(np.sort(keys[int(off[j]) + int(held[j]):int(off[j + 1])]), w[j])
        # an overflowing segment on the pruned way: fill is the count, nothing leaves the segment
        rooms = np.where(cnt > 0, cnt - 1, 0).astype(np.uint64)
        off = np.concatenate([[np.uint64(1)], np.uint64(1) + np.cumsum(rooms)]).astype(np.uint64)
        fill, keys = list_call(ix, Q, r2, off, keys=dev_u64(np.full(int(off[-1]) + 1, PAD)), cells=True)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0
        np.testing.assert_array_equal(fill, cnt)
        assert keys[0] == PAD and keys[-1] == PAD
        for j in range(m):
            got = keys[int(off[j]):int(off[j + 1])]
            assert np.isin(got, w[j]).all() and np.unique(got).size == got.size
        check_list(ix, Q[:4], r2, w[:4], cells=True)       # m < 5: the exact list
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
        rs = dict(radii(d))
        for rname in ("at", "large"):
            r2 = rs[rname]
            for init in (True, False):
                held = np.full(m, 3, np.uint32) if not init else np.zeros(m, np.uint32)
                for batch_d, Qb, fell in ((dfar, Qfar, 1), (d, Q, 0)):
                    want = lists_of(batch_d, r2, base=4)
                    cnt = lengths(want)
                    off = offsets_of(cnt.astype(np.uint64) + held)
                    fill, keys = list_call(ix, Qb, r2, off, fill=dev_counts(m, fill=np.full(m, 3, np.uint32)), init=init, cells=True)
                    st = ix.last_stats()
                    assert st[0] == 4 and (st[2] == fell or rname == "large"), (rname, st)
                    np.testing.assert_array_equal(fill, cnt + held, err_msg=f"{rname} fell={fell} init={init}: fill is exact, not doubled")
                    for j in range(m):
                        h = int(held[j])
                        assert (keys[int(off[j]):int(off[j]) + h] == PAD).all()
                        np.testing.assert_array_equal(np.sort(keys[int(off[j]) + h:int(off[j + 1])]), want[j],
                                                      err_msg=f"{rname} fell={fell} init={init} query {j}")
        far = lists_of(dfar, rs["at"], base=4)
        assert far[1].size == 0 and far[2].size == 0
        assert holds_every_kind([far, lists_of(dfar, rs["large"], base=4)])
    finally:
        ix.close()


def test_two_passes():
    """m = 1024 + 6: two passes of the pruned list.  (The batch repeats 96 queries: the oracle is computed once for them.)"""
    rng = np.random.default_rng(49)
    k, m, m0 = 16, 1024 + 6, 96
    R = rng.random((N17, k), dtype=np.float32)
    Q0 = spread_queries(rng, m0, k)
    rep = np.arange(m) % m0
    d = v0_dist2(Q0, R, k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        seen = []
        for rname, r2 in (radii(d)[0], radii(d)[1], radii(d)[5]):
            w0 = lists_of(d, r2)
            seen.append(w0)
            want = [w0[i] for i in rep]
            check_list(ix, Q0[rep], r2, want, msg=rname, cells=True)
            st = ix.last_stats()
            assert st[0] == 4 and (st[2] == 0 or rname == "large"), st
        assert holds_every_kind(seen)
    finally:
        ix.close()


def test_rows_outside_the_robust_box_appear_exactly_once():
    """The rows of tests/test_count_cells_gpu.py's out-of-box test: 51 of the 64 spread rows lie outside the filter's robust box
    ([3]) — they sit in the layout (norm +INF: the re-rank skips them) and in the outlier list (the outlier kernel lists them).
    Queries right beside each of the 64: the list of a radius that holds just that row has it once, not never and not twice."""
    rng = np.random.default_rng(48)
    k = 16
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    R[:64] = rng.random((64, k), dtype=np.float32)
    Q = (R[:64] + np.float32(1e-3) * rng.random((64, k), dtype=np.float32)).astype(np.float32)
    far = (0.45 + 0.1 * rng.random((6, k))).astype(np.float32)      # queries inside the cluster: long lists at the second radius
    Q = np.concatenate([Q, far])
    d = v0_dist2(Q, R, k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        own = float(d[np.arange(64), np.arange(64)].max())
        seen = []
        for r2 in (own, 10.0 * own, float(np.sort(d[64])[99])):
            want = lists_of(d, r2)
            seen.append(want)
            check_list(ix, Q, r2, want, msg=f"r2={r2}", cells=True)
            st = ix.last_stats()
            assert st[0] == 4 and st[3] == 51, st
        assert (lengths(seen[0])[:64] == 1).sum() >= 51 and holds_every_kind(seen)
    finally:
        ix.close()


def test_per_cell_frames_take_the_exact_list():
    rng = np.random.default_rng(52)
    k, m = 16, 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    _set(CENTRED)
    ix = pkg.KnnIndex(k, R, base_index=6)
    try:
        seen = []
        for rname, r2 in radii(d):
            want = lists_of(d, r2, base=6)
            seen.append(want)
            check_list(ix, Q, r2, want, msg=rname, cells=True)
            assert ix.last_stats()[0] == 1, (rname, ix.last_stats())
        assert holds_every_kind(seen)
    finally:
        ix.close()


@pytest.mark.parametrize("attach", [True, False], ids=["seed_layer_attached", "no_seed_layer"])
def test_a_cell_range_shard_pair_folds_to_the_global_lists(attach):
    rng = np.random.default_rng(26)
    k, n, m = 16, (1 << 19) + 5, 40
    R = rng.random((n, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q[:m], R, k)
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=attach)
    try:
        seen = []
        for rname, r2 in radii(d):
            if r2 == float("inf"):
                continue
            want = lists_of(d, r2)          # the keys carry global row numbers: the ranks' gids
            seen.append(want)
            off = offsets_of(lengths(want))
            fill_d = dev_counts(m, fill=0xDEADBEEF)
            keys_d = dev_u64(np.full(max(int(off[-1]), 1), PAD))
            for r, ix in enumerate(sh.idx):
                fill, keys = list_call(ix, Q, r2, off, fill=fill_d, keys=keys_d, init=(r == 0), cells=True)
                st = ix.last_stats()
                assert st[0] == 4, (r, rname, st)
                if rname != "large":
                    assert st[2] == 0, (r, rname, st)
            np.testing.assert_array_equal(fill, lengths(want), err_msg=rname)
            assert_lists(segments(off, fill, keys), want, rname)
            # the same fold on the exact list: gids there too
            for r, ix in enumerate(sh.idx):
                fill, keys = list_call(ix, Q, r2, off, fill=fill_d, keys=keys_d, init=(r == 0))
                assert ix.last_stats()[0] == 1
            np.testing.assert_array_equal(fill, lengths(want), err_msg=rname)
            assert_lists(segments(off, fill, keys), want, f"{rname} (exact)")
        assert holds_every_kind(seen)
        # each rank's list is its own rows'
        r2 = radii(d)[0][1]
        for r, ix in enumerate(sh.idx):
            own = lists_of(v0_dist2(Q, sh.rows[r].cpu().numpy(), k), r2, gids=sh.gids[r].cpu().numpy())
            check_list(ix, Q, r2, own, msg=f"rank {r}", cells=True)
    finally:
        sh.close()
