"""Top-K on the cell-pruned scan for layouts in per-cell frames (KNN_QUERY_TOPK_FRAMES with option `topk_cells` = 1; DESIGN §4.6
"Per-cell frames") on the GPU against the numpy restatement of v0 (tests/topk_oracle.py).  Bar: bit-exact keys, in order.
"Pruned" means knn_index_last_stats()[0] == 4.  The two layouts: fp16 rows centred per cell (`cells_centre` 1) and 8-bit rows in
each cell's own frame (`cells_rows` 2, `cells_u8_frame` 1)."""
import ctypes

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import keys_index, topk_keys

pytestmark = pytest.mark.gpu
OPTIONS = ("path", "cells", "cells_rows", "cells_centre", "cells_u8_frame", "scan_deal", "topk_cells")
N17 = (1 << 17) + 999          # the smallest shard that gets a cell-sorted layout under `cells` 1: 512 cells
CENTRED = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 1}
U8CELL = {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 1}
FP16 = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2}
LAYOUTS = [("centred_fp16", CENTRED), ("per_cell_u8", U8CELL)]
LAYOUT_IDS = [name for name, _ in LAYOUTS]


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _dev():
    return torch.device("cuda:0")


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


def _keys(m, K):
    return torch.empty(m * K, dtype=torch.int64, device=_dev())


def _host(keys, m, K):
    return keys.cpu().numpy().view(np.uint64).reshape(m, K)


def _topk(ix, Q, K, frames=True, keys=None, init=True, slot=0, stream=0):
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    if keys is None:
        keys = _keys(m, K)
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=_dev())
    ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=init, indices_dev=ind.data_ptr(), slot=slot, stream=stream,
                  frames=frames)
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


def _clusters(rng, k, m, n, nclusters, width):
    c = rng.random((nclusters, k), dtype=np.float32)
    R = (c[rng.integers(0, nclusters, n)] + rng.normal(0, width, (n, k))).astype(np.float32)
    Q = (c[rng.integers(0, nclusters, m)] + rng.normal(0, width, (m, k))).astype(np.float32)
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


# ---- 1. the flag is the only way in ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_the_flag_is_the_only_way_in(name, opts):
    rng = np.random.default_rng(101)
    k, m, K = 8, 40, 8
    R = rng.random((N17, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    want = topk_keys(Q, R, k, K)
    _set(opts)
    ix = pkg.KnnIndex(k, R)
    try:
        pkg.set_option("topk_cells", 1)
        np.testing.assert_array_equal(_topk(ix, Q, K, frames=False), want)
        assert ix.last_stats()[0] == 1, ix.last_stats()             # the option without the flag: the exact top-K, as before
        for v in (0, 2):
            pkg.set_option("topk_cells", v)
            np.testing.assert_array_equal(_topk(ix, Q, K, frames=True), want)
            assert ix.last_stats()[0] == 1, (v, ix.last_stats())    # the flag without the option
        pkg.set_option("topk_cells", 1)
        np.testing.assert_array_equal(_topk(ix, Q, K, frames=True), want)
        assert ix.last_stats()[0] == 4, ix.last_stats()             # both
        # with a real index and real buffers: 16 is no flag of the top-K entry, 8 none of the 1-NN entries' (KNN_EINVAL, nothing runs)
        L = pkg.lib()
        q_d = torch.from_numpy(Q.reshape(-1)).to(_dev())
        keys = _keys(m, K)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        assert L.knn_index_query_topk(ix._h, 0, m, K, vp(q_d), vp(keys), None, None, 16 | pkg.QUERY_INIT_KEYS) != 0
        assert L.knn_index_query_topk(ix._h, 0, m, K, vp(q_d), vp(keys), None, None, 15) == 0      # all four flags together
        assert L.knn_index_query(ix._h, 0, m, vp(q_d), vp(keys), None, None, pkg.QUERY_TOPK_FRAMES | pkg.QUERY_INIT_KEYS) != 0
        assert L.knn_index_query_keys_ex(ix._h, 0, m, vp(q_d), vp(keys), None, pkg.QUERY_TOPK_FRAMES | pkg.QUERY_INIT_KEYS) != 0
        assert L.knn_index_query(ix._h, 0, m, vp(q_d), vp(keys), None, None, pkg.QUERY_INIT_KEYS) == 0
        torch.cuda.synchronize()
    finally:
        ix.close()


def test_the_flag_changes_nothing_on_other_indexes():
    rng = np.random.default_rng(102)
    m, K = 40, 8
    # an fp16 layout in the shard's frame under topk_cells 1: pruned with and without the flag
    k = 8
    R = rng.random((N17, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    want = topk_keys(Q, R, k, K)
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        for frames in (False, True):
            np.testing.assert_array_equal(_topk(ix, Q, K, frames=frames), want)
            assert ix.last_stats()[0] == 4, (frames, ix.last_stats())
    finally:
        ix.close()
    for name in OPTIONS:
        pkg.set_option(name, 0)
    pkg.set_option("topk_cells", 1)
    # a dense-layout index (no cell-sorted layout at this size) and a grid index (k 3): the same path either way
    for k, n in ((8, 70000), (3, 1 << 16)):
        R = rng.random((n, k), dtype=np.float32)
        Q = rng.random((m, k), dtype=np.float32)
        want = topk_keys(Q, R, k, K)
        ix = pkg.KnnIndex(k, R)
        try:
            ways = []
            for frames in (False, True):
                np.testing.assert_array_equal(_topk(ix, Q, K, frames=frames), want)
                ways.append(ix.last_stats()[0])
            assert ways[0] == ways[1] and ways[0] != 4, (k, ways)
        finally:
            ix.close()


# ---- 2. every new form, no fallback ----------------------------------------------------------------------------------------------

FORMS = [
    ("centred_k16_fixed", 16, dict(CENTRED, scan_deal=1)),
    ("centred_k16_counter", 16, dict(CENTRED, scan_deal=2)),
    ("centred_k8_fixed", 8, dict(CENTRED, scan_deal=1)),
    ("centred_k8_counter", 8, dict(CENTRED, scan_deal=2)),
    ("u8_k16", 16, U8CELL),
    ("u8_k5", 5, U8CELL),
]


@pytest.mark.parametrize("name,k,opts", FORMS, ids=[f[0] for f in FORMS])
def test_every_new_form_is_bit_exact_without_fallback(name, k, opts):
    """Uniform rows, 512 cells of ~256 rows: pruned, records handed on, and NO fallback — the shard-frame forms hold the same line at
    this shape, and a cell's own frame only tightens the scores."""
    rng = np.random.default_rng(N17 + k)
    m = 96
    R = rng.random((N17, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=11)
    try:
        want = topk_keys(Q, R, k, 64, base=11)
        for K in (1, 2, 8, 17, 64):
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 4 and st[1] > 0 and st[2] == 0, (name, K, st)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{name} K={K}")
        one = _one_nn(ix, Q)
        assert ix.last_stats()[0] == 4
        np.testing.assert_array_equal(_topk(ix, Q, 1)[:, 0], one)
    finally:
        ix.close()


# ---- 3. clustered rows: the case the feature exists for --------------------------------------------------------------------------

@pytest.mark.parametrize("width", [1e-2, 1e-3])
@pytest.mark.parametrize("name,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_clustered_rows(name, opts, width):
    """64 blobs; at width 1e-3 the cells' frames are at full scale (2^8).  K <= 8: no fallback — candidates per query are about
    K x (rows of the query's cluster) / (seed rows scored), tens to a few hundred, against a room of 4096 + 128 K keys and a pass
    limit of 2^21 records.  K = 64: reported, not asserted."""
    rng = np.random.default_rng(int(1 / width))
    k, m = 16, 96
    Q, R = _clusters(rng, k, m, N17, 64, width)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        want = topk_keys(Q, R, k, 64)
        for K in (1, 8, 64):
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            print(f"clusters64 width {width} {name} K {K}: stats {st}")
            assert st[0] == 4, (K, st)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{name} width={width} K={K}")
            if K <= 8:
                assert st[2] == 0, (K, st)
    finally:
        ix.close()


def test_the_librarys_own_build_for_clustered_rows():
    """k 8, n 2^19 + 77 (the size rule for k 8), no build option: the build's sample sees the clustering and the layout gets
    per-cell frames; only `topk_cells` 1 and the flag are set."""
    rng = np.random.default_rng(303)
    k, m, n = 8, 96, (1 << 19) + 77
    Q, R = _clusters(rng, k, m, n, 64, 1e-3)
    before = pkg.get_option("cells_centred_builds")
    ix = pkg.KnnIndex(k, R)
    try:
        assert pkg.get_option("cells_centred_builds") == before + 1
        pkg.set_option("topk_cells", 1)
        got = _topk(ix, Q, 8)
        st = ix.last_stats()
        assert st[0] == 4, st
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, 8, chunk=16))
    finally:
        ix.close()


# ---- 4. queries a cell's frame cannot hold, and queries nothing bounds -----------------------------------------------------------

@pytest.mark.parametrize("name,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_far_queries_and_a_query_nothing_bounds(name, opts):
    """Tight clusters (16 blobs of width 2e-4: frames at full scale) and queries 20 and 100 box widths away: they fit no cell's
    frame (beyond CELL_FRAME_AMAX cell units), so the prep kernel's far branch runs inside the top-K form; inside the shard's
    amax limit, so the batch is not sent away.  A NaN coordinate: FALLBACK once, every other query still exact; the same batch
    without the NaN, right before and right after on the slot, is pruned without it."""
    rng = np.random.default_rng(404)
    k, m = 16, 64
    Q, R = _clusters(rng, k, m, N17, 16, 2e-4)
    Q[3] = 20.0
    Q[4, :] = 0.5
    Q[4, 7] = 100.0
    Q[5] = -20.0
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=4)
    try:
        wants = {}
        for K in (1, 8, 64):
            wants[K] = topk_keys(Q, R, k, K, base=4)
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            print(f"far queries {name} K {K}: stats {st}")
            assert st[0] == 4, st
            np.testing.assert_array_equal(got, wants[K], err_msg=f"{name} far K={K}")
        # The query nothing bounds, on batches that do NOT fall back on their own (asserted right before and right after), so that
        # st[2] == 1 is the prep form's doing: the far batch at K 64 (the far branch's bounds stand: 12288 candidate keys hold what
        # they admit; at K 1 and 8 the same batch falls back), and the batch without its far queries at K 8.
        near = np.delete(np.arange(m), (3, 4, 5))
        for K, rows in ((64, np.arange(m)), (8, near)):
            Qb, want = Q[rows], wants[K][rows]
            got = _topk(ix, Qb, K)
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, (K, st)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} before NaN K={K}")
            Qnan = Qb.copy()
            Qnan[9, 2] = np.nan
            got = _topk(ix, Qnan, K)
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 1, (K, st)
            others = np.arange(len(rows)) != 9
            np.testing.assert_array_equal(got[others], want[others], err_msg=f"{name} NaN batch K={K}")
            got = _topk(ix, Qb, K)                      # the next clean batch on the slot
            st = ix.last_stats()
            assert st[0] == 4 and st[2] == 0, (K, st)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} after NaN K={K}")
    finally:
        ix.close()


# ---- 5. fewer than K seed rows ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_empty_corner_queries_take_the_wide_sample_in_per_tile_frames(name, opts):
    """A tight block plus 64 rows spread over the unit box, queries in an empty corner: the seed cells hold fewer than 64 rows, so
    the 64 tiles spread over the layout — each scored in its own cell's frame — are merged in."""
    rng = np.random.default_rng(48)
    k, m = 16, 48
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    R[:64] = rng.random((64, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Q[:24] = (0.97 + 0.03 * rng.random((24, k))).astype(np.float32)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        got = _topk(ix, Q, 64)
        st = ix.last_stats()
        print(f"empty corner {name}: stats {st}")
        assert st[0] == 4, st
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, 64))
    finally:
        ix.close()


# ---- 6. out-of-box rows appear once ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_out_of_box_rows_appear_in_the_answer_once(name, opts):
    """tests/test_cells_topk_gpu.py's planted-rows construction on per-cell frames: the rows outside the robust box keep their +INF
    norm through the recentring (the re-rank skips their positions) and reach the lists through the outlier launch — once."""
    rng = np.random.default_rng(48)
    k, m = 16, 48
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    R[:64] = rng.random((64, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Q[:24] = (0.97 + 0.03 * rng.random((24, k))).astype(np.float32)
    planted = np.arange(8)
    R[planted] = (1.2 + 0.1 * rng.random((8, k))).astype(np.float32)
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R, base_index=9)
    try:
        want = topk_keys(Q, R, k, 64, base=9)
        assert all(set(planted + 9) <= set(keys_index(want[q])) for q in range(24))     # the case is what it says
        for K in (8, 64):
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            assert st[0] == 4 and st[3] > 0, st
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{name} K={K}")
            for q in range(24):
                row = keys_index(got[q])
                assert len(set(row)) == K                                            # no row twice
                assert K < 64 or set(planted + 9) <= set(row)
    finally:
        ix.close()


# ---- 7. over-full pass -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_clusters_tighter_than_a_cells_fp16_step(name, opts):
    """Two clusters of normal(0, 1e-9) about a point: either the cell's own frame separates the rows or the pass is over-full and
    the exact top-K answers.  Either way the keys are exact."""
    rng = np.random.default_rng(46)
    k, m = 16, 40
    c = rng.random((2, k), dtype=np.float32)
    R = (c[rng.integers(0, 2, N17)] + rng.normal(0, 1e-9, (N17, k))).astype(np.float32)
    Q = (c[rng.integers(0, 2, m)] + rng.normal(0, 1e-9, (m, k))).astype(np.float32)
    assert len(np.unique(R, axis=0)) > 2                        # not all identical in fp32
    _set(opts)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    try:
        want = topk_keys(Q, R, k, 64)
        for K in (1, 64):
            got = _topk(ix, Q, K)
            st = ix.last_stats()
            print(f"tight clusters {name} K {K}: stats {st} ->", "the exact top-K answered" if st[2] else "the frames separate them")
            assert st[0] == 4 and st[2] in (0, 1), st
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{name} K={K}")
    finally:
        ix.close()


# ---- 8. folds, two passes, alternation -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,opts", LAYOUTS, ids=LAYOUT_IDS)
def test_folds_two_passes_alternating_calls_and_another_slot(name, opts):
    rng = np.random.default_rng(49)
    k = 16
    n = 2 * N17
    R = rng.random((n, k), dtype=np.float32)
    R[N17 + 500:N17 + 550] = R[100:150]          # equal distances across the two halves: the lower global number wins
    m = 1024 + 333
    Q = rng.random((m, k), dtype=np.float32)
    Q[:5] = R[100:105]
    _set(opts)
    pkg.set_option("topk_cells", 1)
    a = pkg.KnnIndex(k, R[:N17], base_index=0)
    b = pkg.KnnIndex(k, R[N17:], base_index=N17)
    try:
        want_a = topk_keys(Q, R[:N17], k, 64, base=0)
        want_b = topk_keys(Q, R[N17:], k, 64, base=N17)
        want_all = np.sort(np.concatenate([want_a, want_b], axis=1), axis=1)[:, :64]   # the union's K smallest
        for K in (8, 64):
            keys = _keys(m, K)
            _topk(b, Q, K, keys=keys, init=True)
            assert b.last_stats()[0] == 4
            got = _topk(a, Q, K, keys=keys, init=False)
            st = a.last_stats()
            assert st[0] == 4 and st[2] == 0, st
            np.testing.assert_array_equal(got, want_all[:, :K], err_msg=f"{name} fold K={K}")
        Qs = Q[:200]
        want8 = want_a[:200, :8]
        for _ in range(2):                        # 1-NN and top-K alternating on one slot
            one = _one_nn(a, Qs)
            assert a.last_stats()[0] == 4
            np.testing.assert_array_equal(one, want8[:, 0])
            np.testing.assert_array_equal(_topk(a, Qs, 8), want8)
            st = a.last_stats()
            assert st[0] == 4 and st[2] == 0, st
        stream = torch.cuda.Stream(device=_dev())   # slot 3 on its own stream
        torch.cuda.synchronize()
        got = _topk(a, Qs, 8, slot=3, stream=stream.cuda_stream)
        assert a.last_stats()[0] == 4
        np.testing.assert_array_equal(got, want8)
    finally:
        a.close()
        b.close()
