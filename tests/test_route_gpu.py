"""Which path answers a call (knn_query_route), on the GPU: for each index below, one call per option setting, the path the
library reports (knn_index_last_stats()[0]) against the route restated in tests/test_route_logic.py, and the answers against the
oracle — 1-NN keys bit-exact against v0, top-K through tests/topk_oracle.py.  The sizes are the smallest each path is built for."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.test_route_logic import CELLS, EXACT, FILTER, GRID, _route
from tests.topk_oracle import KEY_INIT, keys_index, topk_keys

pytestmark = pytest.mark.gpu
OPTIONS = ("path", "cells", "cells_rows", "cells_centre", "topk_cells")
N17 = 1 << 17      # the smallest shard a cell-sorted layout is built for
BASE = 5


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _dev():
    return torch.device("cuda:0")


def _one_nn(ix, Q, init_keys=True):
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    keys = torch.empty(m, dtype=torch.int64, device=_dev())
    ind = torch.full((m,), -7, dtype=torch.int32, device=_dev())
    if not init_keys:
        pkg.keys_init(keys.data_ptr(), m)
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), init_keys=init_keys, indices_dev=ind.data_ptr())
    torch.cuda.synchronize()
    got = keys.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(ind.cpu().numpy(), keys_index(got))
    return got


def _topk(ix, Q, K):
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(_dev())
    keys = torch.empty(m * K, dtype=torch.int64, device=_dev())
    ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=True)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64).reshape(m, K)


def _way(ix, K, m, filter_usable=1, has_cells=0, centred=0, has_grid=0, filter_wanted=0, init_keys=1):
    """The route restated, for index ix under the options as they stand (fp16 rows: cells_rows = 1 at every build here)."""
    return _route(ix.k, K, m, ix.n, pkg.get_option("path"), pkg.get_option("cells"), pkg.get_option("topk_cells"), filter_usable,
                  has_cells, centred, 0, 0, has_grid, 0, filter_wanted, 0, init_keys)[0]


@pytest.fixture(scope="module")
def rows8(oracle):
    rng = np.random.default_rng(817)
    R = rng.random((N17, 8), dtype=np.float32)
    Q = rng.random((1025, 8), dtype=np.float32)
    return R, Q, oracle.v0_keys(8, Q, R, base=BASE), topk_keys(Q[:5], R, 8, 8, base=BASE)


@pytest.fixture(scope="module", params=[2, 1], ids=["shard_frame", "centred"])
def cells8(request, rows8):
    """k 8, 2^17 rows, `cells` = 1 at the build: fp16 rows in the shard's one frame, or in per-cell frames."""
    for name, v in (("cells", 1), ("cells_rows", 1), ("cells_centre", request.param)):
        pkg.set_option(name, v)
    centred_before = pkg.get_option("cells_centred_builds")
    ix = pkg.KnnIndex(8, rows8[0], base_index=BASE)
    centred = pkg.get_option("cells_centred_builds") - centred_before
    for name in OPTIONS:
        pkg.set_option(name, 0)
    assert centred == (request.param == 1)
    yield ix, centred
    ix.close()


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("cells", [0, 2])
def test_cells_index_one_nn_goes_where_the_route_says(cells8, rows8, cells, path):
    ix, centred = cells8
    R, Q, want, _ = rows8
    pkg.set_option("cells", cells)
    pkg.set_option("path", path)
    ways = {}
    for m in (1, 4, 5, 1025):
        got = _one_nn(ix, Q[:m])
        ways[m] = ix.last_stats()[0]
        assert ways[m] == _way(ix, 0, m, has_cells=1, centred=centred), (cells, path, m, ways)
        np.testing.assert_array_equal(got, want[:m], err_msg=f"cells {cells} path {path} m {m}")
    if path == 1:
        assert set(ways.values()) == {EXACT}
    elif cells == 0:
        assert set(ways.values()) == {CELLS}
    elif centred:      # per-cell frames under `cells` = 2: no full scan can read them (the route's known oddity at path 0)
        assert ways == ({1: EXACT, 4: EXACT, 5: CELLS, 1025: CELLS} if path == 0 else dict.fromkeys(ways, CELLS))
    else:
        assert ways == ({1: EXACT, 4: EXACT, 5: FILTER, 1025: FILTER} if path == 0 else dict.fromkeys(ways, FILTER))


@pytest.mark.parametrize("topk_cells", [0, 1])
def test_cells_index_topk_goes_where_the_route_says(cells8, rows8, topk_cells):
    ix, centred = cells8
    R, Q, _, want = rows8
    pkg.set_option("topk_cells", topk_cells)
    for m in (4, 5):
        got = _topk(ix, Q[:m], 8)
        st = ix.last_stats()
        assert st[0] == _way(ix, 8, m, has_cells=1, centred=centred), (topk_cells, m, st)
        # m 4: too few queries for a filter; per-cell frames: the exact top-K; else the pruned scan on request, the full scan by policy
        assert st[0] == (EXACT if m == 4 or centred else CELLS if topk_cells == 1 else FILTER)
        if st[0] != EXACT:
            assert st[3] == 0      # (no out-of-box rows on uniform data: what _way assumes)
        np.testing.assert_array_equal(got, want[:m], err_msg=f"topk_cells {topk_cells} m {m}")


def test_grid_index_serves_path_0_and_the_exact_scan_path_1_and_topk(oracle):
    rng = np.random.default_rng(33)
    k, n, m = 3, 16384, 64
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    want = oracle.v0_keys(k, Q, R, base=BASE)
    ix = pkg.KnnIndex(k, R, base_index=BASE)      # (k <= 4, >= 16384 rows: the grid index, and no filter layouts beside it)
    try:
        for path, way in ((0, GRID), (1, EXACT)):
            pkg.set_option("path", path)
            for init_keys in (True, False):
                got = _one_nn(ix, Q, init_keys=init_keys)
                assert ix.last_stats()[0] == way == _way(ix, 0, m, filter_usable=0, has_grid=1), (path, ix.last_stats())
                np.testing.assert_array_equal(got, want, err_msg=f"path {path}")
        pkg.set_option("path", 0)
        got = _topk(ix, Q, 8)
        assert ix.last_stats()[0] == EXACT == _way(ix, 8, m, filter_usable=0, has_grid=1)
        np.testing.assert_array_equal(got, topk_keys(Q, R, k, 8, base=BASE))
    finally:
        ix.close()


def test_filter_asked_for_below_the_size_rule_is_taken_from_five_queries(oracle):
    rng = np.random.default_rng(40)
    k, n = 40, 4096
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((5, k), dtype=np.float32)
    want = oracle.v0_keys(k, Q, R, base=BASE)
    ix = pkg.KnnIndex(k, R, base_index=BASE)      # (32 < k: the library builds the filter layouts from 4096 rows, filter_wanted)
    try:
        for m, way in ((4, EXACT), (5, FILTER)):
            both = []
            for init_keys in (True, False):
                both.append(_one_nn(ix, Q[:m], init_keys=init_keys))
                assert ix.last_stats()[0] == way == _way(ix, 0, m, filter_wanted=1, init_keys=init_keys), (m, ix.last_stats())
            np.testing.assert_array_equal(both[0], both[1])
            np.testing.assert_array_equal(both[0], want[:m], err_msg=f"m {m}")
    finally:
        ix.close()


def test_empty_shard_leaves_init_keys():
    ix = pkg.KnnIndex(8, np.empty(0, dtype=np.float32), n_local=0, base_index=BASE)
    try:
        Q = np.random.default_rng(1).random((7, 8), dtype=np.float32)
        assert (_one_nn(ix, Q) == KEY_INIT).all()
        assert (_topk(ix, Q, 8) == KEY_INIT).all()
    finally:
        ix.close()
