"""The bin-frame 8-bit scan under both item deals (option `scan_deal`: 1 fixed, 2 block counter), on batches whose cells
list one query, 32, 33 or 385 copies of one (a list longer than its room is scored dense), and on a batch the 8-bit scores
cannot separate (the record areas over-fill).  Bar: bit-exact against the CPU oracle, ties to the lowest index."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.test_cells_gpu import THREADS, _off_the_cube, _query

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _bin_frames():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    pkg.set_option("cells_rows", 2)
    pkg.set_option("cells_u8_frame", 2)
    pkg.set_option("path", 2)
    pkg.set_option("cells", 1)
    yield
    for name in ("path", "cells", "cells_rows", "cells_u8_frame", "scan_deal"):
        pkg.set_option(name, 0)


def _run(oracle, k, Q, R, deal):
    want = oracle.v0(k, Q, R, threads=THREADS)
    pkg.set_option("scan_deal", deal)
    before = pkg.get_option("cells_u8_bin_builds")
    ix = pkg.KnnIndex(k, R)
    try:
        assert pkg.get_option("cells_u8_bin_builds") == before + 1
        got, st = _query(ix, Q)
    finally:
        ix.close()
    np.testing.assert_array_equal(got, want, err_msg=f"deal={deal} stats={st}")
    return st


def _copies(rng, k, sizes):
    pts = rng.random((len(sizes), k), dtype=np.float32)
    return np.ascontiguousarray(np.repeat(pts, sizes, axis=0), dtype=np.float32)


@pytest.mark.parametrize("deal", [1, 2])
@pytest.mark.parametrize("n", [(1 << 17) + 1234, (1 << 19) + 1234])
def test_lists_of_copies(oracle, deal, n):
    rng = np.random.default_rng(n % 1000 + deal)
    k = 16
    R = rng.random((n, k), dtype=np.float32)
    Q = _copies(rng, k, [1, 32, 33, 385])
    st = _run(oracle, k, Q, R, deal)
    assert st[0] == 4, st


@pytest.mark.parametrize("deal", [1, 2])
def test_batch_the_scores_cannot_separate(oracle, deal):
    rng = np.random.default_rng(40 + deal)
    Q, R = _off_the_cube(rng, "tight_clusters", 16, 1024, 1 << 19)
    _run(oracle, 16, Q, R, deal)
