"""8-bit rows in per-dimension bin frames (option `cells_u8_frame` = 2: the layout stays in the shard's one frame, the scan takes a
per-query B operand and a per-(query, cell) pair term) against the CPU oracle.  Bar: bit-exact, ties to the lowest index."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.test_cells_gpu import THREADS, _cases, _off_the_cube, _query

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _bin_frames():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    pkg.set_option("cells_rows", 2)
    pkg.set_option("cells_u8_frame", 2)
    yield
    for name in ("path", "cells", "cells_rows", "cells_centre", "cells_u8_frame"):
        pkg.set_option(name, 0)


def _run(oracle, k, Q, R):
    want = oracle.v0(k, Q, R, threads=THREADS)
    pkg.set_option("path", 2)
    pkg.set_option("cells", 1)
    before = pkg.get_option("cells_u8_builds"), pkg.get_option("cells_u8_bin_builds")
    ix = pkg.KnnIndex(k, R, base_index=7)
    try:
        assert (pkg.get_option("cells_u8_builds"), pkg.get_option("cells_u8_bin_builds")) == (before[0] + 1, before[1] + 1)
        got, st = _query(ix, Q)
        again, _ = _query(ix, Q)
    finally:
        ix.close()
    np.testing.assert_array_equal(got - 7, want, err_msg=f"k={k} stats={st}")
    np.testing.assert_array_equal(again, got)
    return st


def test_option_range():
    with pytest.raises(Exception):
        pkg.set_option("cells_u8_frame", 3)
    assert pkg.get_option("cells_u8_frame") == 2


@pytest.mark.parametrize("k", [3, 8, 15, 16])
@pytest.mark.parametrize("dist", ["uniform", "offset", "lattice", "queries_outside", "copies"])
def test_bin_frames_are_bit_exact(oracle, k, dist):
    rng = np.random.default_rng(k * 91 + len(dist))
    Q, R = _cases(rng, dist, k, 700, (1 << 17) + 1234)
    st = _run(oracle, k, Q, R)
    assert st[0] == 4, st


@pytest.mark.parametrize("dist", ["tight_clusters", "mixture", "one_point"])
def test_bin_frames_forced_on_clustered_data(oracle, dist):
    """Forced where auto would not take them: looser thresholds, more candidates — still every answer exact."""
    rng = np.random.default_rng(3 + len(dist))
    Q, R = _off_the_cube(rng, dist, 16, 1024, 1 << 19)
    _run(oracle, 16, Q, R)


def test_bin_frames_when_every_query_ties_with_many_rows(oracle):
    rng = np.random.default_rng(12)
    k, n, m = 8, (1 << 18) + 5, 1024
    R = (rng.integers(0, 3, (n, k)) * 0.5).astype(np.float32)
    Q = (rng.integers(0, 5, (m, k)) * 0.25).astype(np.float32)
    _run(oracle, k, Q, R)


def test_c3_full_shape_auto_picks_bin_frames_every_query_against_the_oracle(oracle):
    """BASELINE config C3 (k 16, m 1024, n 2^24), every answer, all options on auto: 8-bit rows in bin frames."""
    pkg.set_option("cells_rows", 0)
    pkg.set_option("cells_u8_frame", 0)
    k, m, n = 16, 1024, 1 << 24
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    r_d = torch.empty(n * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(r_d.data_ptr(), n * k, 1001, device=0, stream=stream)
    torch.cuda.synchronize()
    Q = oracle.synth(m * k, 1000).reshape(m, k)
    before = pkg.get_option("cells_u8_builds"), pkg.get_option("cells_u8_bin_builds")
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True, stream=stream)
    try:
        assert (pkg.get_option("cells_u8_builds"), pkg.get_option("cells_u8_bin_builds")) == (before[0] + 1, before[1] + 1)
        got, st = _query(ix, Q)
    finally:
        ix.close()
    assert st[0] == 4 and st[2] == 0, st
    want = oracle.v0(k, Q, oracle.synth(n * k, 1001), threads=THREADS)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("dist", ["tight_clusters", "mixture"])
def test_auto_keeps_per_cell_frames_on_clustered_data(oracle, dist):
    pkg.set_option("cells_u8_frame", 0)
    rng = np.random.default_rng(21 + len(dist))
    k = 16
    Q, R = _off_the_cube(rng, dist, k, 512, 1 << 19)
    want = oracle.v0(k, Q, R, threads=THREADS)
    pkg.set_option("path", 2)
    pkg.set_option("cells", 1)
    before = pkg.get_option("cells_u8_builds"), pkg.get_option("cells_u8_bin_builds")
    ix = pkg.KnnIndex(k, R)
    try:
        assert (pkg.get_option("cells_u8_builds"), pkg.get_option("cells_u8_bin_builds")) == (before[0] + 1, before[1])
        got, _ = _query(ix, Q)
    finally:
        ix.close()
    np.testing.assert_array_equal(got, want)


def test_auto_picks_bin_frames_on_uniform_rows(oracle):
    pkg.set_option("cells_u8_frame", 0)
    rng = np.random.default_rng(5)
    Q, R = _cases(rng, "uniform", 16, 512, (1 << 17) + 1234)
    before = pkg.get_option("cells_u8_bin_builds")
    pkg.set_option("path", 2)
    pkg.set_option("cells", 1)
    ix = pkg.KnnIndex(16, R)
    try:
        assert pkg.get_option("cells_u8_bin_builds") == before + 1
        got, _ = _query(ix, Q)
    finally:
        ix.close()
    np.testing.assert_array_equal(got, oracle.v0(16, Q, R, threads=THREADS))
