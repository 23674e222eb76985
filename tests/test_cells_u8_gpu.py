"""8-bit rows of the cell-pruned scan (option `cells_rows` = 2: one byte per coordinate in each cell's own frame, 20 bytes
per row instead of 36) against the CPU oracle.  The quantiser widens every row's error bound; what must not change is a
single answer.  Bar: bit-exact, ties to the lowest index, whatever the data."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.test_cells_gpu import THREADS, _cases, _off_the_cube, _query

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _u8_rows():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    pkg.set_option("cells_rows", 2)
    yield
    for name in ("path", "cells", "cells_rows", "cells_centre"):
        pkg.set_option(name, 0)


def _run(oracle, k, Q, R):
    want = oracle.v0(k, Q, R, threads=THREADS)
    pkg.set_option("path", 2)
    pkg.set_option("cells", 1)
    before = pkg.get_option("cells_u8_builds")
    ix = pkg.KnnIndex(k, R, base_index=7)
    try:
        assert pkg.get_option("cells_u8_builds") == before + 1     # the layout really has 8-bit rows
        got, st = _query(ix, Q)
        again, _ = _query(ix, Q)
    finally:
        ix.close()
    np.testing.assert_array_equal(got - 7, want, err_msg=f"k={k} stats={st}")
    np.testing.assert_array_equal(again, got)
    return st


@pytest.mark.parametrize("k", [3, 8, 15, 16])
@pytest.mark.parametrize("dist", ["uniform", "offset", "lattice", "clustered", "skewed", "queries_outside", "copies"])
def test_u8_rows_are_bit_exact(oracle, k, dist):
    """lattice: rows and queries on the cuts, exact ties; copies: duplicate rows, distance 0; partly filled K-slots at k 3, 8, 15."""
    rng = np.random.default_rng(k * 77 + len(dist))
    Q, R = _cases(rng, dist, k, 700, (1 << 17) + 1234)
    st = _run(oracle, k, Q, R)
    assert st[0] == 4, st


@pytest.mark.parametrize("dist", ["tight_clusters", "low_rank", "mixture", "one_point"])
def test_u8_rows_on_clustered_and_degenerate_data(oracle, dist):
    """one_point: one cell holds the shard and every distance ties — the batch ends in the over-full fallback (exact
    evaluation of the listed pairs); slower is allowed, a wrong index is not."""
    rng = np.random.default_rng(len(dist))
    Q, R = _off_the_cube(rng, dist, 16, 1024, 1 << 19)
    _run(oracle, 16, Q, R)


def test_u8_rows_on_heavy_tailed_rows(oracle):
    rng = np.random.default_rng(5)
    k, n, m = 16, 1 << 19, 1024
    R = rng.standard_cauchy((n, k)).astype(np.float32)
    Q = rng.normal(0, 1, (m, k)).astype(np.float32)
    _run(oracle, k, Q, R)


def test_u8_rows_when_every_query_ties_with_many_rows(oracle):
    """Rows on a coarse lattice repeated many times over: each query's answer ties with dozens of copies in the same and in
    neighbouring cells, the lowest index must win."""
    rng = np.random.default_rng(11)
    k, n, m = 8, (1 << 18) + 5, 1024
    R = (rng.integers(0, 3, (n, k)) * 0.5).astype(np.float32)
    Q = (rng.integers(0, 5, (m, k)) * 0.25).astype(np.float32)
    _run(oracle, k, Q, R)


def test_c3_full_shape_with_u8_rows_every_query_against_the_oracle(oracle):
    """BASELINE config C3 (k 16, m 1024, n 2^24), every answer, 8-bit rows on request (what the library policy picks there too)."""
    k, m, n = 16, 1024, 1 << 24
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    r_d = torch.empty(n * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(r_d.data_ptr(), n * k, 1001, device=0, stream=stream)
    torch.cuda.synchronize()
    Q = oracle.synth(m * k, 1000).reshape(m, k)
    before = pkg.get_option("cells_u8_builds")
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True, stream=stream)
    try:
        assert pkg.get_option("cells_u8_builds") == before + 1
        got, st = _query(ix, Q)
    finally:
        ix.close()
    assert st[0] == 4 and st[2] == 0, st
    want = oracle.v0(k, Q, oracle.synth(n * k, 1001), threads=THREADS)
    np.testing.assert_array_equal(got, want)


def test_library_policy_picks_u8_rows_for_large_uniform_shards_only(oracle):
    """Auto: 8-bit rows for uniform-like shards of >= 2^24 rows only (gaussian rows and smaller shards measured slower)."""
    k, n = 16, 1 << 24
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pkg.set_option("cells_rows", 0)
    r_d = torch.empty(n * k, dtype=torch.float32, device=dev)
    for fill, rows, want_u8 in (("uniform", n, True), ("gaussian", n, False), ("uniform", 1 << 22, False)):
        if fill == "uniform":
            pkg.synth_fill_device(r_d.data_ptr(), rows * k, 1001, device=0, stream=stream)
        else:
            r_d[: rows * k].normal_()
        torch.cuda.synchronize()
        before = pkg.get_option("cells_u8_builds")
        ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=rows, refs_on_device=True, stream=stream)
        ix.close()
        assert (pkg.get_option("cells_u8_builds") == before + 1) == want_u8, (fill, rows)
    pkg.set_option("cells_rows", 1)
    pkg.synth_fill_device(r_d.data_ptr(), n * k, 1001, device=0, stream=stream)
    torch.cuda.synchronize()
    before = pkg.get_option("cells_u8_builds")
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True, stream=stream)
    ix.close()
    assert pkg.get_option("cells_u8_builds") == before
