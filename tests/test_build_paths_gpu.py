"""The ways a filter layout gets built that the other suites pass through only in the middle of a shape: the seam between the
two chunks of an ingest from host rows (both ingests, a shard just over the 128 MiB from which it goes over in two pieces), and a resident build
whose sampled frame is declined so that the full-range frame takes over.  Bar: bit-exact against the CPU oracle, and the way
the batch was answered (last_stats()[0]) is the one the build under test leads to."""
import os

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
OPTIONS = ("path", "cells", "ingest")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert os.path.exists(pkg.lib_path), "libknn_mi355x.so not built (no CPU fallback exists)"
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


SEAM_K, SEAM_M, SEAM_N = 16, 64, (1 << 21) + 4097   # 128 MiB + 4097 rows: just over the size from which a shard goes over in two pieces
SEAM_HEAD = 1052672                                 # rows of its first chunk, at either ingest's granule


@pytest.fixture(scope="module")
def seam_case(oracle):
    """Uniform rows; the first four queries ARE the rows on both sides of the chunk seam, the shard's last row and its first."""
    k, m, n = SEAM_K, SEAM_M, SEAM_N
    for granule in (1024, 4096):
        assert pkg.debug_ingest_head_rows(k, n, granule) == SEAM_HEAD
        assert pkg.debug_ingest_head_rows(k, 1 << 21, granule) == 1 << 21      # (128 MiB exactly: one piece)
    R = oracle.synth(n * k, 81).reshape(n, k)
    Q = oracle.synth(m * k, 82).reshape(m, k).copy()
    rows = np.array([SEAM_HEAD - 1, SEAM_HEAD, n - 1, 0])
    for i in rows:
        assert int((R == R[i]).all(axis=1).sum()) == 1, f"row {i} has a duplicate"
    Q[:4] = R[rows]
    want = oracle.v0(k, Q, R, threads=THREADS)
    np.testing.assert_array_equal(want[:4], rows)
    R.setflags(write=False)
    Q.setflags(write=False)
    return Q, R, rows, want


@pytest.mark.parametrize("cells,path,ingest,way", [(1, 0, 2, pkg.WAY_CELLS), (2, 2, 1, pkg.WAY_FILTER)],
                         ids=["cell_ingest", "plain_ingest"])
def test_rows_on_both_sides_of_an_ingest_chunk_seam_are_found(seam_case, cells, path, ingest, way):
    """An index created from host rows ships a shard above 128 MiB in two copies and builds its layouts per landed chunk: the
    cell ingest scatters each chunk into the buckets, the plain ingest (path 2 at creation, as the ingest tests of
    test_parity_gpu.py set it) turns each into fragments + norms.  The last row of the first chunk, the first row of the second,
    the shard's last and first row must each be their own nearest neighbour, and the whole batch bit-exact."""
    Q, R, rows, want = seam_case
    plan = pkg.debug_index_build_plan(k=SEAM_K, n_local=SEAM_N, refs_on_device=0, build_filter=-1, build_grid=-1, path=path,
                                      cells=cells, ingest=0, cells_build=0)
    assert plan["ingest"] == ingest, plan
    try:
        pkg.set_option("cells", cells)
        pkg.set_option("path", path)
        ix = pkg.KnnIndex(SEAM_K, R)                    # host rows
        pkg.set_option("path", 0)
        try:
            got = ix.query(Q)
            st = ix.last_stats()
        finally:
            ix.close()
    finally:
        for name in OPTIONS:
            pkg.set_option(name, 0)
    np.testing.assert_array_equal(got[:4], rows, err_msg=f"stats={st}")
    np.testing.assert_array_equal(got, want, err_msg=f"stats={st}")
    assert st[0] == way, st


# (the full-range frame's own cell-sorted build — the counted one — takes the shard; profiles/r15_layout_build.txt says how the
# value was arrived at)
WAY_AFTER_DECLINED_SAMPLE = pkg.WAY_CELLS


def test_full_range_frame_takes_over_when_the_sampled_frame_is_declined(oracle):
    """Resident rows with a NaN in row 0, which is on the build's 4096-row sample stride: the sampled frame is not finite, the
    cell-sorted build from it is given up and the build starts over from the full-range statistics, where the NaN row is an
    outlier like any other (on the exact list: last_stats()[3] >= 1).  One query sits next to row 1."""
    k, m, n = 16, 64, (1 << 17) + 77
    R = oracle.synth(n * k, 83).reshape(n, k).copy()
    Q = oracle.synth(m * k, 84).reshape(m, k).copy()
    R[0, 5] = np.nan
    Q[0] = R[1] + np.float32(1e-3)
    want = oracle.v0(k, Q, R, threads=THREADS)
    assert want[0] == 1
    dev = torch.device("cuda:0")
    r_d = torch.from_numpy(R).to(dev)
    try:
        pkg.set_option("cells", 1)
        ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True, owners=r_d)
        try:
            got = ix.query(Q)
            st = ix.last_stats()
        finally:
            ix.close()
    finally:
        for name in OPTIONS:
            pkg.set_option(name, 0)
    print("stats after a declined sampled frame:", st)
    np.testing.assert_array_equal(got, want, err_msg=f"stats={st}")
    assert st[3] >= 1, st
    assert st[0] == WAY_AFTER_DECLINED_SAMPLE, st
