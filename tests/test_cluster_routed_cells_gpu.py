"""knn_index_self_cluster_within_routed on the cell-pruned scan (KNN_QUERY_COUNT_CELLS; include/knn_mi355x.h 2n) on the GPU.  The bar
everywhere: labels and core mask equal, bit for bit, knn_index_self_cluster_within on the exact way of the same index (pinned to
tests/cluster_oracle.py by the existing tests); knn_index_last_stats()[0] == 4, [2] == 0 unless the test says otherwise; outputs
poisoned before each call.  The shards: tests/cluster_routed_rows.py (tests/test_cluster_routed_logic.py says what they are)."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co
from tests import cluster_routed_rows as rr
from tests import cluster_rows
from tests.cluster_helper import assert_planted, run_cluster
from tests.cluster_routed_helper import core_flags, run_cluster_routed
from tests.count_helper import dev, dev_counts, host_counts
from tests.shards_helper import Shards
from tests.test_within_cells_gpu import BINS, CENTRED, FP16, MATRIX, N17, OPTIONS

pytestmark = pytest.mark.gpu
INF = float("inf")
NIF = [c for c in MATRIX if c[0] == "nif_k20_fixed"][0]
CASES = [
    ("fp16_k16_fixed", 16, dict(FP16, scan_deal=1)),
    ("fp16_k16_counter", 16, dict(FP16, scan_deal=2)),
    ("bins_k16_fixed", 16, dict(BINS, scan_deal=1)),
    ("bins_k16_counter", 16, dict(BINS, scan_deal=2)),
    ("fp16_k8", 8, FP16),
    NIF,
]


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


def assert_same(got, ref, msg=""):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=f"{msg} labels")
    if got[1] is not None and ref[1] is not None:
        np.testing.assert_array_equal(got[1], ref[1], err_msg=f"{msg} core words")


def assert_pruned(st, msg=""):
    assert st[0] == 4 and st[2] == 0, (msg, st)


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_every_layout_form_gives_the_exact_ways_labels_and_the_planted_structures(name, k, opts):
    R, names, off, r, min_pts = rr.planted17(k)
    assert N17 == rr.N17 and off < 64 * 1024 < off + rr.planted_rows(names)          # the block straddles a pass boundary
    _set(opts)
    ix = pkg.KnnIndex(k, R)
    try:
        ref = run_cluster(ix, r * r, min_pts)
        assert ref[2][0] == 1, ref[2]
        got = run_cluster_routed(ix, r * r, min_pts, cells=True)
        assert_pruned(got[2], name)
        assert got[2][3] > 0, got[2]                                                    # the planted rows are out-of-box rows
        assert_same(got, ref, name)
        assert_planted(got[0], core_flags(got[1], N17), names, off, min_pts)
        # a radius that is no power of two: the shard's median 8th-neighbour distance, where most rows have neighbours
        cap = float(np.median(rr.kth_neighbour_dist2(R, k, np.arange(256), 8)))
        ref = run_cluster(ix, cap, min_pts)
        got = run_cluster_routed(ix, cap, min_pts, cells=True)
        assert_pruned(got[2], name)
        assert_same(got, ref, f"{name} median radius")
        assert (got[0] >= 0).mean() > 0.2 and (got[0] < 0).any(), name
    finally:
        ix.close()


def test_the_long_box_equals_the_oracle_on_the_device_and_the_host_forms():
    R, cap = rr.long_box()
    w = rr.want_long_box()
    _set(FP16)
    ix = pkg.KnnIndex(rr.LONG_K, R)
    try:
        labels, core, st = run_cluster_routed(ix, cap, rr.LONG_MIN_PTS, cells=True)
        assert_pruned(st)
        np.testing.assert_array_equal(labels, w["labels"])
        np.testing.assert_array_equal(core, co.core_mask_words(w["core"]))
        hl, hc, info = ix.self_cluster_within_routed_host(cap, rr.LONG_MIN_PTS, cells=True)
        assert ix.last_stats()[0] == 4
        np.testing.assert_array_equal(hl, co.renumber(w["labels"]))
        np.testing.assert_array_equal(hc, w["core"])
        border = int((~w["core"] & (w["labels"] >= 0)).sum())
        assert info == dict(clusters=int(np.unique(w["labels"][w["labels"] >= 0]).size), core=int(w["core"].sum()), border=border,
                            noise=int((w["labels"] < 0).sum()))
    finally:
        ix.close()


def test_without_core_dev_the_labels_are_the_same_and_the_mask_serves_the_masked_calls():
    k = 8
    R, names, off, r, min_pts = rr.planted17(k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        n = ix.n
        labels = torch.full((n,), -7, dtype=torch.int32, device=dev())
        core = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev())
        ix.self_cluster_within_routed(r * r, min_pts, labels.data_ptr(), core_dev=core.data_ptr(), cells=True)
        torch.cuda.synchronize()
        assert_pruned(ix.last_stats())
        bare = run_cluster_routed(ix, r * r, min_pts, want_core=False, cells=True)
        assert_pruned(bare[2])
        np.testing.assert_array_equal(bare[0], labels.cpu().numpy())
        words = core.cpu().numpy().view(np.uint32)
        ref = run_cluster(ix, r * r, min_pts)
        np.testing.assert_array_equal(bare[0], ref[0])
        np.testing.assert_array_equal(words, ref[1])
        flags = core_flags(words, n)
        # "query the core rows only": every row against the mask at a radius beyond the cube's diagonal and the planted block
        m = 8
        q = torch.from_numpy(R[:m].copy()).to(dev())
        counts = dev_counts(m, fill=0xDEADBEEF)
        ix.count_within_masked(m, q.data_ptr(), 1e4, core.data_ptr(), counts.data_ptr(), init=True)
        torch.cuda.synchronize()
        assert (host_counts(counts) == flags.sum()).all() and flags.sum() > 0
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [FP16, BINS], ids=["fp16", "bins"])
def test_a_far_row_and_a_nan_row_fall_back_pass_by_pass_and_the_next_shard_is_pruned_again(opts):
    k, r, min_pts = 8, rr.RADIUS[8], 4
    R, far, bad = rr.fallback_rows(k)
    _set(opts)
    ix = pkg.KnnIndex(k, R)
    try:
        ref = run_cluster(ix, r * r, min_pts)
        got = run_cluster_routed(ix, r * r, min_pts, cells=True)
        assert got[2][0] == 4 and got[2][2] != 0, got[2]                    # the last pass owns the far row: it fell back
        assert_same(got, ref, "fell back")
        assert got[0][far] == -1 and got[0][bad] == -1                       # both noise
        assert (got[0] >= 0).mean() > 0.2
        ones = run_cluster_routed(ix, r * r, 1, cells=True)
        assert ones[2][0] == 4 and ones[2][2] != 0, ones[2]
        assert_same(ones, run_cluster(ix, r * r, 1), "fell back, min_pts 1")
        assert ones[0][far] == far and ones[0][bad] == bad                   # clusters of their own
    finally:
        ix.close()
    clean = R.copy()
    clean[far] = clean[far - 1] * np.float32(0.5)
    clean[bad] = clean[bad - 1] * np.float32(0.5)
    ix = pkg.KnnIndex(k, clean)
    try:
        got = run_cluster_routed(ix, r * r, min_pts, cells=True)
        assert_pruned(got[2], "the shard without the two rows")
        assert_same(got, run_cluster(ix, r * r, min_pts), "the shard without the two rows")
    finally:
        ix.close()


def test_min_pts_one_gives_the_connected_components():
    k = 8
    R, names, off, r, _ = rr.planted17(k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        got = run_cluster_routed(ix, r * r, 1, cells=True)
        assert_pruned(got[2])
        assert core_flags(got[1], N17).all() and (got[0] >= 0).all() and (got[0] <= np.arange(N17)).all()
        assert_same(got, run_cluster(ix, r * r, 1), "min_pts 1")
        assert np.unique(got[0]).size < N17
    finally:
        ix.close()


def test_the_route():
    k = 8
    R, names, off, r, min_pts = rr.planted17(k)
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        ref = run_cluster(ix, r * r, min_pts)
        got = run_cluster_routed(ix, r * r, min_pts)                          # no flag
        assert got[2] == [1, 0, 0, 0], got[2]
        assert_same(got, ref, "no flag")
        pkg.set_option("cells", 2)
        got = run_cluster_routed(ix, r * r, min_pts, cells=True)
        assert got[2][0] == 1, got[2]
        assert_same(got, ref, "cells 2")
        pkg.set_option("cells", 1)
    finally:
        ix.close()
    small = np.ascontiguousarray(R[:5000])
    ix = pkg.KnnIndex(k, small)
    try:
        got = run_cluster_routed(ix, INF, min_pts, cells=True)                # no radius: nothing to prune with
        assert got[2][0] == 1, got[2]
        assert_same(got, run_cluster(ix, INF, min_pts), "+INF")
        assert (got[0] == 0).all()
    finally:
        ix.close()
    _set(CENTRED)                                                             # per-cell frames: not a one-frame layout
    ix = pkg.KnnIndex(k, R)
    try:
        got = run_cluster_routed(ix, r * r, min_pts, cells=True)
        assert got[2][0] == 1, got[2]
        assert_same(got, ref, "per-cell frames")
    finally:
        ix.close()
    for name in OPTIONS:
        pkg.set_option(name, 0)
    G, gnames, goff = cluster_rows.uniform_planted(2)                         # a grid shard
    gr, gmp = cluster_rows.PLANTED_SHAPE[2]
    ix = pkg.KnnIndex(2, G)
    try:
        ref = run_cluster(ix, gr * gr, gmp, grid=True)
        assert ref[2][0] == 3, ref[2]
        for flags in (dict(grid=True), dict(grid=True, cells=True)):          # the grid comes first for a call that carries both
            got = run_cluster_routed(ix, gr * gr, gmp, **flags)
            assert got[2][0] == 3, (flags, got[2])
            assert_same(got, ref, str(flags))
        assert_planted(got[0], core_flags(got[1], ix.n), gnames, goff, gmp)
    finally:
        ix.close()


def test_two_slots_on_two_streams_with_two_radii_equal_their_sequential_answers():
    k = 8
    R, names, off, r, min_pts = rr.planted17(k)
    radii = (r * r, float(np.float32(0.75 * r * r)))
    _set(FP16)
    ix = pkg.KnnIndex(k, R)
    try:
        alone = [run_cluster_routed(ix, cap, min_pts, slot=s, cells=True) for s, cap in enumerate(radii)]
        for a in alone:
            assert_pruned(a[2])
        assert not np.array_equal(alone[0][0], alone[1][0])
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        out = [run_cluster_routed(ix, cap, min_pts, slot=s, stream=streams[s].cuda_stream, sync=False, cells=True)
               for s, cap in enumerate(radii)]
        torch.cuda.synchronize()
        for s in range(2):
            np.testing.assert_array_equal(out[s][0].cpu().numpy(), alone[s][0], err_msg=f"slot {s} labels")
            np.testing.assert_array_equal(out[s][1].cpu().numpy().view(np.uint32), alone[s][1], err_msg=f"slot {s} core words")
    finally:
        ix.close()


def test_a_cell_range_shard_pair_labels_its_own_rows_by_local_row():
    k = 16
    n = (1 << 19) + 5
    R = np.random.default_rng(7600).random((n, k), dtype=np.float32)
    cap = float(np.median(rr.kth_neighbour_dist2(R, k, np.arange(64), 4)))
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=False)
    try:
        for rank, ix in enumerate(sh.idx):
            ref = run_cluster(ix, cap, 3)
            got = run_cluster_routed(ix, cap, 3, cells=True)
            assert_pruned(got[2], f"rank {rank}")
            assert_same(got, ref, f"rank {rank}")
            assert got[0].max() < ix.n and (got[0] >= 0).any() and (got[0] < 0).any()
            flags = core_flags(got[1], ix.n)
            assert flags.any() and (got[0][flags] <= np.flatnonzero(flags)).all()    # a core row's label: a LOCAL row at or below its own
    finally:
        sh.close()
