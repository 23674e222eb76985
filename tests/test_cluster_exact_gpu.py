"""knn_index_self_cluster_within on the exact self-scan (no flag) on the GPU against tests/cluster_oracle.py: k = 3, 5 (a partial
16-chunk) and 40 (KC 3), n = 1507 (no multiple of 64), base_index != 0.  Bar: labels and core mask equal the oracle's exactly — the
definition leaves no freedom — on lattice rows with planted structures (tests/cluster_helper.py), at the parameter corners, on two
slots, twice over, and across the 65536-row chunk boundary of the sweeps."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co
from tests.cluster_helper import assert_planted, planted, run_cluster
from tests.count_helper import dev
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
BASE = 5
N = 1507
MIN_PTS = 5
INF = float("inf")
LATTICE = {3: (13, 0.0), 5: (12, 0.1), 40: (10, 0.01)}    # side of the lattice in the first three axes; P(1) in every further axis
CHUNK = 65536


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


@functools.lru_cache(maxsize=None)
def shard(k):
    """(R [N][k], names, off, nan_row, inf_row): lattice rows (integer coordinates: every distance exact) left of the origin, the
    planted block in the middle of the row order, then one row with a NaN and one with an Inf coordinate."""
    rng = np.random.default_rng(4200 + k)
    P, names, _ = planted(k, 1.0, 0.0, 0.0, rng)
    nb = N - len(P) - 2
    side, p1 = LATTICE[k]
    B = np.zeros((nb, k), dtype=np.float32)
    B[:, :3] = rng.integers(0, side, size=(nb, 3))
    if k > 3:
        B[:, 3:] = rng.random((nb, k - 3)) < p1
    B[:, 0] -= side + 10
    bad = np.zeros((2, k), dtype=np.float32)
    bad[0, k // 2], bad[1, 0] = np.nan, np.inf
    off = 600
    R = np.concatenate([B[:off], P, bad, B[off:]])
    assert R.shape == (N, k) and N % 64
    return R, names, off, off + len(P), off + len(P) + 1


@functools.lru_cache(maxsize=None)
def want(k, max_dist2, min_pts):
    return co.cluster(shard(k)[0], k, max_dist2, min_pts)


def index_of(k):
    return pkg.KnnIndex(k, shard(k)[0], base_index=BASE)


@pytest.mark.parametrize("k", [3, 5, 40])
def test_labels_and_core_mask_equal_the_oracle_and_the_planted_structures_come_out(k):
    R, names, off, nan_row, inf_row = shard(k)
    w = want(k, 1.0, MIN_PTS)
    core, border = w["core"], w["border"]
    shares = (core.mean(), border.mean(), 1.0 - core.mean() - border.mean())
    print(f"k={k}: core {shares[0]:.3f} border {shares[1]:.3f} noise {shares[2]:.3f} of {N} rows, {np.unique(w['labels']).size - 1} clusters")
    assert min(shares) >= 0.05, shares                                     # a condition on the inputs, by the oracle
    assert_planted(w["labels"], core, names, off, MIN_PTS)                 # ... and the structures are what the helper says
    ix = index_of(k)
    try:
        labels, words, st = run_cluster(ix, 1.0, MIN_PTS)
        assert st == [1, 0, 0, 0], st
        np.testing.assert_array_equal(labels, w["labels"])
        np.testing.assert_array_equal(words, co.core_mask_words(core))
        assert_planted(labels, core, names, off, MIN_PTS)
        assert labels[nan_row] == -1 and labels[inf_row] == -1
        # again, and without a core mask: bit for bit the same
        labels2, words2, _ = run_cluster(ix, 1.0, MIN_PTS)
        labels3, none, _ = run_cluster(ix, 1.0, MIN_PTS, want_core=False)
        assert none is None
        np.testing.assert_array_equal(labels2, labels)
        np.testing.assert_array_equal(words2, words)
        np.testing.assert_array_equal(labels3, labels)
        # the host form: the same clusters, numbered 0 .. C - 1 by their representative row
        hl, hc, info = ix.self_cluster_within_host(1.0, MIN_PTS)
        np.testing.assert_array_equal(hl, co.renumber(w["labels"]))
        np.testing.assert_array_equal(hc, core)
        assert info == dict(clusters=np.unique(w["labels"]).size - 1, core=int(core.sum()), border=int(border.sum()),
                            noise=int((w["labels"] < 0).sum()))
    finally:
        ix.close()


@pytest.mark.parametrize("k", [3, 5, 40])
def test_the_parameter_corners(k):
    R, names, off, nan_row, inf_row = shard(k)
    finite = np.isfinite(R).all(axis=1)
    ix = index_of(k)
    try:
        # min_pts = 1: every row core, the labels are the components of the radius graph; the NaN row is a cluster of its own
        labels, words, _ = run_cluster(ix, 1.0, 1)
        w = want(k, 1.0, 1)
        np.testing.assert_array_equal(labels, w["labels"])
        np.testing.assert_array_equal(words, co.core_mask_words(np.ones(N, dtype=bool)))
        assert labels[nan_row] == nan_row and labels[inf_row] == inf_row and (labels >= 0).all()
        assert (labels <= np.arange(N)).all() and (labels[labels] == labels).all()
        # min_pts > n: nothing is core, everything noise
        labels, words, _ = run_cluster(ix, 1.0, N + 1)
        assert (labels == -1).all() and (words == 0).all()
        # max_dist2 = 0 (and -0): only exact duplicates link
        for zero in (0.0, -0.0):
            labels, words, _ = run_cluster(ix, zero, 2)
            w = want(k, 0.0, 2)
            np.testing.assert_array_equal(labels, w["labels"])
            np.testing.assert_array_equal(words, co.core_mask_words(w["core"]))
        copies = names["copies"] + off
        assert (labels[copies] == copies.min()).all() and (labels[names["chain down"] + off] == -1).all()
        # max_dist2 = +INF: one cluster of all the finite rows
        labels, words, _ = run_cluster(ix, INF, MIN_PTS)
        np.testing.assert_array_equal(labels, np.where(finite, np.flatnonzero(finite).min(), -1))
        np.testing.assert_array_equal(words, co.core_mask_words(finite))
        np.testing.assert_array_equal(labels, want(k, INF, MIN_PTS)["labels"])
    finally:
        ix.close()


@pytest.mark.parametrize("k", [3, 40])
def test_the_core_mask_is_a_mask_for_the_masked_calls_and_two_slots_do_not_meet(k):
    R, names, off, _, _ = shard(k)
    w5, w4 = want(k, 1.0, 5), want(k, 1.0, 4)
    ix = index_of(k)
    try:
        # two calls in flight on two slots, different parameters, one synchronisation
        la = torch.full((N,), -7, dtype=torch.int32, device=dev())
        lb = torch.full((N,), -7, dtype=torch.int32, device=dev())
        ca = torch.full(((N + 31) // 32,), -1, dtype=torch.int32, device=dev())
        ix.self_cluster_within(1.0, 5, la.data_ptr(), core_dev=ca.data_ptr(), slot=0)
        ix.self_cluster_within(1.0, 4, lb.data_ptr(), slot=3)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(la.cpu().numpy(), w5["labels"])
        np.testing.assert_array_equal(lb.cpu().numpy(), w4["labels"])
        # "count the core rows within the radius": the mask goes straight into knn_index_count_within_masked
        rows = np.concatenate([np.arange(0, N, 7), names["bridge row"] + off])
        Q = np.ascontiguousarray(R[rows])
        q_d = torch.from_numpy(Q.reshape(-1)).to(dev())
        counts = torch.full((len(rows),), 12345, dtype=torch.int32, device=dev())
        ix.count_within_masked(len(rows), q_d.data_ptr(), 1.0, ca.data_ptr(), counts.data_ptr(), init=True)
        torch.cuda.synchronize()
        d = v0_dist2(Q, R, k)
        expect = ((d < np.float32(np.inf)) & (d <= np.float32(1.0)) & w5["core"][None, :]).sum(axis=1)
        np.testing.assert_array_equal(counts.cpu().numpy(), expect)
        assert expect[-1] == 2                                            # the bridge: one core row of either run
    finally:
        ix.close()


def test_clusters_that_span_the_65536_row_chunk_boundary_come_out_whole():
    """k = 1, n = 65536 + 70, one call: both sweeps run in two chunks of rows.  Rows lie along the axis roughly in row order — gaps of
    a quarter, a half or three units of the radius — so clusters are runs of rows, and the gaps around row 65536 are small: a
    cluster spans the boundary.  A block of rows from the far end is moved to the front of the row order, so some clusters have
    rows in both chunks that are far apart in row number as well."""
    n = CHUNK + 70
    rng = np.random.default_rng(4300)
    gaps = rng.choice(np.array([0.25, 0.5, 3.0]), size=n, p=[0.5, 0.4, 0.1])
    gaps[CHUNK - 80:CHUNK] = 0.25                                           # places 65456 .. 65535 are rows 65486 .. 65565
    gaps[n - 60:] = 0.25
    gaps[n - 60] = 3.0                                                      # ... and the run of the last 60 places is one of its own
    x = np.cumsum(gaps)
    order = np.concatenate([np.arange(n - 30, n), np.arange(n - 30)])       # the last 30 places become rows 0 .. 29
    R = x[order].astype(np.float32).reshape(n, 1)
    assert (R[:, 0].astype(np.float64) == x[order]).all()
    w = co.cluster(R, 1, 1.0, MIN_PTS)
    lab = w["labels"]
    spans = [c for c in np.unique(lab[lab >= 0]) if (np.flatnonzero(lab == c) < CHUNK).any() and (np.flatnonzero(lab == c) >= CHUNK).any()]
    assert len(spans) >= 2 and 0 in lab[CHUNK:], spans                     # across the boundary, and from row 0 to the last rows
    shares = (w["core"].mean(), w["border"].mean(), (lab < 0).mean())
    print(f"chunk crossing: core {shares[0]:.3f} border {shares[1]:.3f} noise {shares[2]:.3f}, {np.unique(lab).size - 1} clusters, "
          f"{len(spans)} across the boundary")
    assert min(shares) >= 0.02, shares
    assert pkg.debug_cluster_plan(k=1, n=n, num_cu=256, core_given=1, grid=0)["chunks"] == 2
    ix = pkg.KnnIndex(1, R, base_index=BASE)
    try:
        labels, words, st = run_cluster(ix, 1.0, MIN_PTS)
        assert st == [1, 0, 0, 0], st
        np.testing.assert_array_equal(labels, lab)
        np.testing.assert_array_equal(words, co.core_mask_words(w["core"]))
    finally:
        ix.close()
