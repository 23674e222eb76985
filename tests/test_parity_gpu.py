"""Parity tests proper: the HIP path (through the C-ABI of libknn_mi355x.so) against the CPU
oracle and the committed golden vectors.  Bar: bit-exact nearest indices."""
import os

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.oracle_lib import TA_SAMPLES
from tests.test_oracle import read_golden_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert os.path.exists(pkg.lib_path), "libknn_mi355x.so not built (no CPU fallback exists)"
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)
    pkg.set_option("shards", 0)


@pytest.fixture(params=[1, 2, 0], ids=["exact", "filter", "auto"])
def path(request):
    pkg.set_option("path", request.param)
    yield request.param
    pkg.set_option("path", 0)


def test_ta_samples_match_reference_golden_file(oracle, path):
    """The reference's own test (main.cu:28-39, seed 1000) against its results.csv."""
    gold = read_golden_indices()
    for i, (k, m, n, Q, R) in enumerate(oracle.ta_samples()):
        got = pkg.cudaCallback(k, m, n, Q, R)
        np.testing.assert_array_equal(got, gold[i], err_msg=f"TA sample {i} {(k, m, n)}")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 16, 17, 33])
@pytest.mark.parametrize("m,n", [(1, 1), (1, 2), (2, 8), (1, 1025), (3, 4097), (47, 1000), (48, 1000),
                                 (64, 333), (130, 2049), (257, 5000), (700, 3001), (1024, 1024), (1500, 777)])
def test_ragged_shapes_bit_exact(oracle, path, k, m, n):
    rng = np.random.default_rng(k * 100003 + m * 1009 + n)
    Q = rng.random((m, k), dtype=np.float32)
    R = rng.random((n, k), dtype=np.float32)
    got = pkg.cudaCallback(k, m, n, Q, R)
    np.testing.assert_array_equal(got, oracle.v0(k, Q, R))


@pytest.mark.parametrize("k,m,n", [(3, 1024, 65536), (16, 1024, 65536), (16, 64, 1 << 18), (3, 5, 1 << 20),
                                   (16, 1, 1 << 20), (16, 1, 5000), (16, 2, 70001), (16, 5, 70001), (16, 8, 70001),
                                   (8, 300, 100000), (16, 1057, 70001), (16, 1100, 70001), (16, 1600, 70001),
                                   (16, 577, 70001), (20, 600, 70001), (20, 1057, 70001), (3, 2100, 70001),
                                   (128, 600, 4100), (40, 513, 9000), (64, 2048, 70000), (33, 1000, 131072),
                                   # 128 < k <= 512: the LDS-tiled filter with 2 / 1 blocks of queries per wave; beyond: exact only
                                   (129, 600, 4100), (200, 70, 9000), (256, 513, 5000), (257, 300, 9000), (384, 1100, 4100),
                                   (512, 200, 5000),
                                   # k > 512: K walked in chunks of 128 dimensions (knn_filter_chunked_kernel); k > 4096: exact only
                                   (513, 100, 3000), (1000, 48, 2000), (640, 300, 4100), (1024, 513, 3000), (1500, 70, 5000),
                                   (4096, 64, 1200), (4100, 48, 600)])
def test_synthetic_uniform_bit_exact(oracle, path, k, m, n):
    Q, R = oracle.synth(m * k, 1000), oracle.synth(n * k, 1001)
    got = pkg.cudaCallback(k, m, n, Q, R)
    np.testing.assert_array_equal(got, oracle.v0(k, Q, R))


def test_ties_pick_lowest_index_across_slices_and_shards(oracle, path):
    k, m, n = 16, 1024, 40000
    rng = np.random.default_rng(5)
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    dup = rng.integers(0, n, size=m)
    Q[:] = R[dup]                     # every query coincides with a reference ...
    R[(dup + 7919) % n] = R[dup]      # ... that also appears a second time, far away
    R[n - 1] = R[0]
    want = oracle.v0(k, Q, R)
    np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), want)
    for shards in (2, 3, 8):
        pkg.set_option("shards", shards)
        np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), want, err_msg=f"shards={shards}")
    pkg.set_option("shards", 0)
    # all references identical: index 0 for every query
    R[:] = R[123]
    np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), np.zeros(m, dtype=np.int32))


def test_nan_inf_and_overflow_semantics(oracle, path):
    k = 4
    rng = np.random.default_rng(11)
    R = rng.random((5000, k), dtype=np.float32)
    Q = rng.random((100, k), dtype=np.float32)
    R[::7, 1] = np.nan
    R[5::11, 2] = np.inf
    R[3::13, 0] = -np.inf
    Q[3, 0] = np.nan          # NaN query: nothing beats +INF -> index 0
    Q[4, 1] = np.inf
    np.testing.assert_array_equal(pkg.cudaCallback(k, 100, 5000, Q, R), oracle.v0(k, Q, R))
    big = np.full((64, k), 3e38, dtype=np.float32)
    qneg = np.full((64, k), -3e38, dtype=np.float32)   # every distance overflows to +INF -> 0
    np.testing.assert_array_equal(pkg.cudaCallback(k, 64, 64, qneg, big), np.zeros(64, dtype=np.int32))
    Rn = np.full((300, k), np.nan, dtype=np.float32)
    np.testing.assert_array_equal(pkg.cudaCallback(k, 100, 300, Q, Rn), np.zeros(100, dtype=np.int32))


def test_wide_dynamic_range_and_offsets(oracle, path):
    """Data far from the origin / tiny / huge scales: the filter's error bound must hold or the
    library must take the exact path; either way indices are bit-exact."""
    k, m, n = 16, 256, 30000
    rng = np.random.default_rng(3)
    for scale, offset in [(1e-3, 1000.0), (1e6, -5e6), (1e-20, 0.0), (1e15, 1e15), (1.0, 0.0)]:
        R = (rng.random((n, k), dtype=np.float32) * np.float32(scale) + np.float32(offset)).astype(np.float32)
        Q = (rng.random((m, k), dtype=np.float32) * np.float32(scale) + np.float32(offset)).astype(np.float32)
        np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), oracle.v0(k, Q, R),
                                      err_msg=f"scale={scale} offset={offset}")
    # clustered data: many near-ties
    centers = rng.random((8, k), dtype=np.float32)
    R = (centers[rng.integers(0, 8, n)] + rng.normal(0, 1e-4, (n, k))).astype(np.float32)
    Q = (centers[rng.integers(0, 8, m)] + rng.normal(0, 1e-4, (m, k))).astype(np.float32)
    np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), oracle.v0(k, Q, R))
    # integer lattice: massive exact ties
    R = rng.integers(0, 4, (n, k)).astype(np.float32)
    Q = rng.integers(0, 4, (m, k)).astype(np.float32)
    np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), oracle.v0(k, Q, R))


def test_sharded_callback_equals_single_shard(oracle, path):
    """cudaCallback's partition + key merge (what the reference got wrong, core.cu:941-943)."""
    k, m, n = 3, 200, 10007
    Q, R = oracle.synth(m * k, 21), oracle.synth(n * k, 22)
    want = oracle.v0(k, Q, R)
    for shards in (1, 2, 4, 7, 8, 64):
        pkg.set_option("shards", shards)
        np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), want, err_msg=f"shards={shards}")
    pkg.set_option("shards", 0)
    # more shards than points (core.cu:867-868)
    pkg.set_option("shards", 8)
    np.testing.assert_array_equal(pkg.cudaCallback(k, m, 3, Q, R[:9]), oracle.v0(k, Q, R[:9]))
    # an empty shard in the host merge: 3 shards of ceil(4 / 3) = 2 rows are [0,2) [2,4) [4,4)
    pkg.set_option("shards", 3)
    np.testing.assert_array_equal(pkg.cudaCallback(k, 5, 4, Q[:15], R[:12]), oracle.v0(k, Q[:15], R[:12]))
    pkg.set_option("shards", 0)


def test_index_api_keys_fold_across_shards_on_device(oracle, path):
    """knn_index_*: device-resident shards folding into one key array (the bench.py data path)."""
    k, m, n = 16, 512, 50000
    Q, R = oracle.synth(m * k, 31), oracle.synth(n * k, 32)
    dev = torch.device("cuda:0")
    q_d = torch.from_numpy(Q).to(dev)
    r_d = torch.from_numpy(R).to(dev)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    pkg.keys_init(keys.data_ptr(), m, stream=stream)
    idxs = []
    for lo, hi in pkg.shard_bounds(n, 3):
        ix = pkg.KnnIndex(k, r_d.data_ptr() + lo * k * 4, n_local=hi - lo, base_index=lo, refs_on_device=True,
                          stream=stream)
        ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), stream=stream)
        idxs.append(ix)
    pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Q, R))
    # keys carry the exact v0 distance bits
    kk = keys.cpu().numpy().view(np.uint64)
    j = 17
    d2 = np.array([kk[j] >> np.uint64(32)], dtype=np.uint64).astype(np.uint32).view(np.float32)[0]
    assert d2 == np.float32(oracle.dist2(Q[j * k:(j + 1) * k], R[int(out[j]) * k:(int(out[j]) + 1) * k]))
    for ix in idxs:
        ix.close()


def _filter_case(rng, name, m, n, k):
    if name == "uniform":
        return rng.random((m, k), dtype=np.float32), rng.random((n, k), dtype=np.float32)
    if name == "offset":      # far from the origin: centring must absorb it
        return ((rng.random((m, k)) * 3 + 1000).astype(np.float32),
                (rng.random((n, k)) * 3 + 1000).astype(np.float32))
    if name == "clustered":
        c = rng.random((5, k))
        return ((c[rng.integers(0, 5, m)] + rng.normal(0, 1e-3, (m, k))).astype(np.float32),
                (c[rng.integers(0, 5, n)] + rng.normal(0, 1e-3, (n, k))).astype(np.float32))
    if name == "mixed_scales":  # per-dimension scales differ by 1e4: small dims fall into fp16 subnormals
        sc = np.logspace(-4, 0, k)
        return ((rng.normal(0, 1, (m, k)) * sc).astype(np.float32), (rng.normal(0, 1, (n, k)) * sc).astype(np.float32))
    if name == "queries_outside":  # queries well outside the references' bounding box
        return ((rng.random((m, k)) * 40 - 20).astype(np.float32), rng.random((n, k)).astype(np.float32))
    raise ValueError(name)


@pytest.mark.parametrize("k", [3, 16, 24, 100, 200, 500, 700, 1100])
@pytest.mark.parametrize("dist", ["uniform", "offset", "clustered", "mixed_scales", "queries_outside"])
def test_filter_scores_stay_inside_the_proven_error_bound(k, dist):
    """The MFMA filter is only sound if |S + M - sigma^2 d^2| <= 2 eta sigma d + eta^2 + rho for
    EVERY pair (knn_filter.hip header).  Checked against a float64 evaluation of the true distance;
    also checks the fragment layout (a swapped row/column map breaks it at once)."""
    rng = np.random.default_rng(k * 7 + len(dist))
    m, n = 70, 1500
    Q, R = _filter_case(rng, dist, m, n, k)
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    pkg.set_option("path", 2)
    try:
        ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    finally:
        pkg.set_option("path", 0)
    scores = torch.full((m, n), float("nan"), dtype=torch.float32, device=dev)
    qn = torch.empty(m, dtype=torch.float32, device=dev)
    sigma, eta, rho, amax, bmax, g2, gam, qbad = ix.debug_filter_scores(m, q_d.data_ptr(), scores.data_ptr(),
                                                                          qn.data_ptr())
    torch.cuda.synchronize()
    ix.close()
    assert qbad == 0 and bmax <= 1.0
    S = scores.cpu().numpy().astype(np.float64)
    M = qn.cpu().numpy().astype(np.float64)
    # reference rows outside the robust box carry +INF scores (they are scanned exactly instead):
    # whole columns, and only a handful
    inside = np.isfinite(S).all(axis=0)
    assert (np.isfinite(S).any(axis=0) == inside).all() and inside.mean() > 0.98
    d2 = ((Q.astype(np.float64)[:, None, :] - R.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    D = sigma * sigma * d2
    err = np.abs(S + M[:, None] - D)[:, inside]
    bound = (2 * eta * np.sqrt(D) + eta * eta + rho + gam * M[:, None])[:, inside]
    D = D[:, inside]
    worst = float((err / bound).max())
    assert worst <= 1.0, (dist, k, worst)
    # the bound must not be vacuous either: on uniform data it stays a small fraction of D
    if dist == "uniform" and k == 16:
        assert float(np.median(bound / D)) < 0.05


def test_filter_path_is_taken_and_reports_candidates(oracle):
    k, m, n = 16, 1024, 1 << 20
    Q, R = oracle.synth(m * k, 1000), oracle.synth(n * k, 1001)
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)   # auto path
    pkg.keys_init(keys.data_ptr(), m)
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
    pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
    torch.cuda.synchronize()
    path_taken, records, fallback, _ = ix.last_stats()
    assert path_taken in (2, 4) and fallback == 0               # 4 = the cell-pruned form of the filter
    assert 0 < records < 400 * m          # ~n/sample survivors per query, far below m*n/32
    np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Q, R))
    ix.close()


@pytest.mark.parametrize("k,m,n", [(256, 2048, 32768), (512, 1024, 16384), (160, 100, 20000), (1024, 1024, 16384), (600, 300, 20001)])
def test_deep_dimensions_take_the_filter_and_stay_bit_exact(oracle, k, m, n):
    """128 < k <= 512 (the reference loops over any k, core.cu:831-835): library policy puts these on the MFMA filter
    (round 2 left them on the row-per-lane exact kernels); gaussian data, planted exact duplicates."""
    rng = np.random.default_rng(k + m)
    R = rng.normal(0, 1, (n, k)).astype(np.float32)
    Q = rng.normal(0, 1, (m, k)).astype(np.float32)
    Q[::7] = R[rng.integers(0, n, len(Q[::7]))]
    R[n - 1] = R[3]
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)   # auto path
    pkg.keys_init(keys.data_ptr(), m)
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
    pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
    torch.cuda.synchronize()
    path_taken, records, fallback, _ = ix.last_stats()
    ix.close()
    assert path_taken == 2 and fallback == 0 and records > 0
    np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Q, R, threads=THREADS))


def test_filter_falls_back_on_the_device_when_queries_rule_it_out(oracle):
    """NaN / Inf / far-away queries are detected on the GPU; the gated exact kernels then scan
    everything — no host round trip, same bit-exact answer."""
    k, m, n = 16, 256, 100000
    Q, R = oracle.synth(m * k, 5).reshape(m, k).copy(), oracle.synth(n * k, 6)
    dev = torch.device("cuda:0")
    r_d = torch.from_numpy(R).to(dev)
    pkg.set_option("path", 2)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    try:
        for what in ("nan", "inf", "far", "clean"):
            Qc = Q.copy()
            if what == "nan":
                Qc[7, 3] = np.nan
            elif what == "inf":
                Qc[9, 0] = np.inf
            elif what == "far":
                Qc[11] = 1e6
            q_d = torch.from_numpy(Qc).to(dev)
            pkg.keys_init(keys.data_ptr(), m)
            ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
            pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
            torch.cuda.synchronize()
            path_taken, records, fallback, _ = ix.last_stats()
            assert path_taken in (2, 4)
            assert (fallback != 0) == (what != "clean"), (what, fallback)
            np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Qc, R), err_msg=what)
    finally:
        pkg.set_option("path", 0)
        ix.close()


def test_device_synth_fill_matches_oracle_generator(oracle):
    x = torch.empty(100003, dtype=torch.float32, device="cuda:0")
    pkg.synth_fill_device(x.data_ptr(), x.numel(), 1001, first=12345,
                          stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(x.cpu().numpy(), oracle.synth(100003, 1001, first=12345))


def test_headline_shape_properties(oracle, path):
    """BASELINE config C3 (k=16, m=1024, n=2^24) at full size: checked through properties that do
    not need a full CPU scan — (1) a seeded subset of queries against the full reference set with
    the oracle, (2) planting an exact copy of each query makes that copy's index the answer,
    (3) splitting the set into shards and min-merging keys gives the same indices."""
    k, m, n = 16, 1024, 1 << 24
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    r_d = torch.empty(n * k, dtype=torch.float32, device=dev)
    q_d = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(r_d.data_ptr(), n * k, 1001, stream=stream)
    pkg.synth_fill_device(q_d.data_ptr(), m * k, 1000, stream=stream)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)

    def run(shards):
        pkg.keys_init(keys.data_ptr(), m, stream=stream)
        held = []
        for lo, hi in pkg.shard_bounds(n, shards):
            ix = pkg.KnnIndex(k, r_d.data_ptr() + lo * k * 4, n_local=hi - lo, base_index=lo,
                              refs_on_device=True, stream=stream)
            ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), stream=stream)
            held.append(ix)
        pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        for ix in held:
            ix.close()
        return out.cpu().numpy().copy()

    whole = run(1)
    np.testing.assert_array_equal(run(8), whole)
    # (1) 24 queries against all 2^24 references on the host
    R = r_d.cpu().numpy()
    Q = q_d.cpu().numpy()
    sel = np.random.default_rng(0).choice(m, 24, replace=False)
    want = oracle.v0(k, Q.reshape(m, k)[sel], R)
    np.testing.assert_array_equal(whole[sel], want)
    # (2) plant copies
    pos = np.random.default_rng(1).choice(n, m, replace=False)
    r2 = r_d.view(n, k)
    r2[torch.from_numpy(pos).to(dev)] = q_d.view(m, k)
    planted = run(1)
    np.testing.assert_array_equal(planted, pos.astype(np.int32))


def test_ta_style_harness_through_the_cpp_function_pointer_boundary(tmp_path, oracle):
    """a TA-style C++ harness (tests/harness/ta_harness.cpp, own code) selects the
    operator through CALLBACKn macros / a function pointer exactly like the reference's main.cu
    and must report 0 errors against its v0 baseline on all 8 samples; the indices it writes are
    the reference's results.csv index lines."""
    import subprocess
    hdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "harness")
    subprocess.check_call(["make", "-C", hdir], stdout=subprocess.DEVNULL)
    csv = tmp_path / "results_indices.csv"
    r = subprocess.run([os.path.join(hdir, "ta_harness"), str(csv)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("errors/total w.r.t. baseline: 0/") == 16
    assert "Callback10, 16, 1024, 65536," in r.stdout
    gold = read_golden_indices()
    lines = csv.read_text().splitlines()
    assert len(lines) == 2 * len(gold)                 # results.csv layout: index line, distance line
    for line, g in zip(lines[0::2], gold):
        assert [int(t) for t in line.split(",") if t] == g.tolist()
    # distance lines: the reference's own for samples 2-7 (its samples 0-1 are use-after-free values)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ta_distances.txt")) as f:
        gdist = [ln.split() for ln in f.read().splitlines() if ln and not ln.startswith("#")]
    for i, line in enumerate(lines[1::2]):
        mine = [t for t in line.split(",") if t]
        assert len(mine) == len(gdist[i])
        if i >= 2:
            assert mine == gdist[i], f"sample {i}"


@pytest.mark.parametrize("chain", [0, 1, 2], ids=["auto", "chained", "free"])
def test_workspace_slots_run_concurrent_batches_on_their_own_streams(oracle, chain):
    """knn_index_query_keys_slot: four different query batches in flight at once (slot b on stream b)
    against one index, repeated, with the scans chained or free to overlap; all stay bit-exact."""
    k, n = 16, 1 << 19
    R = oracle.synth(n * k, 77)
    dev = torch.device("cuda:0")
    r_d = torch.from_numpy(R).to(dev)
    pkg.set_option("filter_chain", chain)
    try:
        ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
        ms = (1024, 300, 77, 2000)
        Qs = [oracle.synth(ms[b] * k, 78 + b) for b in range(4)]
        q_d = [torch.from_numpy(q).to(dev) for q in Qs]
        keys = [torch.empty(m, dtype=torch.int64, device=dev) for m in ms]
        outs = [torch.empty(m, dtype=torch.int32, device=dev) for m in ms]
        streams = [torch.cuda.Stream(device=dev) for _ in range(4)]
        torch.cuda.synchronize()
        for _ in range(6):
            for b in range(4):
                s = streams[b].cuda_stream
                pkg.keys_init(keys[b].data_ptr(), ms[b], stream=s)
                ix.query_keys(ms[b], q_d[b].data_ptr(), keys[b].data_ptr(), stream=s, slot=b)
                pkg.keys_to_indices(keys[b].data_ptr(), ms[b], outs[b].data_ptr(), stream=s)
        torch.cuda.synchronize()
        for b in range(4):
            np.testing.assert_array_equal(outs[b].cpu().numpy(), oracle.v0(k, Qs[b], R), err_msg=f"slot {b}")
        ix.close()
    finally:
        pkg.set_option("filter_chain", 0)
    with pytest.raises(pkg.KnnError):
        ix2 = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
        try:
            ix2.query_keys(8, q_d[0].data_ptr(), keys[0].data_ptr(), slot=8)
        finally:
            ix2.close()


def test_one_far_away_query_does_not_loosen_the_whole_batch(oracle):
    """Thresholds use each query's own coordinate magnitude: a single query 100 box-widths away
    keeps the filter selective for the other 255 (and is itself answered exactly)."""
    k, m, n = 16, 256, 1 << 18
    Q, R = oracle.synth(m * k, 91).reshape(m, k).copy(), oracle.synth(n * k, 92)
    dev = torch.device("cuda:0")
    r_d = torch.from_numpy(R).to(dev)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    recs = {}
    for name, val in (("clean", None), ("outlier", 50.0)):
        Qc = Q.copy()
        if val is not None:
            Qc[5] = val
        q_d = torch.from_numpy(Qc).to(dev)
        pkg.keys_init(keys.data_ptr(), m)
        ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
        pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
        torch.cuda.synchronize()
        path_taken, records, fallback, _ = ix.last_stats()
        assert path_taken in (2, 4) and fallback == 0, (name, fallback)
        np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Qc, R), err_msg=name)
        recs[name] = records
    # the outlier's own threshold is loose (it may keep thousands of survivors); the rest are unchanged
    assert recs["outlier"] < recs["clean"] + 20000, recs
    ix.close()


@pytest.mark.parametrize("k", [16, 40, 128, 256, 512, 1024])
def test_mfma_accumulation_error_is_far_inside_the_assumed_allowance(k):
    """The one unproven constant of the filter bound is omega = kt * 2^-18: the matrix core's internal
    fp32 accumulation error relative to the sum of term magnitudes.  Measured here by rebuilding the
    exact fp16 operands on the host (same centring / scaling / rounding as knn_frag_kernel) and
    evaluating N - 2 a.b in float64."""
    rng = np.random.default_rng(k)
    m, n = 64, 2048
    Q = rng.normal(0, 1, (m, k)).astype(np.float32)
    R = rng.normal(0, 1, (n, k)).astype(np.float32)
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    pkg.set_option("path", 2)
    try:
        ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    finally:
        pkg.set_option("path", 0)
    scores = torch.empty((m, n), dtype=torch.float32, device=dev)
    qn = torch.empty(m, dtype=torch.float32, device=dev)
    sigma = np.float32(ix.debug_filter_scores(m, q_d.data_ptr(), scores.data_ptr(), qn.data_ptr())[0])
    torch.cuda.synchronize()
    ix.close()
    lo, hi = R.min(axis=0), R.max(axis=0)
    c = (np.float32(0.5) * lo + np.float32(0.5) * hi).astype(np.float32)
    b = ((R - c) * sigma).astype(np.float32).astype(np.float16)
    a2 = (((Q - c) * sigma).astype(np.float32).astype(np.float16).astype(np.float32) * np.float32(-2)).astype(np.float16)
    # reference norms as the kernel stores them: sequential fp32 sum of exact products
    bn = b.astype(np.float32)
    N = np.zeros(n, dtype=np.float32)
    for d in range(k):
        N = (N + bn[:, d] * bn[:, d]).astype(np.float32)
    terms = a2.astype(np.float64)[:, None, :] * b.astype(np.float64)[None, :, :]
    exact = N.astype(np.float64)[None, :] + terms.sum(-1)
    mag = np.abs(N.astype(np.float64))[None, :] + np.abs(terms).sum(-1)
    S = scores.cpu().numpy().astype(np.float64)
    rel = float((np.abs(S - exact) / mag).max())
    kt = 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8 if k <= 128 else 16 if k <= 256 else 32 if k <= 512 else 8 * ((k + 127) // 128)
    assert rel <= kt * 2.0 ** -18, rel
    assert rel <= 2.0 ** -20, rel   # in practice about one fp32 rounding per 16-wide K-step


def _kt_of(k):
    return 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8 if k <= 128 else 16 if k <= 256 else 32 if k <= 512 else 8 * ((k + 127) // 128)


OMEGA_CASES = ["alternating", "one_large_term", "subnormal_operands", "mixed_magnitudes"]
OMEGA_WORST = {}


@pytest.mark.parametrize("k", [16, 40, 128, 512, 1024, 4096])
@pytest.mark.parametrize("case", OMEGA_CASES)
def test_mfma_accumulation_error_on_adversarial_operands(case, k):
    """omega = kt * 2^-18 (knn_filter_dev.h) bounds the matrix core's internal accumulation of one score,
    relative to the sum of the magnitudes of what it adds (the norm and the k products).  The gaussian test above cannot see a
    worst case; these operands are built for one, every fp16 value exactly representable so that the float64 reference is
    exact:
      alternating        every row is one value in all dimensions, every query the same with alternating sign: the k products
                         of a pair are +P, -P, +P, ... — total cancellation against k P of magnitude
      one_large_term     dimension 0 of every 16-wide K-step spans [-1, 1], the other fifteen [-2^-5, 2^-5]: one product per
                         step is 2^10 times the others (alignment shifts in the adder tree)
      subnormal_operands the other fifteen dimensions span 2^-15: their fp16 operands are subnormal (a core that flushes them
                         loses those products entirely)
      mixed_magnitudes   magnitudes 2^0 .. 2^-12 cycling over the dimensions with random signs
    The assertion is the bound the threshold derivation uses; the worst figure seen goes into knn_filter_dev.h's comment."""
    rng = np.random.default_rng(k * 31 + len(case))
    m, n = (64, 2048) if k <= 1024 else (16, 512)
    grid = lambda size: (rng.integers(-512, 513, size) / 512.0).astype(np.float32)     # multiples of 2^-9 in [-1, 1]
    d = np.arange(k)
    if case == "alternating":
        R = np.repeat(grid((n, 1)), k, axis=1)
        Q = np.repeat(grid((m, 1)), k, axis=1) * np.where(d % 2 == 0, 1.0, -1.0).astype(np.float32)
        scale = np.ones(k, dtype=np.float32)
    else:
        if case == "one_large_term":
            scale = np.where(d % 16 == 0, 1.0, 2.0 ** -5).astype(np.float32)
        elif case == "subnormal_operands":
            scale = np.where(d % 16 == 0, 1.0, 2.0 ** -15).astype(np.float32)
        else:
            scale = (2.0 ** -(d % 13).astype(np.float64)).astype(np.float32)
        R = grid((n, k)) * scale
        Q = grid((m, k)) * scale
    R[0], R[1] = -scale, scale                           # the range of every dimension is symmetric: the centre is 0 exactly
    R, Q = np.ascontiguousarray(R, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    pkg.set_option("path", 2)
    try:
        ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    finally:
        pkg.set_option("path", 0)
    scores = torch.empty((m, n), dtype=torch.float32, device=dev)
    qn = torch.empty(m, dtype=torch.float32, device=dev)
    sigma = np.float32(ix.debug_filter_scores(m, q_d.data_ptr(), scores.data_ptr(), qn.data_ptr())[0])
    torch.cuda.synchronize()
    ix.close()
    lo, hi = R.min(axis=0), R.max(axis=0)
    c = (np.float32(0.5) * lo + np.float32(0.5) * hi).astype(np.float32)
    assert (c == 0).all() and sigma == np.float32(0.5), (sigma, np.abs(c).max())   # box [-1, 1]: scale 2^-1
    b32 = ((R - c) * sigma).astype(np.float32)
    b = b32.astype(np.float16)
    a32 = ((Q - c) * sigma).astype(np.float32)
    a2 = (a32.astype(np.float16).astype(np.float32) * np.float32(-2)).astype(np.float16)
    if case != "subnormal_operands":                     # every operand exactly representable (else: the nearest subnormal)
        assert (b.astype(np.float32) == b32).all() and (a2.astype(np.float32) == a32 * np.float32(-2)).all()
    else:
        tiny = np.abs(b.astype(np.float32)) < 2.0 ** -14
        assert tiny[:, d % 16 != 0].all() and (b != 0).any()
    bn = b.astype(np.float32)
    N = np.zeros(n, dtype=np.float32)
    for dd in range(k):
        N = (N + bn[:, dd] * bn[:, dd]).astype(np.float32)
    A, B = a2.astype(np.float64), b.astype(np.float64)
    exact = N.astype(np.float64)[None, :] + A @ B.T      # (products of fp16 values are exact in float64; the float64 sums of
    mag = np.abs(N.astype(np.float64))[None, :] + np.abs(A) @ np.abs(B).T   #  <= 4096 terms are good to 2^-40 of `mag`)
    S = scores.cpu().numpy().astype(np.float64)
    ok = mag > 0
    rel = float((np.abs(S - exact)[ok] / mag[ok]).max())
    kt = _kt_of(k)
    OMEGA_WORST[(case, k)] = rel
    print("omega %-20s k %5d kt %3d: worst |S - exact| / magnitudes = 2^%.2f (allowance kt 2^-18 = 2^%.2f)"
          % (case, k, kt, np.log2(max(rel, 1e-300)), np.log2(kt * 2.0 ** -18)))
    assert rel <= kt * 2.0 ** -18, (case, k, rel)


@pytest.mark.parametrize("k,m", [(16, 1), (16, 7), (16, 300), (3, 5), (8, 64)])
def test_device_pointers_that_are_only_4_byte_aligned(oracle, path, k, m):
    """A borrowed device reference set / query batch may start at any float: the 16-byte fast paths
    (rlane16, frag16, stats4) must step aside and the result stays bit-exact."""
    n = 70001
    R, Q = oracle.synth(n * k, 5), oracle.synth(m * k, 6)
    dev = torch.device("cuda:0")
    r_buf = torch.empty(n * k + 3, dtype=torch.float32, device=dev)
    q_buf = torch.empty(m * k + 3, dtype=torch.float32, device=dev)
    for off in (1, 3):
        r_buf[off:off + n * k] = torch.from_numpy(R).to(dev)
        q_buf[off:off + m * k] = torch.from_numpy(Q).to(dev)
        keys = torch.empty(m, dtype=torch.int64, device=dev)
        out = torch.empty(m, dtype=torch.int32, device=dev)
        ix = pkg.KnnIndex(k, r_buf.data_ptr() + 4 * off, n_local=n, refs_on_device=True)
        pkg.keys_init(keys.data_ptr(), m)
        ix.query_keys(m, q_buf.data_ptr() + 4 * off, keys.data_ptr())
        pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
        torch.cuda.synchronize()
        ix.close()
        np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Q, R), err_msg=f"offset {off} floats")


def test_many_queries_few_references(oracle, path):
    k, m, n = 16, 70000, 3000
    Q, R = oracle.synth(m * k, 8), oracle.synth(n * k, 9)
    np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), oracle.v0(k, Q, R))


@pytest.mark.parametrize("k", [16, 5])
def test_far_out_reference_rows_are_scanned_exactly_not_allowed_to_stretch_the_box(oracle, k):
    """Robust box: a few reference rows far outside mean +- 8 sigma leave the filter (listed, scanned
    exactly each query) instead of coarsening the fp16 grid for everybody — including when one of them
    IS the nearest neighbour of a query."""
    rng = np.random.default_rng(17 + k)
    m, n = 300, 200000
    R = rng.normal(0, 1, (n, k)).astype(np.float32)
    far = rng.choice(n, 500, replace=False)
    R[far] *= np.float32(300.0)                       # heavy tail: 500 rows ~300 sigma out
    R[far[:3], 0] = np.float32(1e30)                  # and a few beyond fp16 range after scaling
    Q = rng.normal(0, 1, (m, k)).astype(np.float32)
    Q[:20] = R[far[10:30]] + np.float32(0.25)         # queries whose nearest neighbour is an outlier row
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    pkg.keys_init(keys.data_ptr(), m)
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
    pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
    torch.cuda.synchronize()
    path_taken, records, fallback, n_out = ix.last_stats()
    ix.close()
    want = oracle.v0(k, Q, R)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert path_taken in (2, 4) and 400 <= n_out <= 2000, (path_taken, n_out)
    assert np.isin(want[:20], far).sum() >= 15        # the planted queries really resolve to outlier rows


@pytest.mark.parametrize("k", [17, 16, 40])
def test_repeated_filter_launches_never_miss_a_survivor(oracle, k):
    """Regression: small reference sets make every missed filter record visible (each 32-row tile
    holds ~1-3 % of the answers).  A stale MFMA accumulator read in the last query tile of a group
    (k = 17: two chained MFMAs, no independent one behind them) used to lose one about once in 60
    launches; tools/mfma_hazard_audit.py is the static half of this test."""
    pkg.set_option("path", 2)
    try:
        for (m, n) in [(1500, 777), (700, 3001), (1024, 1024)]:
            rng = np.random.default_rng(k * 100003 + m * 1009 + n)
            Q = rng.random((m, k), dtype=np.float32)
            R = rng.random((n, k), dtype=np.float32)
            want = oracle.v0(k, Q, R)
            for rep in range(40):
                got = pkg.cudaCallback(k, m, n, Q, R)
                np.testing.assert_array_equal(got, want, err_msg=f"rep {rep} shape {(m, n)}")
    finally:
        pkg.set_option("path", 0)


def test_pooled_staging_buffers_are_reused_and_can_be_trimmed(oracle):
    """Host-input calls keep their device staging buffers between calls (knn_trim releases them):
    a sequence of calls with growing, shrinking and equal sizes stays bit-exact, and the pool holds
    something afterwards."""
    pkg.trim()
    rng = np.random.default_rng(99)
    for (k, m, n) in [(16, 100, 5000), (16, 100, 5000), (3, 1000, 40000), (16, 64, 300), (8, 7, 100000),
                      (16, 100, 5000), (16, 1024, 70000)]:
        Q = rng.random((m, k), dtype=np.float32)
        R = rng.random((n, k), dtype=np.float32)
        np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), oracle.v0(k, Q, R), err_msg=str((k, m, n)))
    held = pkg.trim()
    assert held > 0
    assert pkg.trim() == 0
    Q = rng.random((50, 4), dtype=np.float32)
    R = rng.random((999, 4), dtype=np.float32)
    np.testing.assert_array_equal(pkg.cudaCallback(4, 50, 999, Q, R), oracle.v0(4, Q, R))


@pytest.mark.parametrize("k,m,n", [(16, 1024, 1200001), (3, 77, 6 << 20), (16, 5, 1 << 20), (33, 130, 700000)])
def test_streamed_one_shot_scan_matches_v0(oracle, k, m, n):
    """cudaCallback's chunked path (exact scan of each chunk under the copy of the next): forced on,
    alone and with the reference set split into several shards, against the staged paths."""
    Q, R = oracle.synth(m * k, 31), oracle.synth(n * k, 32)
    R[(n // 2) * k:(n // 2 + 1) * k] = R[:k]          # a duplicate row in a later chunk: lower index must win
    want = oracle.v0(k, Q, R)
    try:
        for stream, shards in [(2, 0), (2, 3), (1, 0), (0, 0)]:
            pkg.set_option("stream", stream)
            pkg.set_option("shards", shards)
            np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), want, err_msg=f"stream={stream} shards={shards}")
    finally:
        pkg.set_option("stream", 0)
        pkg.set_option("shards", 0)


def test_randomised_differential_cases_against_the_oracle(oracle):
    """tools/fuzz_parity.py, 80 seeded cases: random k, m, n, data distribution (ties, clusters, heavy
    tails, offsets, a stray NaN/Inf), forced path, shard count and one-shot strategy."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(__file__), "..", "tools",
                                                                               "fuzz_parity.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    rng = np.random.default_rng(2026)
    try:
        for case in range(80):
            assert fuzz.one_case(oracle, rng, case), case
    finally:
        for name in ("path", "shards", "stream"):
            pkg.set_option(name, 0)


@pytest.mark.parametrize("k,expect_filter", [(17, False), (16, False), (100, True)])
def test_index_policy_builds_the_filter_early_for_dimensions_without_a_compiled_exact_kernel(oracle, k, expect_filter):
    """Resident index of 20000 rows: k = 16 (compile-time exact kernel) and k = 17 (run-time-k form of
    it) stay exact below 65536 rows; k = 100 costs 303 exact lane-ops per pair at one query per lane, so
    the MFMA filter is built and used from 4096 rows.  Either way indices are bit-exact."""
    m, n = 600, 20000
    Q, R = oracle.synth(m * k, 41), oracle.synth(n * k, 42)
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    pkg.keys_init(keys.data_ptr(), m)
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
    pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
    torch.cuda.synchronize()
    path_taken = ix.last_stats()[0]
    ix.close()
    np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Q, R))
    assert (path_taken in (2, 4)) == expect_filter, path_taken


def test_rccl_exchange_step_with_a_one_device_communicator(oracle):
    """The library's own collective (knn_rccl.cpp): ncclCommInitAll + ncclAllReduce(uint64, min) in a
    group, here with the one GPU a test box has.  (a) the exported knn_keys_allreduce_min leaves a
    1-rank reduction unchanged and rejects a device list with repeats; (b) cudaCallback with option
    rccl = 1 merges through RCCL (counted) and stays bit-exact, for the staged and the streamed
    one-shot paths; (c) rccl = 2 and more shards than devices take the host merge."""
    dev = torch.device("cuda:0")
    assert pkg.get_option("rccl_version") >= 20000           # librccl could be opened
    m = 1000
    keys = torch.randint(0, 2**62, (m,), dtype=torch.int64, device=dev)
    before = keys.clone()
    pkg.keys_allreduce_min([0], [keys.data_ptr()], m, streams=[torch.cuda.current_stream().cuda_stream])
    torch.cuda.synchronize()
    assert torch.equal(keys, before)
    with pytest.raises(pkg.KnnError):
        pkg.keys_allreduce_min([0, 0], [keys.data_ptr(), keys.data_ptr()], m)
    with pytest.raises(pkg.KnnError):
        pkg.keys_allreduce_min([7], [keys.data_ptr()], m)     # no such device here
    try:
        for (k, mm, n, stream) in [(16, 300, 70001, 0), (3, 1024, 1 << 20, 0), (16, 64, 1200001, 2), (5, 1, 7, 0)]:
            Q, R = oracle.synth(mm * k, 51), oracle.synth(n * k, 52)
            want = oracle.v0(k, Q, R)
            pkg.set_option("stream", stream)
            pkg.set_option("rccl", 1)
            done = pkg.get_option("rccl_reductions")
            np.testing.assert_array_equal(pkg.cudaCallback(k, mm, n, Q, R), want, err_msg=f"rccl {(k, mm, n)}")
            assert pkg.get_option("rccl_reductions") == done + 1
            pkg.set_option("rccl", 2)
            np.testing.assert_array_equal(pkg.cudaCallback(k, mm, n, Q, R), want)
            pkg.set_option("rccl", 0)
            pkg.set_option("shards", 3)                       # more shards than GPUs: host merge
            np.testing.assert_array_equal(pkg.cudaCallback(k, mm, n, Q, R), want)
            pkg.set_option("shards", 0)
            assert pkg.get_option("rccl_reductions") == done + 1
    finally:
        for name in ("rccl", "shards", "stream"):
            pkg.set_option(name, 0)


def test_ta_sequence_uses_one_gpu_per_call_and_at_most_one_communicator_set(oracle, capfd):
    """the TA harness' eight samples (n = 2, 8, 1024, 65536, ...) in sequence.  Round 3 fanned each of them
    out over every visible GPU and kept one RCCL communicator set per device list it met ({0, 1} for n = 2, {0..7} after).
    Now: every TA sample is one shard (the reference's rule, core.cu:871-872), the trace line says so, and however the
    calls vary the process holds at most ONE communicator set — also with rccl = 1 forcing the exchange step."""
    os.environ["KNN_MI355X_TRACE_CALL"] = "1"    # (read once per process: set before the first cudaCallback of the suite matters
    try:                                         #  only for the trace assertion below, which is skipped when it came too late)
        for rccl in (0, 1):
            pkg.set_option("rccl", rccl)
            for i, (k, m, n, Q, R) in enumerate(oracle.ta_samples()):
                np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), oracle.v0_serial(k, Q, R), err_msg=f"TA sample {i}")
                assert pkg.get_option("last_shards") == 1, (i, k, m, n)
                assert pkg.get_option("rccl_comm_sets") <= 1
        # a large one-shot call on this node: every visible GPU (here: the one there is)
        k, m, n = 16, 64, 1200001
        Q, R = oracle.synth(m * k, 51), oracle.synth(n * k, 52)
        np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), oracle.v0(k, Q, R))
        assert pkg.get_option("last_shards") == pkg.debug_shard_policy(k, m, n, pkg.device_count())
        assert pkg.get_option("rccl_comm_sets") <= 1
        # a reduction over another device list than the process' set is refused, not answered with a second set
        if pkg.get_option("rccl_comm_sets") == 1 and pkg.device_count() > 1:
            keys = torch.zeros(8, dtype=torch.int64, device=torch.device("cuda:1"))
            with pytest.raises(pkg.KnnError):
                pkg.keys_allreduce_min([1], [keys.data_ptr()], 8)
        err = capfd.readouterr().err
        if "[knn call]" in err:
            assert "-> 1 shard(s)" in err
    finally:
        del os.environ["KNN_MI355X_TRACE_CALL"]
        pkg.set_option("rccl", 0)


def test_a_failing_rccl_reduction_falls_back_to_the_host_merge(oracle):
    """in the automatic mode a run-time RCCL failure (communicator creation on a node it does not
    like, a failed collective) must not end the process — the reduction writes to scratch buffers, so the shards' keys are
    still what the scans left and the host merge takes over.  The test hook KNN_MI355X_TEST_RCCL_FAIL makes the reduction
    fail after the shards have run; on a one-GPU box that code is only reachable with rccl = 1, whose own reaction (the
    reference's print-and-exit) the hook replaces by the automatic mode's."""
    k, m, n = 16, 257, 150001
    Q, R = oracle.synth(m * k, 61), oracle.synth(n * k, 62)
    want = oracle.v0(k, Q, R)
    done = pkg.get_option("rccl_reductions")
    os.environ["KNN_MI355X_TEST_RCCL_FAIL"] = "1"
    try:
        pkg.set_option("rccl", 1)
        np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), want)
        assert pkg.get_option("rccl_reductions") == done      # nothing was reduced by RCCL: the host merged
    finally:
        del os.environ["KNN_MI355X_TEST_RCCL_FAIL"]
        pkg.set_option("rccl", 0)
    pkg.set_option("rccl", 1)
    try:
        np.testing.assert_array_equal(pkg.cudaCallback(k, m, n, Q, R), want)
        assert pkg.get_option("rccl_reductions") == done + 1  # and without the hook RCCL does reduce
    finally:
        pkg.set_option("rccl", 0)


def test_grid_index_on_one_live_axis_with_hundreds_of_thousands_of_cells(oracle):
    """k = 1 (and k <= 4 with one varying axis) gives the grid up to 2^19 cells on its one axis, where the
    fp32 cell assignment is off by a visible fraction of a cell; the stop rule's allowance has to cover that
    (tests/test_grid_logic.py restates the rule on the CPU).  Here the device: a box not anchored at 0, a sparse stretch,
    every answer against the oracle."""
    rng = np.random.default_rng(12)
    n, m = 1 << 21, 4096
    x = (3.7 + 2.0 * rng.random(n)).astype(np.float32)
    keep = (np.abs(x - np.float32(5.5)) > 0.1) | (rng.random(n) < 0.02)
    R1 = x[keep]
    Q1 = (3.7 + 2.0 * rng.random(m)).astype(np.float32)
    for k in (1, 3):
        if k == 1:
            R, Q = R1.reshape(-1, 1), Q1.reshape(-1, 1)
        else:                                    # one varying axis among three
            R = np.zeros((len(R1), 3), dtype=np.float32)
            R[:, 1] = R1
            R[:, 0] = np.float32(0.25)
            R[:, 2] = np.float32(-7.0)
            Q = np.zeros((m, 3), dtype=np.float32)
            Q[:, 1] = Q1
            Q[:, 0] = np.float32(0.25)
            Q[:, 2] = np.float32(-7.0)
        want = oracle.v0(k, Q, R, threads=THREADS)
        ix = pkg.KnnIndex(k, R)
        try:
            got = ix.query(Q)
            st = ix.last_stats()
        finally:
            ix.close()
        assert st[0] == 3, st                    # served by the grid index
        np.testing.assert_array_equal(got, want, err_msg=f"k={k}")


@pytest.mark.parametrize("k,m,n", [(16, 1024, 3_300_001), (3, 700, 6 << 20), (40, 600, 900_000)])
def test_ingest_builds_the_layouts_chunk_by_chunk_under_the_copy(oracle, k, m, n):
    """an index created from HOST rows ships them in chunks and builds every chunk's MFMA
    layouts as it lands, with the robust box taken from a strided host sample.  Checked against the oracle
    and against the copy-then-build path, with the cases a sampled box must survive: far-out rows, NaN and
    Inf rows that only show up in LATE chunks (one of them the nearest neighbour of a query), duplicates
    across chunks (lowest index wins)."""
    rng = np.random.default_rng(n + k)
    R = oracle.synth(n * k, 61).reshape(n, k).copy()
    Q = oracle.synth(m * k, 62).reshape(m, k).copy()
    late = n - 1 - rng.choice(n // 8, 40, replace=False)          # rows of the last chunk
    R[late[:10]] *= np.float32(500.0)                              # far outside the sampled box
    R[late[10:14], 0] = np.nan
    R[late[14:18], k - 1] = np.inf
    R[late[18]] = np.float32(1e30)
    Q[:5] = R[late[:5]] + np.float32(0.5)                          # nearest neighbour = a far-out late row
    R[late[20]] = R[3]                                             # duplicate of an early row: index 3 must win
    Q[5] = R[3]
    want = oracle.v0(k, Q, R)
    assert np.isin(want[:5], late[:10]).all() and want[5] == 3
    try:
        # (ingest, cells): layouts under the copy / copy then build, both without the cell sort (which needs the
        # whole shard resident and therefore always copies first), then the library's own policy
        for ingest, cells in ((0, 2), (1, 2), (0, 0)):
            pkg.set_option("ingest", ingest)
            pkg.set_option("cells", cells)
            pkg.set_option("path", 2)
            ix = pkg.KnnIndex(k, R)                                 # host rows
            pkg.set_option("path", 0)
            got = ix.query(Q)
            st = ix.last_stats()
            ix.close()
            np.testing.assert_array_equal(got, want, err_msg=f"ingest={ingest} cells={cells}")
            # the filter ran (NaN / Inf rows are outliers like any other), no device fallback
            assert st[0] == (4 if cells == 0 and k <= 16 else 2), (ingest, cells, st)
            # (copy-then-build — which the cell sort uses too — takes its box from the full range, which the far-out
            # rows stretch to 12 MADs: the five far-away queries may then overflow the candidate lists at k = 3 and
            # the exact scan answers the batch; the sampled box of the ingest path keeps them inside the lists)
            assert st[2] == 0 or ingest == 1 or cells == 0, (ingest, cells, st)
            assert 10 <= st[3] <= 4096, st                          # the planted rows are on the exact list
    finally:
        pkg.set_option("ingest", 0)
        pkg.set_option("cells", 0)
        pkg.set_option("path", 0)


def test_ingest_stays_exact_when_the_sample_misses_the_data(oracle):
    """A reference set whose rows sit far outside what a strided sample sees (every row NOT on the sample
    stride is scaled by 50): the sampled box would send almost everything to the exact list.  The build
    notices (more than n/32 outliers), redoes the layouts from the resident rows with full-range
    statistics, and — this data defeats that box too — ends on the exact kernels.  Never a wrong index."""
    k, m, n = 16, 300, 1 << 20
    R = oracle.synth(n * k, 71).reshape(n, k).copy()
    Q = oracle.synth(m * k, 72).reshape(m, k).copy()
    stride = n // 16384
    mask = np.ones(n, dtype=bool)
    mask[::stride] = False
    R[mask] *= np.float32(50.0)
    Q *= np.float32(50.0)
    pkg.set_option("path", 2)
    try:
        ix = pkg.KnnIndex(k, R)
        got = ix.query(Q)
        st = ix.last_stats()
        ix.close()
    finally:
        pkg.set_option("path", 0)
    np.testing.assert_array_equal(got, oracle.v0(k, Q, R))
    assert st[0] in (1, 2) and st[3] <= n // 32, st


def _grid_cases(rng, name, m, n, k):
    if name == "uniform":
        return rng.random((m, k), dtype=np.float32), rng.random((n, k), dtype=np.float32)
    if name == "offset":        # far from the origin: fp32 spacing is a visible fraction of a cell
        return ((rng.random((m, k)) + 4096).astype(np.float32), (rng.random((n, k)) + 4096).astype(np.float32))
    if name == "clustered":     # most cells empty, a few crowded: long ring walks and big cells
        c = rng.random((6, k))
        return ((c[rng.integers(0, 6, m)] + rng.normal(0, 2e-3, (m, k))).astype(np.float32),
                (c[rng.integers(0, 6, n)] + rng.normal(0, 2e-3, (n, k))).astype(np.float32))
    if name == "lattice":       # integer coordinates: massive exact ties, the lowest index must win
        return rng.integers(0, 12, (m, k)).astype(np.float32), rng.integers(0, 12, (n, k)).astype(np.float32)
    if name == "queries_outside":   # far outside the box (the ring search gives up: gated brute force) and just outside
        q = rng.random((m, k)) * 3 - 1
        q[: m // 4] = rng.random((m // 4, k)) * 2000 - 1000
        return q.astype(np.float32), rng.random((n, k)).astype(np.float32)
    if name == "skewed":        # one axis 1e4 times longer than the others, heavy-tailed
        sc = np.ones(k)
        sc[0] = 1e4
        return ((rng.standard_cauchy((m, k)) * sc).astype(np.float32), (rng.standard_cauchy((n, k)) * sc).astype(np.float32))
    raise ValueError(name)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("dist", ["uniform", "offset", "clustered", "lattice", "queries_outside", "skewed"])
def test_grid_index_for_low_k_is_bit_exact(oracle, k, dist):
    """the uniform-grid index (k <= 4) against the oracle — ring search with the stop rule
    `best < LB^2 (1 - 1e-6)`, ties by lowest index, queries outside the box, crowded and empty cells,
    NaN / Inf queries, several shards folding into one key array with global indices."""
    rng = np.random.default_rng(1000 * k + len(dist))
    m, n = 700, 150_000
    Q, R = _grid_cases(rng, dist, m, n, k)
    Q[3, 0] = np.nan
    Q[5, k - 1] = np.inf
    R[n // 2] = R[7]                    # duplicate row: index 7 must win over n // 2
    Q[9] = R[7]
    want = oracle.v0(k, Q, R)
    assert want[9] <= 7 and want[3] == 0 and want[5] == 0
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)
    pkg.set_option("path", 3)
    try:
        for shards in (1, 3):
            pkg.keys_init(keys.data_ptr(), m)
            paths = []
            for lo, hi in pkg.shard_bounds(n, shards):
                ix = pkg.KnnIndex(k, r_d.data_ptr() + lo * k * 4, n_local=hi - lo, base_index=lo, refs_on_device=True)
                ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
                torch.cuda.synchronize()
                paths.append(ix.last_stats()[0])
                ix.close()
            pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{dist} k={k} shards={shards}")
            if dist in ("uniform", "offset", "queries_outside"):
                assert paths == [3] * shards, paths          # the grid really was the path taken
    finally:
        pkg.set_option("path", 0)


def test_grid_index_is_the_resident_path_at_c2_scale_and_steps_aside_for_bad_data(oracle):
    """Policy: a resident shard with k <= 4 and >= 16384 rows is served by the grid (C2: k 3, n 2^20); rows
    with NaN / Inf, identical rows and tiny shards are not — the brute-force kernels take those."""
    k, m, n = 3, 1024, 1 << 20
    Q, R = oracle.synth(m * k, 1000), oracle.synth(n * k, 1001)
    dev = torch.device("cuda:0")
    q_d = torch.from_numpy(Q).to(dev)
    keys = torch.empty(m, dtype=torch.int64, device=dev)
    out = torch.empty(m, dtype=torch.int32, device=dev)

    def run(Rh, nn):
        r_d = torch.from_numpy(np.ascontiguousarray(Rh)).to(dev)
        ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=nn, refs_on_device=True)
        pkg.keys_init(keys.data_ptr(), m)
        ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
        pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
        torch.cuda.synchronize()
        st = ix.last_stats()
        ix.close()
        return out.cpu().numpy().copy(), st[0]

    got, path = run(R, n)
    np.testing.assert_array_equal(got, oracle.v0(k, Q, R, threads=16))
    assert path == 3
    Rb = R.reshape(n, k).copy()
    Rb[12345, 1] = np.nan
    got, path = run(Rb, n)
    np.testing.assert_array_equal(got, oracle.v0(k, Q, Rb, threads=16))
    assert path != 3
    Rc = np.tile(R[:k], (70000, 1))                      # every row identical: no box to grid
    got, path = run(Rc, 70000)
    np.testing.assert_array_equal(got, np.zeros(m, dtype=np.int32))
    assert path != 3
    got, path = run(R[:5000 * k], 5000)
    np.testing.assert_array_equal(got, oracle.v0(k, Q, R[:5000 * k]))
    assert path != 3


def test_deep_k_scan_is_bit_exact_on_ragged_shapes(oracle):
    """The LDS-tiled scan for 32 < k <= 128 (four reference tiles per barrier by LDS-DMA above k = 64): indices and row
    masks on shapes that leave tiles, query groups and K-steps ragged."""
    try:
        for (k, m, n) in [(128, 2048, 40000), (100, 1000, 70001), (65, 600, 9000), (40, 1500, 33333)]:
            Q, R = oracle.synth(m * k, 81), oracle.synth(n * k, 82)
            dev = torch.device("cuda:0")
            q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
            keys = torch.empty(m, dtype=torch.int64, device=dev)
            out = torch.empty(m, dtype=torch.int32, device=dev)
            pkg.set_option("path", 2)
            ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
            pkg.keys_init(keys.data_ptr(), m)
            ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())     # (path stays forced: shards below 65536 rows)
            pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
            torch.cuda.synchronize()
            st = ix.last_stats()
            ix.close()
            pkg.set_option("path", 0)
            np.testing.assert_array_equal(out.cpu().numpy(), oracle.v0(k, Q, R), err_msg=str((k, m, n)))
            assert st[0] in (2, 4) and st[2] == 0, st
    finally:
        pkg.set_option("path", 0)


def test_grid_index_give_up_flag_is_reset_between_batches_on_a_slot(oracle):
    """The flag that un-gates the brute-force scan behind the grid query lives in two alternating words per
    workspace slot (no memset between batches): batches with far-outside queries (flag raised) and batches without
    alternate on one index and one slot, and on two slots in flight; every answer stays bit-exact."""
    k, m, n = 3, 256, 200_000
    rng = np.random.default_rng(123)
    R = rng.random((n, k), dtype=np.float32)
    near = [rng.random((m, k), dtype=np.float32) for _ in range(3)]
    far = [(rng.random((m, k)) * 4000 - 2000).astype(np.float32) for _ in range(3)]
    batches = [near[0], far[0], far[1], near[1], far[2], near[2], near[0]]
    dev = torch.device("cuda:0")
    r_d = torch.from_numpy(R).to(dev)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    outs = []
    for j, Q in enumerate(batches):
        slot = j % 2 if j >= 3 else 0
        st = streams[slot]
        q_d = torch.from_numpy(Q).to(dev)
        keys = torch.empty(m, dtype=torch.int64, device=dev)
        out = torch.empty(m, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        pkg.keys_init(keys.data_ptr(), m, stream=st.cuda_stream)
        ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), stream=st.cuda_stream, slot=slot)
        pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr(), stream=st.cuda_stream)
        outs.append((out, q_d, keys))
    torch.cuda.synchronize()
    assert ix.last_stats()[0] == 3
    ix.close()
    for j, Q in enumerate(batches):
        np.testing.assert_array_equal(outs[j][0].cpu().numpy(), oracle.v0(k, Q, R), err_msg=f"batch {j}")


@pytest.mark.parametrize("k,nindexes", [(16, 1), (20, 2)], ids=["one_index", "two_indexes_k20"])
def test_one_index_driven_from_several_host_threads(oracle, k, nindexes):
    """Round 2 documented "one index, one host thread"; the index now serialises its callers.  Four threads, each with
    its own slot, stream and batch, 20 calls each on ONE index (ctypes drops the GIL inside the library): every answer is
    v0's.  two_indexes_k20: thread t queries index t % 2 with batches of 1024 (even t) or 800 (odd t) queries — the NIF scan
    of both asks for more than the default 64 KiB of LDS, a different amount each, and the kernel's limit is the device's:
    it must never drop under a launch of the other index (one index's mutex covers only its own calls)."""
    import threading
    n = 1 << 18
    R = oracle.synth(n * k, 77)
    dev = torch.device("cuda:0")
    r_d = torch.from_numpy(R).to(dev)
    pkg.set_option("cells", 1)
    try:
        ixs = [pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True) for _ in range(nindexes)]
    finally:
        pkg.set_option("cells", 0)
    nthreads, rounds = 4, 20
    ms = [512] * nthreads if nindexes == 1 else [1024 if t % 2 == 0 else 800 for t in range(nthreads)]
    Qs = [oracle.synth(ms[t] * k, 300 + t).reshape(ms[t], k) for t in range(nthreads)]
    wants = [oracle.v0(k, Q, R, threads=THREADS) for Q in Qs]
    errors = []

    def worker(t):
        try:
            m, ix = ms[t], ixs[t % nindexes]
            st = torch.cuda.Stream(device=dev)
            q_d = torch.from_numpy(Qs[t]).to(dev)
            keys = torch.empty(m, dtype=torch.int64, device=dev)
            out = torch.empty(m, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for _ in range(rounds):
                ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), stream=st.cuda_stream, slot=t, init_keys=True)
                pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr(), stream=st.cuda_stream)
                st.synchronize()
                if not (out.cpu().numpy() == wants[t]).all():
                    errors.append((t, "mismatch"))
                    return
                if ix.last_stats()[0] != 4:
                    errors.append((t, "not the pruned scan", ix.last_stats()))
                    return
        except Exception as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for ix in ixs:
        ix.close()
    assert not errors, errors


def test_rccl_always_refuses_a_call_whose_shards_are_not_the_visible_devices():
    """option rccl = 1 is documented as "always; the call dies when RCCL cannot serve".  A call split over another
    number of GPUs than are visible (option `shards`, or the policy picking fewer) has no communicator set: round 4 merged it
    on the host in silence.  Now it prints the reference's error line and exits 1 (child process: the entry point exit()s)."""
    import subprocess
    import sys
    child = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import multicore_hw2_amd as pkg\n"
        "pkg.set_option('rccl', 1)\n"
        "pkg.set_option('shards', pkg.device_count() + 2)\n"
        "rng = np.random.default_rng(1)\n"
        "Q, R = rng.random(16 * 8, dtype=np.float32), rng.random(16 * 4000, dtype=np.float32)\n"
        "pkg.cudaCallback(16, 8, 4000, Q, R)\n"
        "print('returned')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "returned" not in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-300:])
    assert "rccl = 1 but the call's shards are not the visible devices" in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("dist", ["uniform", "gaussian", "near_copies", "far_queries"])
@pytest.mark.parametrize("k,m,n", [(128, 4096, 65536), (100, 1000, 70001), (72, 2500, 40000), (256, 4096, 65536), (400, 2048, 33000)])
def test_thresholds_that_tighten_during_the_deep_k_launch_keep_every_answer(oracle, dist, k, m, n):
    """Round 5: for 64 < k <= 512 every score below a query's threshold is also a new bound for that
    query — threshold' = max(floor, score + margin), shared between the blocks that scan other tile ranges for the same
    queries through atomic minima on one word per query (knn_thr_kernel has the derivation).  Same answers as v0 with the
    running thresholds on (default) and off (option run_thresholds = 2), FEWER re-ranked candidates with them on; near
    copies (answers at distance ~0: the clamp region of the threshold function, where the floor takes over) and far-away
    queries (thresholds that let most rows through) are the edge cases of the margin argument."""
    rng = np.random.default_rng(k + m)
    if dist == "uniform":
        Q, R = oracle.synth(m * k, 91).reshape(m, k), oracle.synth(n * k, 92).reshape(n, k)
    elif dist == "gaussian":
        Q, R = rng.normal(0, 1, (m, k)).astype(np.float32), rng.normal(0, 1, (n, k)).astype(np.float32)
    elif dist == "near_copies":
        R = oracle.synth(n * k, 92).reshape(n, k).copy()
        Q = (R[rng.integers(0, n, m)] + rng.normal(0, 1e-4, (m, k))).astype(np.float32)
        Q[::7] = R[rng.integers(0, n, len(Q[::7]))]                      # exact copies too
    else:
        R = oracle.synth(n * k, 92).reshape(n, k)
        Q = oracle.synth(m * k, 91).reshape(m, k).copy()
        Q[: m // 4] = (Q[: m // 4] * 3.0 - 1.0).astype(np.float32)       # a quarter of the queries outside the references' box
    Q, R = np.ascontiguousarray(Q), np.ascontiguousarray(R)
    want = oracle.v0(k, Q, R)
    dev = torch.device("cuda:0")
    q_d, r_d = torch.from_numpy(Q).to(dev), torch.from_numpy(R).to(dev)
    records = {}
    try:
        for mode in (0, 2):
            pkg.set_option("path", 2)
            pkg.set_option("run_thresholds", mode)
            pkg.set_option("sample_stride", 8)                            # (like for like: the policy samples less with them on)
            ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
            keys = torch.empty(m, dtype=torch.int64, device=dev)
            out = torch.empty(m, dtype=torch.int32, device=dev)
            for _ in range(2):                                            # (twice: the running words are re-made per batch)
                pkg.keys_init(keys.data_ptr(), m)
                ix.query_keys(m, q_d.data_ptr(), keys.data_ptr())
                pkg.keys_to_indices(keys.data_ptr(), m, out.data_ptr())
                torch.cuda.synchronize()
                np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"{dist} {(k, m, n)} run_thresholds={mode}")
            st = ix.last_stats()
            ix.close()
            assert st[0] == 2 and st[2] == 0, st
            records[mode] = st[1]
    finally:
        pkg.set_option("path", 0)
        pkg.set_option("run_thresholds", 0)
        pkg.set_option("sample_stride", 0)
    assert records[0] <= records[2], records
    print("run_thresholds %s %s: %d candidates re-ranked with the running thresholds, %d without" % (dist, (k, m, n), records[0], records[2]))
    if dist in ("uniform", "gaussian") and m >= 4096:      # (few queries: every block sees a handful of tiles — nothing to tighten)
        assert records[0] < 0.8 * records[2], records      # the point of it: fewer candidates reach the exact re-rank
