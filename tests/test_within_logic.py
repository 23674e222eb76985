"""Radius-bounded top-K (knn_index_query_topk_within, include/knn_mi355x.h section 2c): the host arithmetic — the capped bound of
the cell-pruned scan through knn_debug_within_bound against rational arithmetic, the grid plan through knn_debug_grid_within_plan
—, the interface's mirror, and what the compiler made of the new kernels.  No GPU."""
import ctypes
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INF = float("inf")


# ---- the capped bound -----------------------------------------------------------------------------------------------------

def _v0(q, r):
    """v0's fp32 squared distance of one query to one row (tests/topk_oracle.py's arithmetic)."""
    d = np.float32(0)
    for a, b in zip(q, r):
        diff = np.float32(a) - np.float32(b)
        d = np.float32(d + np.float32(diff * diff))
    return d


def _exact_d2(q, r):
    return sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(q, r))


def _consts(k, sigma, amax, bmax, nmax):
    """knn_bound_consts (knn_filter_dev.h) restated: eta, eta^2, rho, gamma of a shard, in float64."""
    kt = (k + 15) // 16
    u = 2.0 ** -24
    theta = 2.0 ** -11 + 2.0 ** -23
    thp = theta / (1.0 - theta)
    nu0 = 2.0 ** -14 * 1.001
    kp = 16.0 * kt
    emax = thp * (amax + bmax) + 2.0 * nu0
    eta2 = k * emax * emax
    gam = (kp + 2.0) * u
    rho = (kt * 2.0 ** -18 + 2.0 * gam) * 2.0 * (nmax + kp * amax * amax) + kp * 2.0 ** -27 + 2.0 ** -21 * nmax + 2.0 ** -24
    return math.sqrt(eta2), eta2, rho, gam


@pytest.mark.parametrize("k", [1, 3, 8, 16, 20, 32])
@pytest.mark.parametrize("log2_sigma", [-6, 0, 9])
def test_capped_bound_holds_for_rows_at_and_one_ulp_either_side_of_the_radius(k, log2_sigma):
    """For a row whose v0 distance E is exactly max_dist2, one ulp under it and one ulp over it (the 1 + 1e-6 the stored Dup is
    taken larger by covers one ulp, 2^-23): its exact scaled distance D is at most the capped Dup, and its score — at most
    D + 2 eta sqrt(D) + eta^2 + rho - mq (1 - gamma), the filter's error bound — is below the threshold.  With a seed score far
    above the radius the cap is what binds (not vacuous: Dup stays within 1e-5 of sigma^2 max_dist2 (1 + g2)), and the gate of the
    re-rank lets the row's v0 value through."""
    rng = np.random.default_rng(1000 * k + log2_sigma + 77)
    sigma = np.float32(2.0 ** log2_sigma)
    s2 = Fraction(float(sigma)) ** 2
    g2 = (k + 3) * 1.0001 / 2 ** 24
    eta, eta2, rho, gam = _consts(k, float(sigma), 1.0, 1.0, float(k))
    for trial in range(10):
        q = ((rng.random(k) - 0.5) / float(sigma)).astype(np.float32)
        mq = float(np.sum((q.astype(np.float64) * float(sigma)) ** 2))
        r = (q.astype(np.float64) + rng.normal(size=k) * (0.3 * rng.random() / float(sigma)) / math.sqrt(k)).astype(np.float32)
        e = _v0(q, r)
        assert e > 0
        d = float(_exact_d2(q, r) * s2)
        u_far = 4.0 * k - mq   # a seed score of a row far beyond the radius: Dup(u) is far above dup_r
        for r2 in (e, np.nextafter(e, np.float32(INF)), np.nextafter(e, np.float32(0))):
            thr, dup, gate = pkg.debug_within_bound(k, float(sigma), 1.0, 1.0, float(k), u_far, mq, float(r2))
            assert math.isfinite(thr) and math.isfinite(dup)
            assert d <= dup, (k, trial, float(r2), d, dup)
            assert thr > d + 2.0 * eta * math.sqrt(d) + eta2 + rho - mq * (1.0 - gam), (k, trial, float(r2))
            assert gate >= e, (k, trial, float(r2), gate, float(e))
            cap = float(s2) * (float(r2) * (1.0 + g2) + k * 2.0 ** -125)
            assert cap <= dup <= cap * (1.0 + 1e-5), (dup, cap)
            # a seed score below the radius: knn_threshold's own bound binds, the cap changes nothing
            u_near = d * 0.25 - mq
            plain = pkg.debug_topk_gate(k, float(sigma), 1.0, 1.0, float(k), u_near, mq)
            both = pkg.debug_within_bound(k, float(sigma), 1.0, 1.0, float(k), u_near, mq, float(r2))
            assert both[1] == min(plain[1], dup) and both[0] <= plain[0] and both[0] <= thr


@pytest.mark.parametrize("k", [1, 8, 16, 32])
def test_no_seed_score_and_no_radius(k):
    """u = +INF (fewer than K finite seed scores): a finite radius gives a finite threshold — the cap alone —, the value a very
    large seed score gives.  max_dist2 = +INF: knn_debug_topk_gate's three values exactly, for finite and infinite u."""
    sigma, mq = 0.5, 0.37 * k / 16
    for r2 in (0.0, 1e-30, 0.01, 3.5, 1e6):
        thr, dup, gate = pkg.debug_within_bound(k, sigma, 1.0, 1.0, float(k), INF, mq, r2)
        assert math.isfinite(thr) and math.isfinite(dup) and math.isfinite(gate) and gate >= np.float32(r2), (r2, thr, dup, gate)
        assert (thr, dup, gate) == pkg.debug_within_bound(k, sigma, 1.0, 1.0, float(k), 1e30, mq, r2)
    assert pkg.debug_within_bound(k, sigma, 1.0, 1.0, float(k), 0.1, mq, 0.0)[2] < 1e-30   # radius 0: duplicates only
    for u in (-mq, 0.0, 0.3, 2.0 * k, INF):
        assert pkg.debug_within_bound(k, sigma, 1.0, 1.0, float(k), u, mq, INF) == \
            pkg.debug_topk_gate(k, sigma, 1.0, 1.0, float(k), u, mq), u
    out = (ctypes.c_double * 3)()
    f = pkg.lib().knn_debug_within_bound
    for bad in (-1.0, float("nan")):
        assert f(k, ctypes.c_float(sigma), 1.0, 1.0, float(k), 0.0, mq, ctypes.c_float(bad), out) != 0


# ---- the grid plan --------------------------------------------------------------------------------------------------------

BUDGET = 1 << 15   # cells of the largest walk a radius may ask for: the plain plan's largest (k 4, K 64: 13^4)


def test_grid_within_plan():
    base = dict(m=70, has_grid=1, path=0, flag=1)
    for k in (1, 2, 3, 4):
        for K in (1, 8, 17, 64):
            plain = pkg.debug_grid_topk_plan(k=k, K=K, **base)
            assert pkg.debug_grid_within_plan(k=k, K=K, radius_rings=0, **base) == plain          # no radius: the plain plan
            most = max(r for r in range(1, BUDGET) if (2 * r + 1) ** k <= BUDGET)                  # the budget's last ring count
            assert (2 * plain["rmax"] + 1) ** k <= BUDGET                                          # the plain plan is inside it
            for rings in (1, plain["rmax"], plain["rmax"] + 1, most, most + 1, 10 * most, 1 << 30):
                got = pkg.debug_grid_within_plan(k=k, K=K, radius_rings=rings, **base)
                want = dict(plain, rmax=rings if plain["rmax"] < rings <= most else plain["rmax"])
                assert got == want, (k, K, rings, got, want)
    assert pkg.debug_grid_within_plan(k=1, K=8, radius_rings=16383, **base)["rmax"] == 16383
    assert pkg.debug_grid_within_plan(k=4, K=1, radius_rings=6, **base)["rmax"] == 6
    assert pkg.debug_grid_within_plan(k=4, K=1, radius_rings=7, **base)["rmax"] == \
        pkg.debug_grid_topk_plan(k=4, K=1, **base)["rmax"]
    for off in (dict(has_grid=0), dict(flag=0), dict(path=1), dict(path=2)):                      # use = 0 zeroes the rest
        got = pkg.debug_grid_within_plan(**dict(base, k=3, K=8, radius_rings=9, **off))
        assert got == dict.fromkeys(pkg.GRID_TOPK_PLAN, 0), (off, got)
    with pytest.raises(pkg.KnnError, match="knn_debug_grid_within_plan"):
        pkg.debug_grid_within_plan(k=3, K=8, radius_rings=-1, **base)
    with pytest.raises(pkg.KnnError, match="knn_debug_grid_within_plan"):
        pkg.debug_grid_within_plan(k=5, K=8, radius_rings=1, **base)


# ---- the interface ---------------------------------------------------------------------------------------------------------

def test_header_prototypes_are_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = {
        "knn_index_query_topk_within":
            "int knn_index_query_topk_within(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2, "
            "unsigned long long *keys_dev, int *indices_dev, void *stream, unsigned flags);",
        "knn_index_query_topk_within_host":
            "int knn_index_query_topk_within_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2, "
            "int *indices_host, float *dist2_host, int *counts_host );",
    }
    flat = re.sub(r"\s+", " ", header)
    L = pkg.lib()
    for name, proto in protos.items():
        assert re.sub(r"\s+", " ", proto) in flat, name
        assert name in pkg.EXPORTED_SYMBOLS
        assert len(getattr(L, name).argtypes) == proto.count(",") + 1, name
    for name in ("knn_debug_grid_within_plan", "knn_debug_within_bound"):
        assert name in pkg.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.knn_index_query_topk_within.argtypes[5] is ctypes.c_float and L.knn_index_query_topk_within_host.argtypes[4] is ctypes.c_float
    # no index: an error before anything else, whatever the radius
    for r2 in (1.0, -1.0, float("nan"), INF):
        assert L.knn_index_query_topk_within(None, 0, 1, 1, None, r2, None, None, None, 1) != 0
        assert L.knn_index_query_topk_within_host(None, 1, 1, None, r2, None, None, None) != 0
    assert callable(pkg.KnnIndex.query_topk_within) and callable(pkg.KnnIndex.query_topk_within_host)


# ---- what the compiler made of the new kernels ---------------------------------------------------------------------------

def _metadata(tmp_path, names):
    procs = []
    for name in names:
        src = os.path.join(ROOT, "multicore_hw2_amd", "csrc", name + ".hip")
        procs.append(subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                                       "--cuda-device-only", "-o", str(tmp_path / (name + ".s")), src]))
    meta = {}
    for name, p in zip(names, procs):
        assert p.wait() == 0, name
        text = (tmp_path / (name + ".s")).read_text()
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
            meta[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1)),
                                int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)))
    return meta


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_new_kernels_use_no_scratch_and_the_prep_forms_stay_within_their_twins_registers(tmp_path):
    """The radius forms of the top-K prep kernel (one per PW, KT of the one-frame top-K forms): zero scratch and at most the VGPRs
    of the plain top-K form of the same shape.  The radius forms of the grid and of the exact top-K kernel and the clip kernel:
    zero scratch."""
    meta = _metadata(tmp_path, ("knn_cells", "knn_grid", "knn_exact"))

    def one(pattern):
        names = [n for n in meta if re.search(pattern, n)]
        assert len(names) == 1, (pattern, names)
        return names[0]

    preps = [n for n in meta if "knn_cells_prep_within_kernel" in n]
    assert len(preps) == 4, preps
    for name in preps:
        pw, sd, kt = re.search(r"within_kernelILi(\d)ELi(\d)ELi(\d)E", name).groups()
        twin = one(r"knn_cells_prep_kernelILi%sELi%sELi%sELb0ELb1E" % (pw, sd, kt))
        assert meta[name][1] == 0, (name, meta[name])
        assert meta[name][0] <= meta[twin][0], (name, meta[name], meta[twin])
    grids = [n for n in meta if "knn_grid_within_kernel" in n]
    exacts = [n for n in meta if re.search(r"knn_exact_topk_kernelILi\dELb1E", n)]
    assert len(grids) == 4 and len(exacts) == 9, (grids, exacts)
    for name in grids + exacts + [one("knn_topk_clip_kernel")]:
        assert meta[name][1] == 0, (name, meta[name])
