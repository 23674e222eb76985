"""Top-K on the cell-pruned scan, the parts that need no GPU: the K-th smallest seed score the preparation kernel
hands to the threshold (its host restatement, knn_debug_seed_kth), the plan of a pruned top-K call (knn_debug_cells_topk_plan)
against the rules restated here, the option, and what the compiler made of the new kernels.

What the host hooks share with the device code, and what they restate: knn_debug_seed_kth runs the kernel's key map and
compare-exchange (knn_seed_key, knn_seed_cx, knn_seed_lane_holds_row) over 64 array elements; the lane select, the waves' and the
block's merges are the same network written over arrays, and the rule that a wide-sample tile inside a seed cell is left out is the
caller's here (it is exercised on the GPU only: tests/test_cells_topk_gpu.py's empty-corner case).  knn_debug_topk_gate shares
knn_threshold and knn_topk_gate with the kernels and repeats the prep kernel's three lines that store Dup (times 1 + 1e-6, rounded
up to fp32): a change to those lines has to be made in both places."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 8, 17, 64)


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import multicore_hw2_amd as p
    if not os.path.exists(p.lib_path):
        import __graft_entry__ as g
        g.build()
    return p


# ---- the K-th seed rule ------------------------------------------------------------------------------------------------------

def _kth_brute(scores, K):
    """K-th smallest FINITE score (+-inf and NaN are not real rows), +inf when there are fewer."""
    s = np.asarray(scores, dtype=np.float32)
    s = np.sort(s[np.isfinite(s)])
    return np.float32(np.inf) if s.size < K else s[K - 1]


@pytest.mark.parametrize("pw", [2, 4])
@pytest.mark.parametrize("K", KS)
def test_kth_seed_score_is_the_kth_smallest_real_score(pkg, K, pw):
    rng = np.random.default_rng(1000 * K + pw)
    for trial in range(40):
        n = int(rng.integers(1, 1300))
        s = (rng.normal(size=n) * 10.0 ** int(rng.integers(-3, 4))).astype(np.float32)
        if trial % 3 == 0:
            s = np.round(s * 4) / 4                       # ties across tiles and waves
        s[rng.random(n) < rng.choice([0.0, 0.3, 0.97])] = np.inf   # padding / out-of-box positions: +INF norm
        if trial % 5 == 0:
            s[rng.integers(0, n)] = np.nan
            s[rng.integers(0, n)] = -np.inf
        got = np.float32(pkg.debug_seed_kth(s, [], K, pw))
        want = _kth_brute(s, K)
        # never below the K-th smallest real score of the scored positions (the rule's validity), and exactly it (its tightness)
        assert got >= want and got == want, (trial, n, K, got, want)
        if K == 1 and np.isfinite(s).any():
            assert got == s[np.isfinite(s)].min()          # the 1-NN minimum


@pytest.mark.parametrize("K", KS)
def test_wide_sample_is_merged_in_only_when_the_seed_cells_hold_fewer_than_k(pkg, K):
    rng = np.random.default_rng(7 + K)
    for trial in range(30):
        nfin = int(rng.integers(0, 2 * K + 2))             # finite seed scores
        seed = np.full(int(rng.integers(max(nfin, 1), 400)), np.inf, dtype=np.float32)
        seed[rng.permutation(seed.size)[:nfin]] = rng.random(nfin, dtype=np.float32) + 5.0
        wfin = int(rng.integers(0, 2 * K + 2))
        wide = np.full(2048, np.inf, dtype=np.float32)
        wide[rng.permutation(2048)[:wfin]] = rng.random(wfin, dtype=np.float32)   # all BELOW the seed scores
        got = np.float32(pkg.debug_seed_kth(seed, wide, K, 4))
        if nfin >= K:      # enough real rows in the seed cells: the wide sample is not looked at
            assert got == _kth_brute(seed, K), (trial, nfin, wfin)
        else:              # merged: the K-th smallest of both; +INF exactly when fewer than K are finite in all
            assert got == _kth_brute(np.concatenate([seed, wide]), K), (trial, nfin, wfin)
            assert np.isinf(got) == (nfin + wfin < K)
    assert np.isinf(pkg.debug_seed_kth([], [], K, 4))
    for bad in (0, 65):
        with pytest.raises(pkg.KnnError):
            pkg.debug_seed_kth([1.0], [], bad, 4)


# ---- the plan ---------------------------------------------------------------------------------------------------------------

def _size_rule(k):
    return 1 << 19 if k <= 12 else 1 << 20 if k <= 16 else 1 << 22 if k <= 21 else 1 << 23 if k <= 23 else 1 << 24 if k <= 25 else 1 << 62


# the seven instantiations of knn_cells_records_kernel<DYN, KT, NIF, U8>
COMPILED = {(0, 1, 0, 0), (1, 1, 0, 0), (0, 2, 1, 0), (1, 2, 1, 0), (0, 2, 0, 0), (1, 2, 0, 0), (1, 1, 0, 1)}
# layouts as the build options make them: (cells_rows, cells_u8_frame / cells_centre) -> (centred, rows_u8, bins)
LAYOUTS = {"fp16": (0, 0, 0), "fp16_centred": (1, 0, 0), "u8_per_cell": (1, 1, 0), "u8_bins": (0, 1, 1)}


def test_plan_reaches_exactly_the_compiled_forms_and_policy_declines(pkg):
    """Option 1 reaches exactly the seven compiled record-only forms, never SELF or CTR; option 0 (policy) declines every shard —
    below the size rule for good, at or above it until the A/B measurements the policy is to rest on are taken;
    option 2 never.  (That no 1-NN tail or gather is launched is not a plan field: knn_cells_query_topk's sequence has neither.)"""
    seen = set()
    for k in range(1, 33):
        for n in ((1 << 17) + 999, 1 << 19, (1 << 20) - 1, 1 << 20, 1 << 22, 1 << 24):
            ncells = min(65536, 1 << max(9, (n // 256).bit_length() - 1))
            for lname, (centred, rows_u8, bins) in LAYOUTS.items():
                if rows_u8 and k > 16:
                    continue
                for K in KS:
                    for opt in (0, 1, 2):
                        for m, deal, several in ((96, 0, 0), (1024, 1, 0), (1357, 2, 1), (4, 0, 0)):
                            p = pkg.debug_cells_topk_plan(k=k, K=K, m=m, n=n, topk_cells=opt, has_cells=1, centred=centred,
                                                          rows_u8=rows_u8, bins=bins, sharded=0, n_outliers=0, ncells=ncells,
                                                          nitems=ncells + 7, cap=384 if k <= 20 else 640, several_slots=several,
                                                          scan_blocks=0, scan_deal=deal, num_cu=256, rec_cap=1 << 22, cells=0)
                            served = lname in ("fp16", "u8_bins") and m >= 5
                            want = served and opt == 1
                            if opt == 0:
                                assert p["use"] == 0, (k, n, lname, K)        # below AND above _size_rule(k), for now
                            assert p["use"] == int(want), (k, n, lname, K, opt, m, p)
                            if not want:
                                continue
                            form = (p["scan_dyn"], p["scan_kt"], p["scan_nif"], p["scan_u8"])
                            assert form in COMPILED, (k, lname, form)
                            seen.add(form)
                            kt = 1 if k <= 16 else 2
                            assert p["scan_kt"] == kt and p["prep_kt"] == kt and p["scan_u8"] == rows_u8
                            assert p["scan_nif"] == int(16 < k <= 30)
                            assert p["scan_self"] == 0 and p["scan_ctr"] == 0 and p["prep_ctr"] == 0      # never SELF, never CTR
                            assert p["match_waves"] in (8, 16) and p["prep_pw"] in (2, 4)
                            assert p["passes"] == -(-m // 1024) and p["pass_m"] == min(m, 1024)
                            assert p["ccap"] == min(4096 + 128 * K, (32 << 20) // m)
                            # the rooms: the waves' slices and the shared overflow area inside the record buffer
                            assert p["nlists"] == p["blocks"] * p["waves"] and p["nlists"] * p["slice"] <= p["ovf_base"]
                            assert p["ovf_base"] + p["ovf_cap"] == 1 << 22
                            assert p["waves"] == (12 if kt == 1 else 16)
                            if deal:
                                assert p["scan_dyn"] == (1 if rows_u8 else deal - 1)
    assert seen == COMPILED, COMPILED - seen


def test_plan_declines_what_the_path_does_not_serve(pkg):
    base = dict(k=16, K=8, m=256, n=1 << 24, topk_cells=1, has_cells=1, centred=0, rows_u8=0, bins=0, sharded=0, n_outliers=0,
                ncells=65536, nitems=65536, cap=384, several_slots=0, scan_blocks=0, scan_deal=0, num_cu=256, rec_cap=1 << 22, cells=0)
    assert pkg.debug_cells_topk_plan(**base)["use"] == 1
    for change in (dict(has_cells=0), dict(sharded=1), dict(centred=1), dict(rows_u8=1, bins=0), dict(m=4), dict(topk_cells=2),
                   dict(n_outliers=(4096 + 128 * 8) // 2 + 1), dict(k=33), dict(K=65)):
        assert pkg.debug_cells_topk_plan(**dict(base, **change))["use"] == 0, change
    # policy declines (for now: everywhere); `topk_cells` = 1 serves the layout whatever `cells` says
    assert pkg.debug_cells_topk_plan(**dict(base, topk_cells=0))["use"] == 0
    assert pkg.debug_cells_topk_plan(**dict(base, topk_cells=0, cells=2))["use"] == 0
    assert pkg.debug_cells_topk_plan(**dict(base, topk_cells=1, cells=2))["use"] == 1


def test_topk_cells_option_round_trips(pkg):
    for v in (1, 2, 0):
        pkg.set_option("topk_cells", v)
        assert pkg.get_option("topk_cells") == v
    with pytest.raises(pkg.KnnError):
        pkg.set_option("topk_cells", 3)
    assert pkg.get_option("topk_cells") == 0


# ---- what the compiler made of the new kernels ---------------------------------------------------------------------------

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_topk_kernels_use_no_scratch_stay_within_their_twins_registers_and_fold_no_keys(tmp_path):
    """Every record-only scan and every top-K prep instantiation: zero scratch and at most the VGPRs of its 1-NN twin (the scan:
    the run-time-k form of the same shape; the prep kernel: the same PW, KT); the record-only scans hold no 64-bit global
    atomic-min (the 1-NN scans do: the pattern is checked on them)."""
    src = os.path.join(ROOT, "multicore_hw2_amd", "csrc", "knn_cells.hip")
    asm = tmp_path / "knn_cells.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                           "-o", str(asm), src])
    text = asm.read_text()
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        meta[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1)),
                            int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)))
    bodies = dict(re.findall(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M))
    atomic_min64 = re.compile(r"\b(global|flat)_atomic_[us]?min_x2\b")

    def one(pattern):
        names = [n for n in meta if re.search(pattern, n)]
        assert len(names) == 1, (pattern, names)
        return names[0]

    records = [n for n in meta if "knn_cells_records_kernel" in n]
    assert len(records) == 7, records
    for name in records:
        dyn, kt, nif, u8 = re.search(r"records_kernelILb([01])ELi(\d)ELb([01])ELb([01])E", name).groups()
        twin = one(r"knn_cells_scan_kernelILb%sELi0ELb0ELi%sELb0ELb%sELb%sE" % (dyn, kt, nif, u8))
        assert meta[name][1] == 0, (name, meta[name])
        assert meta[name][0] <= meta[twin][0], (name, meta[name], meta[twin])
        assert meta[name][0] <= (80 if kt == "1" else 128)
        assert not atomic_min64.search(bodies[name]), name
        assert atomic_min64.search(bodies[twin]), twin
        assert "v_mfma" in bodies[name]
    preps = [n for n in meta if re.search(r"knn_cells_prep_kernelILi\dELi\dELi\dELb0ELb1E", n)]
    assert len(preps) == 4, preps
    for name in preps:
        pw, sd, kt = re.search(r"prep_kernelILi(\d)ELi(\d)ELi(\d)E", name).groups()
        twin = one(r"knn_cells_prep_kernelILi%sELi%sELi%sELb0ELb0E" % (pw, sd, kt))
        assert meta[name][1] == 0, (name, meta[name])
        assert meta[name][0] <= meta[twin][0], (name, meta[name], meta[twin])


# ---- the distance gate of the re-rank ------------------------------------------------------------------------------------

def _v0(q, R):
    """v0's fp32 squared distances of one query to rows R (tests/topk_oracle.py's arithmetic)."""
    d = np.zeros(R.shape[0], dtype=np.float32)
    for j in range(R.shape[1]):
        diff = q[j] - R[:, j]
        d = d + diff * diff
    return d


def _exact_d2(q, r):
    from fractions import Fraction
    return sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(q, r))


@pytest.mark.parametrize("k", [1, 3, 8, 16, 20, 32])
@pytest.mark.parametrize("log2_sigma", [-6, 0, 9])
def test_distance_gate_never_discards_a_row_v0_ranks_within_k(pkg, k, log2_sigma):
    """knn_topk_gate against exact rational arithmetic.  Dup = D0up (1+g2)^2 + sigma^2 tau bounds the K seed rows' real scaled
    distances by D0up; the gate must let through the v0 value of EVERY row whose real distance is <= D0up — rows exactly at the
    bound, one ulp under and one ulp over it in single coordinates included — because the K-th smallest v0 value of the shard is at
    most the largest v0 value among those K rows.  Rows v0 ranks within K of a pool that holds K such rows pass with them."""
    from fractions import Fraction
    rng = np.random.default_rng(100 * k + log2_sigma + 50)
    sigma = np.float32(2.0 ** log2_sigma)
    s2 = Fraction(float(sigma)) ** 2
    g2 = Fraction((k + 3) * 1.0001) / 2 ** 24
    tau = Fraction(k, 2 ** 125)
    for trial in range(12):
        q = ((rng.random(k) - 0.5) / float(sigma)).astype(np.float32)
        mq = float(np.sum((q.astype(np.float64) * float(sigma)) ** 2))
        u = float(rng.random() * 0.5 * k / 16 - mq)                 # a seed score: scaled squared distance minus the query's norm
        thr, dupf, gate = pkg.debug_topk_gate(k, float(sigma), 1.0, 1.0, float(k), u, mq)
        assert np.isfinite(dupf) and gate >= dupf / float(s2)
        assert gate <= dupf / float(s2) * (1 + 2.0 ** -19) + 2.0 ** -119      # not vacuous
        d0up = (Fraction(dupf) - s2 * tau) / (1 + g2) ** 2               # real scaled squared distance the seed rows stay within
        radius = (float(d0up) / float(s2)) ** 0.5                         # in the rows' own units
        rows = []
        for _ in range(60):                                                # rows at the bound: a random direction, scaled to it
            v = rng.normal(size=k)
            v *= radius / np.linalg.norm(v)
            r = (q.astype(np.float64) - v).astype(np.float32)
            rows.append(r)
            for _ in range(3):                                             # ... and single coordinates one ulp up and down
                r2 = r.copy()
                j = int(rng.integers(0, k))
                r2[j] = np.nextafter(r2[j], np.float32(rng.choice([-np.inf, np.inf])))
                rows.append(r2)
        R = np.stack(rows)
        inside = np.array([_exact_d2(q, r) * s2 <= d0up for r in R])
        assert inside.any() and (~inside).any(), (k, trial)                # the pool straddles the bound
        e = _v0(q, R)
        assert (e[inside] <= np.float32(gate)).all(), (k, trial, float(e[inside].max()), gate)
        K = min(8, int(inside.sum()))                                      # K seed rows inside the bound; v0's ranking of the pool
        kth = np.sort(e[inside])[K - 1]                                    # >= the pool's K-th smallest v0 value
        assert (e[e <= kth] <= np.float32(gate)).all()
    _, dup_bad, gate_bad = pkg.debug_topk_gate(k, float(sigma), 1.0, 1.0, float(k), float("inf"), 0.0)
    assert not (gate_bad < np.inf)                                         # a query nothing bounds: the pass falls back anyway
