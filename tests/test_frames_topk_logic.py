"""Top-K on the cell-pruned scan for layouts in per-cell frames (KNN_QUERY_TOPK_FRAMES; DESIGN §4.6 "Per-cell frames"), the parts
that need no GPU: the plan and the route with the hooks' third `centred` value (2 = per-cell frames and the call carries the flag),
the conversion of a seed score into a frame-free bound (knn_debug_frame_dup runs the kernel's own lines, knn_frame_dup.h) with
the selection over the converted values (knn_debug_seed_kth), the flag's hygiene, and what the compiler made of the new kernels."""
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

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


# ---- the plan and the route ---------------------------------------------------------------------------------------------------

# layouts as the build options make them -> (centred, rows_u8, bins), and the values of the hooks' `centred` input that describe
# them: 0 the shard's frame, 1 per-cell frames, 2 per-cell frames and the call carries the flag.  (For fp16 rows the hook's 2 IS
# the centred layout, so "fp16" has no third value; 8-bit rows in bin frames are never centred, so 2 there is the flag alone.)
LAYOUTS = {"fp16": ((0, 0, 0), (0,)), "fp16_centred": ((1, 0, 0), (1, 2)), "u8_per_cell": ((1, 1, 0), (1, 2)),
           "u8_bins": ((0, 1, 1), (0, 2))}
# knn_cells_frame_records_kernel<DYN, U8>
COMPILED = {(0, 0), (1, 0), (1, 1)}


def _ccap(K, m):
    return min(4096 + 128 * K, (32 << 20) // m)


def test_plan_takes_per_cell_frames_exactly_with_the_flag_and_the_option(pkg):
    seen = set()
    for k in range(1, 17):
        for n in ((1 << 17) + 999, 1 << 20, 1 << 24):
            ncells = min(65536, 1 << max(9, (n // 256).bit_length() - 1))
            for lname, ((_, rows_u8, bins), values) in LAYOUTS.items():
                for centred in values:
                    for K in KS:
                        for opt in (0, 1, 2):
                            for m, deal, several in ((96, 0, 0), (1024, 1, 0), (1357, 2, 1), (4, 0, 0), (600000, 0, 0)):
                                for sharded in (0, 1, 2):
                                    for n_outliers in (0, _ccap(K, m) // 2 + 1):
                                        args = dict(k=k, K=K, m=m, n=n, topk_cells=opt, has_cells=1, centred=centred, rows_u8=rows_u8,
                                                    bins=bins, sharded=sharded, n_outliers=n_outliers, ncells=ncells, nitems=ncells + 7,
                                                    cap=384, several_slots=several, scan_blocks=0, scan_deal=deal, num_cu=256,
                                                    rec_cap=1 << 22, cells=0)
                                        p = pkg.debug_cells_topk_plan(**args)
                                        call = m >= 5 and _ccap(K, m) >= 64 and n_outliers <= _ccap(K, m) // 2
                                        frames = (centred == 2 and opt == 1 and lname in ("fp16_centred", "u8_per_cell") and
                                                  sharded == 0 and call)
                                        # the parent's rule for a layout in the shard's frame (a cell-range shard is fp16: with its flag)
                                        one_frame = (lname in ("fp16", "u8_bins") and opt == 1 and call and
                                                     (sharded == 0 or (sharded == 2 and lname == "fp16")))
                                        if lname == "u8_bins" and sharded:
                                            continue      # (not a layout a cell-range shard has)
                                        assert p["use"] == int(frames or one_frame), (lname, args, p)
                                        if lname == "u8_bins":      # the flag on a layout in the shard's frame changes nothing
                                            assert p == pkg.debug_cells_topk_plan(**dict(args, centred=0)), (args, p)
                                        if centred == 1:            # per-cell frames without the flag: never, as before
                                            assert p["use"] == 0
                                        # the route's way is 4 exactly when the plan says use and `path` is 0 or 2
                                        if m == 96 and n_outliers == 0 and K in (1, 64):
                                            for path in range(4):
                                                r = pkg.debug_query_route(**dict(args, path=path, filter_usable=1, has_grid=0,
                                                                                 filter_wanted=0, init_keys=1))
                                                assert (r["way"] == 4) == bool(p["use"] and path in (0, 2)), (args, path, r)
                                                assert r["topk_use"] == int(r["way"] == 4)
                                        if not frames:
                                            continue
                                        assert p["prep_ctr"] == 1 and p["scan_ctr"] == 1 and p["scan_kt"] == 1 and p["prep_kt"] == 1
                                        assert p["scan_self"] == 0 and p["scan_nif"] == 0 and p["scan_u8"] == rows_u8
                                        assert p["waves"] == 16 and p["blocks"] <= 256          # one block of 16 waves per CU
                                        assert p["nlists"] == p["blocks"] * 16 and p["nlists"] * p["slice"] <= p["ovf_base"]
                                        assert p["ovf_base"] + p["ovf_cap"] == 1 << 22
                                        m_padded = (min(m, 1024) + 31) // 32 * 32
                                        # the fp32 query rows, sqrt(Dup) and Dup per query, one norm window per wave
                                        assert p["lds_bytes"] == m_padded * (64 + 4 + 4) + 16 * 9 * 8 * 16
                                        assert p["scan_lds_limit"] == 1024 * 72 + 16 * 9 * 8 * 16
                                        assert p["match_waves"] in (8, 16) and p["prep_pw"] in (2, 4)
                                        assert p["passes"] == -(-m // 1024) and p["pass_m"] == min(m, 1024)
                                        assert p["ccap"] == _ccap(K, m)
                                        form = (p["scan_dyn"], p["scan_u8"])
                                        assert form in COMPILED, (lname, form)
                                        if deal:
                                            assert p["scan_dyn"] == (1 if rows_u8 else deal - 1)
                                        seen.add(form)
    assert seen == COMPILED, COMPILED - seen
    # k > 16 has no per-cell frames; the flag changes nothing there
    base = dict(k=20, K=8, m=96, n=1 << 24, topk_cells=1, has_cells=1, centred=2, rows_u8=0, bins=0, sharded=0, n_outliers=0,
                ncells=65536, nitems=65536, cap=640, several_slots=0, scan_blocks=0, scan_deal=0, num_cu=256, rec_cap=1 << 22, cells=0)
    assert pkg.debug_cells_topk_plan(**base)["use"] == 0


# ---- the conversion and the selection -----------------------------------------------------------------------------------------

FRAME_AMAX = 16384.0
F32 = np.float32


def _frame(rng, k, log2_sigma=None, log2_ratio=None):
    """A cell's frame: centre [16], scale = sigma x ratio, ratio (a power of two, 1 .. 2^8), bmax, nmax (filled by the caller)."""
    sigma = 2.0 ** (int(rng.integers(-3, 4)) if log2_sigma is None else log2_sigma)
    ratio = 2.0 ** (int(rng.integers(0, 9)) if log2_ratio is None else log2_ratio)
    fr = np.zeros(20, dtype=F32)
    fr[:k] = (rng.random(k) - 0.5).astype(F32) / F32(sigma)
    fr[16], fr[17], fr[18], fr[19] = sigma * ratio, ratio, 1.0, float(k)
    return fr


def _in_frame(k, fr, x):
    """(fp16 coordinates as float64 [16], the computed norm as the layout makes it) of a row or query x in the frame: fp32
    subtract, exact power-of-two scale, fp16 to nearest even; exact products, fp32 sums (two halves of eight, then their sum)."""
    sc = np.zeros(16, dtype=F32)
    sc[:k] = (np.asarray(x, dtype=F32)[:k] - fr[:k]) * fr[16]
    with np.errstate(over="ignore"):
        h = sc.astype(np.float16).astype(F32)
    part = [F32(0), F32(0)]
    for d in range(16):
        part[d >> 3] = F32(part[d >> 3] + h[d] * h[d])
    return h.astype(np.float64), F32(part[0] + part[1])


def _mirror(k, fr, q, u):
    """knn_frame_query + knn_frame_dup restated with numpy scalars (same operations in the same order; doubles are IEEE both
    sides): (Dup, far)."""
    sc = np.zeros(16, dtype=F32)
    sc[:k] = (np.asarray(q, dtype=F32)[:k] - fr[:k]) * fr[16]
    n32 = F32(0)
    nrm = F32(0)
    amax = F32(0)
    bad = False
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(16):
            n32 = F32(n32 + sc[d] * sc[d])
            back = F32(np.float16(sc[d]))
            bad = bad or not abs(back) < np.inf
            amax = max(amax, abs(back))
            nrm = F32(nrm + back * back)
            bad = bad or not abs(F32(np.float16(back * F32(-2.0)))) < np.inf
    far = bool(bad or not amax <= FRAME_AMAX)
    if not abs(u) < np.inf:
        return np.inf, far
    uu = 2.0 ** -24
    theta = 2.0 ** -11 + 2.0 ** -23
    thp = theta / (1.0 - theta)
    nu0 = 2.0 ** -14 * 1.001
    a, bmax, nmaxc, scale, ratio = (0.0 if far else float(amax)), float(fr[18]), float(fr[19]), float(fr[16]), float(fr[17])
    emax = thp * (a + bmax) + 2.0 * nu0
    eta2 = k * emax * emax
    eta = np.sqrt(eta2)
    omega = 1 * 2.0 ** -18
    gam = (16.0 + 2.0) * uu
    mmax = 16.0 * a * a
    rho = (omega + 2.0 * gam) * 2.0 * (nmaxc + mmax) + 16.0 * 2.0 ** -27
    rho += 2.0 ** -21 * nmaxc + 2.0 ** -24
    g2 = (k + 3.0) * uu * 1.0001
    tau = k * 2.0 ** -125
    sigma2 = scale * scale
    with np.errstate(over="ignore"):
        if far:
            reach = np.sqrt(np.float64(n32)) * (1.0 + 1e-6) + np.sqrt(np.float64(k)) * bmax * 1.001 + 0.001
            dup = reach * reach * (1.0 + 1e-5) * (1.0 + g2) * (1.0 + g2) + sigma2 * tau
            if not dup < 1e300:
                return np.inf, far
        else:
            mq = float(nrm)
            dt = float(u) + mq * (1.0 + 1.01 * gam) + rho
            dt = max(dt, 0.0)
            sq0 = eta + np.sqrt(dt + 2.0 * eta2)
            dup = sq0 * sq0 * (1.0 + g2) * (1.0 + g2) + sigma2 * tau
            thr = dup + 2.0 * eta * np.sqrt(dup) + eta2 + rho - mq * (1.0 - gam)
            thr += abs(thr) * 1e-6 + 1e-30
            if not thr < float(np.finfo(F32).max):      # (the kernel: the fp32 threshold is not finite)
                return np.inf, far
        dup = dup / (ratio * ratio) * (1.0 + 1e-6)
        df = F32(dup)
        if float(df) < dup:
            df = np.nextafter(df, F32(np.inf))
    return float(df), far


@pytest.mark.parametrize("k", [1, 5, 8, 16])
def test_frame_dup_is_non_decreasing_in_the_score_and_equals_its_restatement(pkg, k):
    rng = np.random.default_rng(500 + k)
    for trial in range(40):
        fr = _frame(rng, k)
        fr[18], fr[19] = rng.random() + 0.01, k * rng.random() + 0.01
        far = trial % 4 == 3
        q = fr[:16].copy()
        if far:      # beyond CELL_FRAME_AMAX cell units in every coordinate (some beyond the fp16 range)
            q[:k] += (np.sign(rng.random(k) - 0.5) * FRAME_AMAX * (1.5 + 6.0 * rng.random(k)) / fr[16]).astype(F32)
        else:
            q[:k] += ((rng.random(k) - 0.5) * (2.0 * FRAME_AMAX * 0.9) / fr[16]).astype(F32)
        _, mq = _in_frame(k, fr, q)
        mq = mq if np.isfinite(mq) else F32(0)      # (a far query's scores are the rows' norms)
        us = np.sort(np.concatenate([(rng.random(60) * 4.0 * k - float(mq)), [-float(mq), -float(mq) - 1.0, 1e30, 3e38]])).astype(F32)
        dups = [pkg.debug_frame_dup(k, fr, q, u) for u in us]
        assert all(d[1] == far for d in dups), (trial, dups[0])
        vals = np.array([d[0] for d in dups])
        assert (np.diff(vals) >= 0).all(), (trial, us, vals)                    # (a) non-decreasing
        assert vals[0] >= 0.0
        for u, d in zip(us[::7], dups[::7]):
            assert d == _mirror(k, fr, q, u), (trial, u, d, _mirror(k, fr, q, u))
        assert np.isinf(pkg.debug_frame_dup(k, fr, q, np.inf)[0]) and np.isinf(pkg.debug_frame_dup(k, fr, q, np.nan)[0])
    with pytest.raises(pkg.KnnError):
        pkg.debug_frame_dup(17, _frame(rng, 16), np.zeros(17, dtype=F32), 0.0)


@pytest.mark.parametrize("pw", [2, 4])
@pytest.mark.parametrize("K", [1, 2, 17, 64])
def test_block_value_is_the_kth_smallest_of_all_per_position_conversions(pkg, K, pw):
    """(b) The kernel keeps each seed cell's smallest scores (a sorted list of up to 64), converts the list entries, and merges
    the cells' lists as keys: the block's value must equal the K-th smallest of the conversions of ALL finite positions, brute
    force — which is what the monotonicity buys.  Fewer than K: the wide sample (tiles in their own frames) merged in, or +INF."""
    rng = np.random.default_rng(900 + 10 * K + pw)
    k = 8
    for trial in range(12):
        q = (rng.random(k) - 0.5).astype(F32)

        def cells(ncells, nmax_rows, p_hole):
            out_kernel, out_all = [], []
            for _ in range(ncells):
                fr = _frame(rng, k, log2_sigma=0)
                fr[:k] = q + ((rng.random(k) - 0.5) * (60000.0 if rng.random() < 0.25 else 2.0) / fr[16]).astype(F32)   # some far
                _, mq = _in_frame(k, fr, q)
                n = int(rng.integers(1, nmax_rows))
                s = (rng.random(n) * 2.0 * k - float(mq)).astype(F32)
                s[rng.random(n) < p_hole] = np.inf                    # padding and out-of-box positions
                fin = np.sort(s[np.isfinite(s)])
                conv = lambda u: pkg.debug_frame_dup(k, fr, q, u)[0]
                out_kernel += [conv(u) for u in fin[:64]]            # the cell's list: its 64 smallest, converted
                out_all += [conv(u) for u in fin]
            return np.array(out_kernel, dtype=F32), np.array(out_all, dtype=F32)

        p_hole = [0.0, 0.5, 0.98][trial % 3]
        seed_k, seed_all = cells(4, 300, p_hole)
        wide_k, wide_all = cells(int(rng.integers(0, 20)), 32, p_hole)
        got = F32(pkg.debug_seed_kth(seed_k, wide_k, K, pw))

        def kth(v):
            v = np.sort(v[np.isfinite(v)])
            return F32(np.inf) if v.size < K else v[K - 1]

        if np.isfinite(seed_all).sum() >= K:
            assert got == kth(seed_all), (trial, got, kth(seed_all))
        else:
            both = np.concatenate([seed_all, wide_all])
            assert got == kth(both), (trial, got, kth(both))
            assert np.isinf(got) == (np.isfinite(both).sum() < K)


def _exact_d2(q, r, k):
    return sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(q[:k], r[:k]))


@pytest.mark.parametrize("k", [1, 5, 8, 16])
def test_frame_dup_bounds_the_rows_exact_distance(pkg, k):
    """(c) Soundness against exact rational arithmetic.  A row of a cell and a query, both rounded to fp16 in the cell's frame as the
    layout and the kernel round them; the row's score from those operands (its computed norm plus the exact dot product with the
    B operand — what the matrix core accumulates, up to the rho the bound allows for); the returned Dup, in the shard's units,
    is >= sigma^2 x the row's exact squared distance to the query.  Rows at the frame's edge, a query at CELL_FRAME_AMAX, and a
    far query (every row of the cell within `reach`)."""
    rng = np.random.default_rng(700 + k)
    checked_far = checked_edge = 0
    for trial in range(60):
        fr = _frame(rng, k)
        scale, ratio = float(fr[16]), float(fr[17])
        sigma2 = Fraction(scale / ratio) ** 2
        kind = trial % 3
        j = int(rng.integers(0, k))
        if kind == 1:
            fr[j] = F32(0)            # so that (q - centre) x scale below is exactly CELL_FRAME_AMAX (powers of two)
        rows = fr[None, :16] + np.pad(((rng.random((24, k)) * 2.0 - 1.0) / scale).astype(F32), ((0, 0), (0, 16 - k)))
        rows[:4, :k] = fr[:k] + (np.sign(rng.random((4, k)) - 0.5) / scale).astype(F32)       # the frame's edge: |coordinate| = 1
        rows = rows.astype(F32)
        hr = [_in_frame(k, fr, r) for r in rows]
        fr[18] = max(np.abs(h).max() for h, _ in hr)
        fr[19] = max(float(nr) for _, nr in hr)
        q = fr[:16].copy()
        if kind == 0:        # a query among the rows
            q[:k] += ((rng.random(k) * 2.0 - 1.0) * 1.5 / scale).astype(F32)
        elif kind == 1:      # a query at CELL_FRAME_AMAX in one coordinate
            q[:k] += ((rng.random(k) * 2.0 - 1.0) * 100.0 / scale).astype(F32)
            q[j] = F32(FRAME_AMAX / scale)
        else:                # a far query: beyond CELL_FRAME_AMAX cell units
            q[:k] += (np.sign(rng.random(k) - 0.5) * (FRAME_AMAX * (1.5 + rng.random(k) * 100.0)) / scale).astype(F32)
        hq, _ = _in_frame(k, fr, q)
        far_expected = not np.abs(hq).max() <= FRAME_AMAX
        for r, (h, nr) in zip(rows, hr):
            if not np.abs(h).max() < np.inf:
                continue
            u = float(nr) if far_expected else float(nr) + float(np.dot(h, -2.0 * hq))    # (far: a zero B operand leaves the norm)
            dup, far = pkg.debug_frame_dup(k, fr, q, F32(u))
            assert far == far_expected and (kind != 1 or (not far and np.abs(hq).max() == FRAME_AMAX)), (trial, kind)
            assert np.isfinite(dup), (trial, kind, u)
            exact = sigma2 * _exact_d2(q, r, k)
            assert Fraction(dup) >= exact, (trial, kind, dup, float(exact))
            if kind == 0:      # not vacuous: within a few per cent and an absolute allowance of the exact value
                assert dup <= float(exact) * 1.05 + 0.02 / ratio ** 2 + 1e-4, (trial, dup, float(exact))
            checked_far += far
            checked_edge += kind == 1
    assert checked_far > 100 and checked_edge > 100


# ---- the flag -------------------------------------------------------------------------------------------------------------------

def test_flag_value_and_rejections(pkg):
    assert pkg.QUERY_TOPK_FRAMES == 8
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        assert re.search(r"^#define KNN_QUERY_TOPK_FRAMES 8u$", f.read(), flags=re.M)
    L = pkg.lib()
    # Without an index these calls fail whatever the flags are: they show only that nothing crashes before the argument check.
    # What carries the check here is the masks' source text below; the behaviour — 16 rejected and 15 accepted by the top-K
    # entry, 8 rejected by the 1-NN entries, each with a real index — is in tests/test_frames_topk_gpu.py.
    assert L.knn_index_query_topk(None, 0, 1, 1, None, None, None, None, 16) != 0
    for flags in range(16):
        assert L.knn_index_query_topk(None, 0, 1, 1, None, None, None, None, flags) != 0      # (no index: still an error)
    assert L.knn_index_query(None, 0, 1, None, None, None, None, pkg.QUERY_TOPK_FRAMES) != 0
    assert L.knn_index_query_keys_ex(None, 0, 1, None, None, None, pkg.QUERY_TOPK_FRAMES) != 0
    # the masks themselves: the top-K entry admits exactly the four flags (values up to 15), the 1-NN entries only INIT_KEYS
    with open(os.path.join(ROOT, "multicore_hw2_amd", "csrc", "knn_api.cpp")) as f:
        src = f.read()
    masks = re.findall(r"flags & ~\(unsigned\)\(?([A-Z_| ]+)\)?\) != 0u", src)
    assert masks, "no flag masks found"
    full = {"KNN_QUERY_INIT_KEYS", "KNN_QUERY_TOPK_PARTIAL", "KNN_QUERY_TOPK_GRID", "KNN_QUERY_TOPK_FRAMES"}
    sets = [set(s.strip() for s in mk.split("|")) for mk in masks]
    assert sets.count(full) == 1, sets
    assert all(s == full or s == {"KNN_QUERY_INIT_KEYS"} for s in sets), sets


# ---- what the compiler made of the new kernels ---------------------------------------------------------------------------

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_frame_kernels_use_no_scratch_and_stay_within_their_twins_registers(tmp_path):
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

    def one(pattern):
        names = [n for n in meta if re.search(pattern, n)]
        assert len(names) == 1, (pattern, names)
        return names[0]

    records = [n for n in meta if "knn_cells_frame_records_kernel" in n]
    assert len(records) == 3, records
    forms = set()
    for name in records:
        dyn, u8 = re.search(r"frame_records_kernelILb([01])ELb([01])E", name).groups()
        forms.add((int(dyn), int(u8)))
        twin = one(r"knn_cells_scan_kernelILb%sELi0ELb0ELi1ELb1ELb0ELb%sE" % (dyn, u8))
        assert meta[name][1] == 0, (name, meta[name])
        assert meta[name][0] <= meta[twin][0], (name, meta[name], meta[twin])
        assert "v_mfma" in bodies[name]
        assert not re.search(r"\b(global|flat)_atomic_[us]?min_x2\b", bodies[name]), name      # record-only: no key is folded
    assert forms == COMPILED
    preps = [n for n in meta if re.search(r"knn_cells_prep_kernelILi\dELi\dELi\dELb1ELb1E", n)]
    assert len(preps) == 2, preps
    for name in preps:
        pw, sd, kt = re.search(r"prep_kernelILi(\d)ELi(\d)ELi(\d)E", name).groups()
        assert (sd, kt) == ("2", "1")
        twin = one(r"knn_cells_prep_kernelILi%sELi2ELi1ELb1ELb0E" % pw)
        assert meta[name][1] == 0, (name, meta[name])
        assert meta[name][0] <= meta[twin][0], (name, meta[name], meta[twin])
        assert "v_mfma" in bodies[name]
