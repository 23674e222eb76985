"""8-bit rows in per-dimension bin frames (option `cells_u8_frame` = 2): the host copies of the quantiser (knn_u8_bin_code through
knn_debug_u8_bin_row) and of the scan's threshold (knn_u8_bin_threshold through knn_debug_u8_bin_threshold), against float64.

The scan passes a row when  N'' + B.r^  <  thr - B.w_c  (knn_filter_dev.h).  For random (query, row) pairs whose true distance is
within Dup, the score — with the matrix core's worst accumulation error added against us — must pass."""
import ctypes

import numpy as np
import pytest

import multicore_hw2_amd as pkg


def _bin_row(row, centre, scale, w):
    k = row.size
    f = pkg.lib().knn_debug_u8_bin_row
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.c_double)]
    f.restype = ctypes.c_int
    r = np.ascontiguousarray(row, dtype=np.float32)
    c = np.ascontiguousarray(centre, dtype=np.float32)
    wv = np.ascontiguousarray(w, dtype=np.float32)
    codes = np.zeros(k, dtype=np.uint8)
    err = ctypes.c_double()
    assert f(k, r.ctypes.data, c.ctypes.data, ctypes.c_float(scale), wv.ctypes.data, codes.ctypes.data, ctypes.byref(err)) == 0
    return codes, err.value


def _threshold_fn():
    f = pkg.lib().knn_debug_u8_bin_threshold
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                  ctypes.POINTER(ctypes.c_float)]
    f.restype = ctypes.c_int
    out = ctypes.c_float()

    def thr(k, b16, dup, ratio, er, nmax, w1):
        bits = np.ascontiguousarray(b16.astype(np.float16).view(np.uint16))
        assert f(k, bits.ctypes.data, dup, ratio, er, nmax, w1, ctypes.byref(out)) == 0
        return out.value
    return thr


def _w_of(rng, k, lim=4.0):
    return (np.rint(rng.uniform(-lim, lim, k) * 64.0) / 64.0).astype(np.float32)   # multiples of 2^-6: exact in fp16


@pytest.mark.parametrize("k", [3, 8, 15, 16])
def test_bin_rows_are_within_err_of_the_exact_offsets(k):
    rng = np.random.default_rng(100 + k)
    worst = 0.0
    for _ in range(3000):
        centre = (rng.random(k, dtype=np.float32) * 200.0 - 100.0).astype(np.float32)
        e = int(rng.integers(-12, 8))
        scale = np.float32(2.0 ** e)
        w = _w_of(rng, k)
        # a row inside its bin box: |(x - centre) s - w| <= 1
        row = (centre + (w.astype(np.float64) + rng.uniform(-1.0, 1.0, k)) / float(scale)).astype(np.float32)
        codes, err = _bin_row(row, centre, scale, w)
        exact = (row.astype(np.float64) - centre.astype(np.float64)) * float(scale) - w.astype(np.float64)
        deq = (codes.astype(np.float64) - 128.0) / 128.0
        dev = np.abs(exact - deq)
        assert dev.max() <= err * (1 + 1e-6), (dev.max(), err)
        assert err <= 2.0 ** -7 + 2.0 ** -18
        worst = max(worst, dev.max())
    assert worst > 2.0 ** -9     # the test reaches the rounding's scale


def test_bin_rows_adversarial():
    """Half-way codes, the clamp, zero and large offsets, subnormal distances."""
    thr = [0.0, 1.0, -1.0, 127.5 / 128, -127.5 / 128, 0.5 / 128, -0.5 / 128, 1e-40, 1.0 + 2.0 ** -20]
    for centre0 in (0.0, 3.0, 4096.25, -1.0e5):
        for scale in (1.0, 2.0 ** -10, 16.0):
            for wv in (0.0, 0.015625, -31.984375, 17.5):
                for v in thr:
                    centre = np.full(16, centre0, dtype=np.float32)
                    w = np.full(16, wv, dtype=np.float32)
                    row = (centre + np.float32((wv + v) / scale)).astype(np.float32)
                    codes, err = _bin_row(row, centre, np.float32(scale), w)
                    exact = (row.astype(np.float64) - centre.astype(np.float64)) * scale - wv
                    deq = (codes.astype(np.float64) - 128.0) / 128.0
                    assert np.abs(exact - deq).max() <= err * (1 + 1e-6), (centre0, scale, wv, v)


def _f32_dot(b, w):
    """B.w_c as the scan makes it: per half, exact fp32 products summed in fp32 in dimension order, then half 0 + half 1."""
    prod = (b.astype(np.float32) * w.astype(np.float32)).astype(np.float32)   # exact
    halves = []
    for h in (0, 1):
        acc = prod[8 * h]
        for i in range(1, 8):
            acc = np.float32(acc + prod[8 * h + i])
        halves.append(acc)
    return np.float32(halves[0] + halves[1])


@pytest.mark.parametrize("k", [16, 8])
def test_bin_threshold_passes_every_pair_within_dup(k):
    """200 000 random pairs (float64 reference): a row at true distance <= Dup is never ruled out by the fp32 threshold, even
    with the matrix core's accumulation error (2^-18 of the magnitudes, the allowance knn_bound_consts pins) against it."""
    rng = np.random.default_rng(7 + k)
    thr = _threshold_fn()
    n = 100_000   # per k: 200 000 pairs in all
    slack_seen = []
    for it in range(n):
        e = int(rng.integers(0, 5))
        ratio = np.float32(2.0 ** e)
        w = np.zeros(16, dtype=np.float32)
        w[:k] = _w_of(rng, k, lim=float(rng.choice([0.5, 2.0, 8.0])))
        r = np.zeros(16)
        r[:k] = rng.uniform(-1.0, 1.0, k)
        code = np.clip(np.rint(r * 128.0), -128, 127)
        rh = code / 128.0
        er = np.float32(np.abs(r - rh).max() * (1 + 1e-6) + 2.0 ** -40)
        # the query in the shard's frame (sigma units), rounded to fp16 there, times 2^e: the scan's B operand = -2 p~
        row_full = w.astype(np.float64) + r                       # the exact row, s units
        spread = float(rng.choice([0.01, 0.3, 1.0, 3.0]))
        p = np.zeros(16)
        p[:k] = row_full[:k] + rng.normal(0.0, spread, k)          # query near the row, s units
        h = (p / float(ratio)).astype(np.float32).astype(np.float16)
        b = (h.astype(np.float32) * np.float32(-2.0) * ratio).astype(np.float16)
        D = float(np.sum((p - row_full) ** 2))                     # true squared distance, s units
        dup_sigma = np.float32(D / float(ratio) ** 2 * (1.0 + rng.uniform(0.0, 1e-3)))
        if float(dup_sigma) * float(ratio) ** 2 < D:
            dup_sigma = np.nextafter(dup_sigma, np.float32(np.inf))
        full = w.astype(np.float64) + rh
        nexact = float(np.sum(full ** 2))
        nstored = np.float32(nexact)
        bb = b.astype(np.float64)
        dotr = float(np.sum(bb * rh))
        mag = abs(float(nstored)) + float(np.sum(np.abs(bb * rh)))
        score = float(nstored) + dotr + 2.0 ** -18 * mag            # the MFMA's error, against us
        w1 = np.float32(np.sum(np.abs(w.astype(np.float64))) * (1 + 1e-6))
        t = thr(k, b, float(dup_sigma), float(ratio), float(er), float(nstored), float(w1))
        th = np.float32(np.float32(t) - _f32_dot(b, w))
        assert score < float(th), (it, score, float(th), D)
        slack_seen.append((float(th) - score) / max(D, 1e-3))
    # and it is not vacuous: the slack stays a small multiple of the distance for the pairs that matter
    assert np.median(slack_seen) < 0.5
