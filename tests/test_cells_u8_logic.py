"""8-bit rows of the cell-pruned scan (option `cells_rows`): the host copy of the quantiser (knn_u8_code through the
knn_debug_u8_row hook) and its bound.  For random and adversarial rows in a cell's frame, the dequantised row r^ =
(code - 128) / 128 lies within eta of the exact row (double arithmetic) — the row's part of eta alone must cover it."""
import ctypes

import numpy as np
import pytest

import multicore_hw2_amd as pkg


def _u8_row(row, centre, scale, amax=1.0):
    k = row.size
    f = pkg.lib().knn_debug_u8_row
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.c_double)]
    f.restype = ctypes.c_int
    r = np.ascontiguousarray(row, dtype=np.float32)
    c = np.ascontiguousarray(centre, dtype=np.float32)
    codes = np.zeros(k, dtype=np.uint8)
    out = (ctypes.c_double * 2)()
    assert f(k, r.ctypes.data, c.ctypes.data, ctypes.c_float(scale), amax, codes.ctypes.data, out) == 0
    return codes, out[0], out[1]


def _check(row, centre, scale):
    codes, er, eta = _u8_row(row, centre, scale)
    exact = (row.astype(np.float64) - centre.astype(np.float64)) * scale
    deq = (codes.astype(np.float64) - 128.0) / 128.0
    dev = np.abs(exact - deq)
    assert dev.max() <= er * (1 + 1e-6), (dev.max(), er)
    assert np.sqrt(np.sum(dev ** 2)) <= eta, (np.sqrt(np.sum(dev ** 2)), eta)
    return dev.max(), er


@pytest.mark.parametrize("k", [3, 8, 15, 16])
def test_u8_rows_are_within_eta_of_the_exact_rows(k):
    rng = np.random.default_rng(k)
    worst = 0.0
    for _ in range(3000):
        centre = (rng.random(k, dtype=np.float32) * 2000.0 - 1000.0).astype(np.float32)
        e = int(rng.integers(-20, 10))
        scale = np.float32(2.0 ** e)
        row = (centre + (rng.random(k) * 2.0 - 1.0) / scale).astype(np.float32)   # inside the cell's box: |v| <= 1
        d, er = _check(row, centre, scale)
        worst = max(worst, d)
        assert er <= 2.0 ** -7 + 2.0 ** -20   # (2^-8 + 2^-22 unless the fp32 row, rounded, left the box: the clamp)
    assert worst > 2.0 ** -9     # the test reaches the rounding's scale


@pytest.mark.parametrize("k", [1, 16])
def test_u8_adversarial_rows(k):
    """Half-way values (round to even), the clamp at +1, the box's edges, zeros, subnormal offsets, huge centres."""
    cases = [0.0, 1.0, -1.0, 127.5 / 128, -127.5 / 128, 0.5 / 128, 1.5 / 128, -0.5 / 128, 1e-40, -1e-30,
             np.nextafter(np.float32(1.0), np.float32(0.0)), 1.0 + 2.0 ** -20]
    for centre0 in (0.0, 3.0, 4096.25, -1.0e6):
        for scale in (1.0, 2.0 ** -12, 256.0):
            for v in cases:
                centre = np.full(k, centre0, dtype=np.float32)
                row = (centre + np.float32(v / scale)).astype(np.float32)
                d, er = _check(row, centre, np.float32(scale))
                assert abs(v) > 1.0 or er <= 2.0 ** -7 + 2.0 ** -20, (v, er)   # (outside the box: still covered, by its own er)


def test_cells_rows_option_is_range_checked():
    assert pkg.get_option("cells_rows") == 0
    with pytest.raises(Exception):
        pkg.set_option("cells_rows", 3)
    pkg.set_option("cells_rows", 2)
    assert pkg.get_option("cells_rows") == 2
    pkg.set_option("cells_rows", 0)
