"""tests/margin_cases.py on the CPU: the conditions of the inputs tests/test_filter_margin_gpu.py feeds the filters — they are
properties of the inputs, not of any kernel — for every (k, rows) of its table of forms."""
import numpy as np
import pytest

from tests import margin_cases as mc
from tests.topk_oracle import keys_index, topk_keys

SHAPES = sorted({(f["k"], f["n"]) for f in mc.FORMS})
FP16_KS = sorted({f["k"] for f in mc.FORMS if f["fp16"]})


def test_the_table_names_every_form_once():
    assert len(set(mc.FORM_NAMES)) == len(mc.FORMS) == 31
    assert {f["k"] for f in mc.FORMS if f["kind"] == "dense"} == {3, 16, 32, 128, 200, 600}
    cells = [f for f in mc.FORMS if f["kind"] == "cells"]
    assert sum(f["name"].startswith("cells_fp16") for f in cells) == 12          # 3 k x both deals x both list makers
    assert {f["k"] for f in cells if "nif" in f["name"]} == {20, 30} and {f["k"] for f in cells if "window" in f["name"]} == {31, 32}
    for f in mc.FORMS:
        assert set(f["opts"]) <= set(mc.OPTIONS), f["name"]
        assert f["rungs"] == (mc.RUNGS_FEW if f["k"] > 32 else mc.RUNGS_ALL), f["name"]
        assert f["one_nn"] == {"dense": 2, "cells": 4, "shards": 4, "grid": 3}[f["kind"]]


@pytest.mark.parametrize("k,n", SHAPES, ids=[f"k{k}_n{n}" for k, n in SHAPES])
def test_every_shell_is_its_querys_nearest_rows_and_scrambled_by_fp16(k, n):
    case = mc.make_shells(k, n, seed=1000 + k)
    R, Q, members, d = case["R"], case["Q"], case["members"], case["d"]
    assert Q.shape == (mc.SHELL_M, k) and members.shape == (mc.SHELL_M, mc.SHELL_S)
    assert d >= mc.MIN_RADIUS and R.dtype == np.float32 and Q.dtype == np.float32
    assert (Q >= 0.2).all() and (Q < 0.8).all() and (R >= 0.0).all() and (R < 1.0).all()
    assert np.unique(members).size == members.size                     # scattered over distinct row numbers ...
    assert (np.diff(members, axis=1) < 0).any() and members.max() > n // 2     # ... not in radius order, not at the front
    # the shell rows sit where they should: radius d (1 + j 1e-5) to fp32 rounding of the coordinates (2^-24 each)
    r = np.sqrt(((R[members].astype(np.float64) - Q.astype(np.float64)[:, None, :]) ** 2).sum(axis=2))
    want_r = d * (1.0 + np.arange(mc.SHELL_S) * mc.SHELL_STEP)
    assert np.abs(r / want_r[None, :] - 1.0).max() < np.sqrt(k) * 2.0 ** -24 / d
    clearance, distinct = mc.check_shells(case)
    assert clearance > mc.CLEARANCE, clearance      # the oracle's 24 nearest rows of every query are exactly its shell
    assert distinct                                 # and no two of them tie: the order is decided by distance alone
    if k in FP16_KS:
        not_min, differs = mc.guard_shares(case)
        assert not_min >= mc.WINNER_NOT_MIN_FLOOR and differs >= mc.TOP8_DIFFERS_FLOOR, (k, not_min, differs)


@pytest.mark.parametrize("k,n", [(3, 40000), (5, mc.N17), (16, 70000)])
def test_the_shell_oracle_is_the_oracle_over_all_rows(k, n):
    """shell_topk_keys ranks 24 rows; tests/topk_oracle.topk_keys over the whole set says the same (a sample of the queries)."""
    case = mc.make_shells(k, n, seed=1000 + k)
    sel = slice(0, 24)
    full = topk_keys(case["Q"][sel], case["R"], k, mc.SHELL_S, base=7, chunk=8)
    np.testing.assert_array_equal(mc.shell_topk_keys(case, mc.SHELL_S, base=7)[sel], full)
    assert (np.sort(keys_index(full) - 7, axis=1) == np.sort(case["members"][sel], axis=1)).all()


def test_frame_sigma_restates_frame_scale():
    for h, want in ((0.5, 1.0), (0.53125, 1.0), (0.999, 1.0), (1.0, 0.5), (0.26, 2.0), (0.25, 2.0), (300.0, 2.0 ** -9), (3e-5, 2.0 ** 15)):
        s = mc.frame_sigma(h)
        assert s == want and 0.5 <= h * s < 1.0, (h, s)
    rng = np.random.default_rng(5)
    for h in np.exp(rng.uniform(np.log(1e-12), np.log(1e12), 2000)):
        assert 1024.0 < mc.reach_in_half_widths(h) <= 2048.0


def test_rung_arithmetic():
    assert mc.RUNGS_ALL == tuple(range(21)) and set(mc.RUNGS_FEW) <= set(mc.RUNGS_ALL)
    assert [mc.rung_offset(e) for e in (0, 8, 13, 20)] == [0.5, 128.0, 4096.0, 524288.0]
    assert mc.rung_offset(1e20) == 1e20 and mc.rung_offset(3e38) == 3e38
    # in frame units (see expected_fallback): every rung up to 8 inside kAmaxLimit, every rung from 13 outside, for any frame
    for e in mc.RUNGS_ALL:
        lo, hi = 0.4 * 2.0 ** e, 1.2 * 2.0 ** e
        want = False if hi <= mc.AMAX_LIMIT and e <= 8 else True if lo > mc.AMAX_LIMIT and e >= 13 else None
        assert mc.expected_fallback(e) is want, e
    assert mc.expected_fallback(1e20) is True and mc.expected_fallback(3e38) is True
    for k in (3, 16, 20, 600):
        rng = np.random.default_rng(k)
        dirs = mc.directions(k)
        assert len(dirs) == (4 if k > 16 else 3)
        for e in (0, 8, 14, 20, 1e20, 3e38):
            Q = mc.rung_queries(k, e, rng)
            off = mc.rung_offset(e)
            assert Q.shape == (4 * len(dirs), k) and Q.dtype == np.float32 and np.isfinite(Q).all()
            for i, (name, dims, signs) in enumerate(dirs):
                blk = Q[4 * i:4 * i + 4].astype(np.float64)
                moved = np.zeros(k, dtype=bool)
                moved[dims] = True
                np.testing.assert_array_equal(blk[:, moved], np.tile(np.float32(0.5 + np.array(signs) * off).astype(np.float64), (4, 1)))
                assert ((blk[:, ~moved] >= 0.0) & (blk[:, ~moved] < 1.0)).all()
                # the rung's reach is its largest |coordinate - c|, in every direction the same
                assert np.abs(np.abs(blk - 0.5).max(axis=1) / max(off, 0.5) - 1.0).max() < 1e-6, (k, e, name)
        box = rng.random((52, k), dtype=np.float32)
        B = mc.rung_batch(k, 13, box, rng)
        assert B.shape == (64, k) and (B[4 * len(dirs):] == box[:64 - 4 * len(dirs)]).all()
    assert "+axis16" in [d[0] for d in mc.directions(20)] and mc.directions(20)[1][1] == [19]
    # past fp32: v0's squared difference overflows for both
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e20) * np.float32(1e20)) and np.isinf(np.float32(3e38) * np.float32(3e38))
