"""Inputs that put rows inside the filters' error margin and queries out at the filters' reach (test infrastructure; numpy only).
Used by tests/test_filter_margin_gpu.py; its own conditions are checked on the CPU by tests/test_margin_cases_logic.py.

Family A, shells: uniform rows in [0,1)^k and, around each of m queries in [0.2,0.8)^k, S rows at radii d (1 + j 1e-5), j = 0 .. S-1,
in random directions (float64, rounded to fp32), scattered over random row numbers.  The radii differ by 1e-5 relative; a row's
fp16 score errs by hundreds of times that, so the order by score is scrambled against the order by v0 distance and the true winner
has to pass a threshold drawn from ANOTHER row's lower score.  The generator guarantees (and check_shells re-derives in float64)
that every row outside a query's shell is further than 1.002 x the outermost radius: the v0 order of the first S rows of a query is
then an order of its shell rows alone (v0's fp32 sum is within (k + 3) 2^-24 relative of the exact distance: 4e-5 at k = 600), so
the oracle for K <= S needs the S shell rows only.

Family B, ladder: queries at offset h 2^e from the box middle c (h = half the rows' range), e = 0 .. 20, along +axis 0, -axis k-1
(for k > 16 a dimension the cells are not cut on), the alternating-sign diagonal and, for k > 16, +axis 16; the other coordinates
uniform in the box.  Two rungs past fp32: offset 1e20 (v0's distance overflows to +INF) and 3e38."""
import numpy as np

from tests.topk_oracle import topk_keys

SHELL_M, SHELL_S, SHELL_STEP = 256, 24, 1e-5
FP16_STEP_OF_BOX = 2.0 ** -11          # one fp16 step of a coordinate at the edge of a frame whose box half-width is < 1
MIN_RADIUS = 16 * FP16_STEP_OF_BOX     # a shell is at least 16 fp16 steps wide: NOT "tighter than the fp16 step"
CLEARANCE = 1.002                      # every other row is beyond CLEARANCE x the outermost radius
# floors of the two guard shares (asserted on the CPU for every k of the table and on the GPU for the inputs actually used)
WINNER_NOT_MIN_FLOOR, TOP8_DIFFERS_FLOOR = 0.75, 0.9

RUNGS_ALL = tuple(range(21))
RUNGS_FEW = (0, 4, 8, 10, 11, 13, 16)
RUNG_IN_REACH, RUNG_OUT_OF_REACH = 8, 13   # e <= 8: inside every frame's reach; e >= 13: outside (see reach_in_half_widths)
PAST_FP32 = (1e20, 3e38)
AMAX_LIMIT = 1024.0                    # kAmaxLimit, knn_filter_dev.h: frame units


def shell_radius(k):
    """d per k: >= MIN_RADIUS, and small enough that no uniform row of 2^17 falls inside a shell (k 3 and 5: the generator
    places the queries where that holds)."""
    return 0.008 if k <= 3 else 0.01 if k <= 5 else 0.02 if k <= 8 else 0.03


def frame_sigma(h):
    """frame_scale (knn_filter.hip) restated: the power of two that brings the box half-width h into [0.5, 1)."""
    if h <= 0.0:
        return 1.0
    _, ex = np.frexp(h)
    return float(np.ldexp(1.0, -int(ex)))


def reach_in_half_widths(h):
    """The filter's reach from the frame centre, in units of the half-width h of its box: AMAX_LIMIT / (h sigma) — in
    (1024, 2048] for every h, because h sigma lies in [0.5, 1)."""
    return AMAX_LIMIT / (h * frame_sigma(h))


def _min_dist2_to(points, rows, chunk=128):
    """float64 [len(points)]: squared distance to the nearest of `rows`."""
    P = np.asarray(points, dtype=np.float64)
    Rr = np.asarray(rows, dtype=np.float64)
    rn = (Rr * Rr).sum(axis=1)
    out = np.empty(P.shape[0])
    for c0 in range(0, P.shape[0], chunk):
        p = P[c0:c0 + chunk]
        d = (p * p).sum(axis=1)[:, None] + rn[None, :] - 2.0 * (p @ Rr.T)
        out[c0:c0 + chunk] = d.min(axis=1)
    return out


def make_shells(k, n, seed, m=SHELL_M, S=SHELL_S, d=None):
    """dict(R [n][k] fp32, Q [m][k] fp32, members [m][S] row numbers (member j at radius d (1 + j 1e-5)), d)."""
    d = shell_radius(k) if d is None else d
    assert d >= MIN_RADIUS
    rng = np.random.default_rng(seed)
    R = rng.random((n, k), dtype=np.float32)
    slots = rng.choice(n, m * S, replace=False)
    background = np.ones(n, dtype=bool)
    background[slots] = False
    outer = d * (1.0 + (S - 1) * SHELL_STEP)
    # queries: candidates in [0.2, 0.8)^k with no background row within the clearance, then pairwise apart so that no shell
    # reaches into another's clearance
    cand = (0.2 + 0.6 * rng.random((4 * m, k))).astype(np.float32)
    clear = _min_dist2_to(cand, R[background]) > (CLEARANCE * 1.001 * outer) ** 2
    apart = (2.0 * outer * CLEARANCE * 1.001) ** 2
    picked = []
    for i in np.flatnonzero(clear):
        c = cand[i].astype(np.float64)
        if all(((c - cand[j].astype(np.float64)) ** 2).sum() > apart for j in picked):
            picked.append(i)
            if len(picked) == m:
                break
    assert len(picked) == m, (k, n, len(picked))
    Q = np.ascontiguousarray(cand[picked])
    u = rng.normal(0.0, 1.0, (m, S, k))
    u /= np.sqrt((u * u).sum(axis=2, keepdims=True))
    radii = d * (1.0 + np.arange(S) * SHELL_STEP)
    rows = Q.astype(np.float64)[:, None, :] + radii[None, :, None] * u
    members = slots.reshape(m, S)
    R[members.reshape(-1)] = rows.reshape(m * S, k).astype(np.float32)
    return dict(k=k, n=n, R=R, Q=Q, members=members, d=d)


def check_shells(case):
    """The input's own conditions, re-derived in float64 from R, Q and members alone: (smallest distance of a row outside the
    query's shell) / (largest distance of a shell row), minimum over the queries — must exceed CLEARANCE —, and whether the S v0
    distances of every shell are distinct."""
    R, Q, members, k = case["R"], case["Q"], case["members"], case["k"]
    m, S = members.shape
    Rd = R.astype(np.float64)
    rn = (Rd * Rd).sum(axis=1)
    worst = np.inf
    for c0 in range(0, m, 64):
        q = Q[c0:c0 + 64].astype(np.float64)
        D = (q * q).sum(axis=1)[:, None] + rn[None, :] - 2.0 * (q @ Rd.T)
        rows = np.arange(q.shape[0])[:, None]
        inner = D[rows, members[c0:c0 + 64]].max(axis=1)
        D[rows, members[c0:c0 + 64]] = np.inf
        worst = min(worst, float(np.sqrt((D.min(axis=1) / inner).min())))
    keys = shell_topk_keys(case, S)
    distinct = bool(((keys[:, 1:] >> np.uint64(32)) > (keys[:, :-1] >> np.uint64(32))).all())
    return worst, distinct


def shell_topk_keys(case, K, base=0, gids=None):
    """uint64 [m][K], K <= S: tests/topk_oracle.topk_keys of every query over its shell rows (which hold its S nearest: see the
    module's docstring), carrying base + row — or gids[row] — as the global number."""
    R, Q, members, k = case["R"], case["Q"], case["members"], case["k"]
    assert K <= members.shape[1]
    out = np.empty((Q.shape[0], K), dtype=np.uint64)
    for q in range(Q.shape[0]):
        mem = np.sort(members[q])
        g = mem.astype(np.uint64) + np.uint64(base) if gids is None else np.asarray(gids)[mem].astype(np.uint64)
        out[q] = topk_keys(Q[q], R[mem], k, K, gids=g)[0]
    return out


def fp16_scores(case, centre=0.5, h=0.5 * (1.0 + 1.0 / 16.0)):
    """The filter's score of every shell row against its query, restated: rows and queries centred (fp32 subtract), scaled by the
    frame's power of two and rounded to fp16; S = |r~|^2 - 2 q~.r~ (float64 from there on: the matrix core's own accumulation
    error is thousands of times below the rounding of the operands).  The frame is the box middle and frame_scale's sigma for a
    box of half-width h — not the library's exact centre: the shares below are statistical.  float64 [m][S]."""
    R, Q, members = case["R"], case["Q"], case["members"]
    sigma = np.float32(frame_sigma(h))
    c = np.float32(centre)
    qt = ((Q - c) * sigma).astype(np.float16).astype(np.float64)
    rt = ((R[members] - c) * sigma).astype(np.float16).astype(np.float64)
    return (rt * rt).sum(axis=2) - 2.0 * (rt * qt[:, None, :]).sum(axis=2)


def guard_shares(case):
    """(share of queries whose v0 winner is NOT the shell row of lowest fp16 score, share whose v0 top-8 is not the set of the 8
    lowest scores).  Both near 1 is what makes the input a test of the margin."""
    members = case["members"]
    m, S = members.shape
    sc = fp16_scores(case)
    want = shell_topk_keys(case, 8)
    want_rows = (want & np.uint64(0xFFFFFFFF)).astype(np.int64)
    by_score = np.take_along_axis(members, np.argsort(sc, axis=1, kind="stable"), axis=1)
    not_min = float(np.mean(by_score[:, 0] != want_rows[:, 0]))
    differs = float(np.mean([set(by_score[q, :8]) != set(want_rows[q]) for q in range(m)]))
    return not_min, differs


# ---- family B --------------------------------------------------------------------------------------------------------------------

def directions(k):
    """(name, dimensions moved, their signs) — the offset is the same magnitude in every dimension moved."""
    out = [("+axis0", [0], [1.0]), ("-axis_last", [k - 1], [-1.0]),
           ("diagonal", list(range(k)), [1.0 if j % 2 == 0 else -1.0 for j in range(k)])]
    if k > 16:
        out.append(("+axis16", [16], [1.0]))
    return out


def rung_offset(e, h=0.5):
    """Rung e: h 2^e; the two rungs past fp32 are named by their offsets."""
    return h * 2.0 ** e if e in RUNGS_ALL else float(e)


def rung_queries(k, e, rng, per_direction=4, c=0.5, h=0.5):
    """fp32 [per_direction x directions][k]: uniform in the box, then the moved dimensions set to c +- offset."""
    off = rung_offset(e, h)
    dirs = directions(k)
    Q = rng.random((per_direction * len(dirs), k), dtype=np.float32)
    for i, (_, dims, signs) in enumerate(dirs):
        for j, s in zip(dims, signs):
            Q[i * per_direction:(i + 1) * per_direction, j] = np.float32(c + s * off)
    return Q


def rung_batch(k, e, box_queries, rng, m=64):
    """One batch of m: the rung's queries first, then queries inside the box (a prefix of box_queries: shared by every rung)."""
    far = rung_queries(k, e, rng)
    return np.ascontiguousarray(np.concatenate([far, box_queries[:m - far.shape[0]]]))


def expected_fallback(e):
    """stats[2] == 1 of a batch holding rung e: False (in reach), True (out of reach) or None (9 .. 12: depends on where in
    [0.5, 1) the frame's scaled half-width fell).  Derived, not measured: the rung's largest |coordinate - c| is h 2^e with h the
    TRUE half-width; the frame's box has half-width H in [h (1 - 1/16), h (1 + 1/16)] (the build sample's range, widened by 1/32
    on either side) with its centre within h/16 of c, and H sigma lies in [0.5, 1) — so in frame units the rung sits between
    0.4 x 2^e and 1.2 x 2^e: inside kAmaxLimit = 1024 for e <= 8 (at most 308), beyond it for e >= 13 (at least 3276).  The rungs
    between are left to the frame."""
    if e not in RUNGS_ALL:
        return True
    return False if e <= RUNG_IN_REACH else True if e >= RUNG_OUT_OF_REACH else None


# ---- the forms: one row per compiled way a row can be discarded ---------------------------------------------------------------------

N17 = (1 << 17) + 999
DENSE = {"path": 2, "cells": 2}
FP16 = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2}          # tests/test_cells_topk_gpu.py
BINS = {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 2}
CELL_U8 = {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 1}
# name, kind, k, rows, options, way of a 1-NN call (stats[0]), way of a top-K call under `topk_cells` 1 (1: the exact top-K scan —
# per-cell frames and the grid index have no top-K filter), whether the rows the filter scores are fp16 (the guard shares and
# stats[2] == 0 apply), rungs of the ladder
FORMS = []


def _form(name, kind, k, n, opts, one_nn, topk, fp16=True, rungs=RUNGS_ALL, m_shell=SHELL_M):
    FORMS.append(dict(name=name, kind=kind, k=k, n=n, opts=dict(opts), one_nn=one_nn, topk=topk, fp16=fp16, rungs=rungs,
                      m_shell=m_shell))


for _k in (3, 16, 32):
    _form(f"dense_k{_k}", "dense", _k, 70000, DENSE, 2, 2)
# the LDS-tiled scan takes k 128 from 16 query tiles on (m > 480): its batches are padded to 512 with queries inside the box
_form("tiled_k128_run", "dense", 128, 66000, dict(DENSE, run_thresholds=0), 2, 2, rungs=RUNGS_FEW, m_shell=512)
_form("tiled_k128_fixed", "dense", 128, 66000, dict(DENSE, run_thresholds=2), 2, 2, rungs=RUNGS_FEW, m_shell=512)
_form("tiled_k200_run", "dense", 200, 66000, dict(DENSE, run_thresholds=0), 2, 2, rungs=RUNGS_FEW)
_form("tiled_k200_fixed", "dense", 200, 66000, dict(DENSE, run_thresholds=2), 2, 2, rungs=RUNGS_FEW)
_form("chunked_k600", "dense", 600, 65600, DENSE, 2, 2, rungs=RUNGS_FEW)
for _k in (3, 5, 16):
    for _deal in (1, 2):
        for _lists in (1, 2):
            _form(f"cells_fp16_k{_k}_deal{_deal}_lists{_lists}", "cells", _k, N17, dict(FP16, scan_deal=_deal, cells_lists=_lists),
                  4, 4)
for _k in (20, 30):
    _form(f"cells_nif_k{_k}", "cells", _k, N17, FP16, 4, 4)
for _k in (31, 32):
    _form(f"cells_window_k{_k}", "cells", _k, N17, FP16, 4, 4)
for _k in (8, 16):
    _form(f"cells_centred_k{_k}", "cells", _k, N17, dict(FP16, cells_centre=1), 4, 1)
_form("cells_u8_cell_k16", "cells", 16, N17, CELL_U8, 4, 1, fp16=False)
for _k in (8, 16):
    _form(f"cells_u8_bins_k{_k}", "cells", _k, N17, BINS, 4, 4, fp16=False)
_form("shards_k16", "shards", 16, 1 << 18, {}, 4, 4)
_form("grid_k3", "grid", 3, 40000, {}, 3, 1)
FORM_NAMES = [f["name"] for f in FORMS]
# options a form may set, all of them reset after it (build-time and per-call ones alike)
OPTIONS = ("path", "cells", "cells_rows", "cells_centre", "cells_u8_frame", "scan_deal", "cells_lists", "run_thresholds",
           "topk_cells")
