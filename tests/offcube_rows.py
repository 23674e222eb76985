"""Rows off the unit cube for the radius family on the cell-pruned scan (test infrastructure, no GPU import): the shards, the
queries, the oracle's distances, the radii, the masks and the own-row windows that tests/test_offcube_rows_logic.py (CPU),
tests/test_offcube_within_gpu.py, tests/test_offcube_each_gpu.py, tests/test_offcube_self_gpu.py and
tests/test_offcube_masked_gpu.py share.

Every batch is N17 rows and M = 64 queries of one distribution — the kinds tests/test_cells_gpu.py's 1-NN tests build at the same
size:

  uniform    the control: the unit cube, queries spread up to 0.6 beyond it along axis 0 (tests/test_within_cells_gpu.py's kind)
  offset     uniform + 4096.0 in rows and queries: the cell cuts sit at 4096.x
  lattice    coordinates in {0, .25, .5, .75, 1}: rows and queries ON the cuts, distances that many rows hold exactly; every fourth
             query moved 0.75 out along axis 0, so some counts are 0
  clustered  16 blobs of sigma 0.01, queries of sigma 0.02 with a ramp up to 0.1 along axis 0
  skewed     x ** 4: the quantile cuts are far from the middle of the range
  scaled     uniform times a power of two per dimension, exponents from -6 .. 6, the same scales for rows and queries
  copies     every query is a row (distance 0); odd queries are then moved up to 0.6 out along axis 0; 64 further rows are
             overwritten with copies of the 64 source rows

lattice and copies also hold one run of five equal consecutive rows, RUN_FIRST .. RUN_FIRST + 4: the own-row window of the self
tests starts in its middle, so an own row has copies of itself before it, outside the window, and behind it, inside; and query
RUN_QUERY sits on the run: five rows at distance 0 (a lattice of 16 or 20 dimensions has no other equal rows).

Radii come from the oracle's own distances (tests.topk_oracle.v0_dist2): `at` a value some row holds exactly, `below` the next
float towards 0, `zero`, and for lattice and copies `tiny`, the smallest subnormal.  At every radius handed out the oracle's
largest count is at most CAP = 64 — asserted here: nothing drives a record pass over-full.  Everything is made once per
(name, k) and handed out read-only."""
import functools

import numpy as np

from tests.count_oracle import counts_of
from tests.outlier_rows import spread_queries
from tests.self_oracle import self_dist2
from tests.topk_oracle import v0_dist2

N17 = (1 << 17) + 999               # tests/test_within_cells_gpu.py's: the smallest shard that gets a cell-sorted layout
M = 64                              # queries of a batch, and rows of an own-row window
BASE = 11                           # base_index of every index built on these rows
CAP = 64                            # no radius handed out holds more rows than this for any query
NAMES = ("uniform", "offset", "lattice", "clustered", "skewed", "scaled", "copies")
TIED = ("lattice", "copies")        # the distributions with exact copies of rows: a `tiny` radius, a run, a one-per-run mask
KS = (8, 16, 20)
WINDOW_FIRST = 2090                 # 2090 % 64 == 42: the window starts inside a block of 64 rows
RUN_FIRST, RUN = WINDOW_FIRST - 2, 5
RUN_QUERY = 2                       # the query of lattice and copies that sits on the run of equal rows (stays where it is: 2 % 4, even)
INF = np.float32(np.inf)
F32 = np.float32
TINY = float(np.nextafter(F32(0), F32(1)))          # the smallest subnormal
EACH_KINDS = ("held", "below", "zero", "nan", "minus_one")      # of tests.each_oracle.KINDS: those a list-sized cap leaves room for
# the layouts of tests/test_within_cells_gpu.py's matrix the batches run on: (name, k, options)
_FP16 = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2}
_BINS = {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 2}
LAYOUTS = (("fp16_k8", 8, _FP16), ("fp16_k16", 16, _FP16), ("bins_k16", 16, _BINS), ("nif_k20_fixed", 20, dict(_FP16, scan_deal=1)))
PAIRS = [(name, layout) for name in NAMES for layout in LAYOUTS]
PAIR_IDS = [f"{name}-{layout[0]}" for name, layout in PAIRS]
# (distribution, layout) pairs the 1-NN test of tests/test_cells_gpu.py asserts the pruned way for: never skipped
NEVER_SKIPPED = {(name, "fp16_k16") for name in ("uniform", "offset", "skewed", "clustered")}

assert WINDOW_FIRST % 64 and RUN_FIRST < WINDOW_FIRST < RUN_FIRST + RUN - 1


def _frozen(a):
    a.setflags(write=False)
    return a


def seed_of(name, k):
    return 9100 + 100 * NAMES.index(name) + k


@functools.lru_cache(maxsize=None)
def scales(k):
    """float32 [k]: the powers of two of `scaled`, exponents drawn from -6 .. 6 once per k."""
    e = np.random.default_rng(seed_of("scaled", k) + 7).integers(-6, 7, k)
    return _frozen(np.ldexp(F32(1), e).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rows_and_queries(name, k):
    """(R float32 [N17][k], Q float32 [M][k]), read-only."""
    rng = np.random.default_rng(seed_of(name, k))
    n, m = N17, M
    R = rng.random((n, k), dtype=np.float32)
    if name in ("uniform", "offset", "scaled"):
        Q = spread_queries(rng, m, k)
        if name == "offset":
            R += F32(4096.0)
            Q += F32(4096.0)
        elif name == "scaled":
            R *= scales(k)
            Q *= scales(k)
    elif name == "lattice":
        R = (rng.integers(0, 5, (n, k)) * 0.25).astype(np.float32)
        R[RUN_FIRST:RUN_FIRST + RUN] = R[WINDOW_FIRST]
        Q = (rng.integers(0, 5, (m, k)) * 0.25).astype(np.float32)
        Q[::4, 0] += F32(0.75)
        Q[RUN_QUERY] = R[RUN_FIRST]
    elif name == "clustered":
        c = rng.random((16, k), dtype=np.float32)
        R = (c[rng.integers(0, 16, n)] + rng.normal(0, 0.01, (n, k))).astype(np.float32)
        Q = (c[rng.integers(0, 16, m)] + rng.normal(0, 0.02, (m, k))).astype(np.float32)
        Q[:, 0] += np.linspace(0.0, 0.1, m, dtype=np.float32)
    elif name == "skewed":
        R = R ** 4
        Q = rng.random((m, k), dtype=np.float32) ** 4
        Q[:, 0] += np.linspace(0.0, 0.6, m, dtype=np.float32)
    elif name == "copies":
        R[RUN_FIRST:RUN_FIRST + RUN] = R[WINDOW_FIRST]
        free = np.setdiff1d(np.arange(n), np.arange(RUN_FIRST, RUN_FIRST + RUN))
        picked = rng.choice(free, 2 * m, replace=False)
        src, further = picked[:m], picked[m:]
        R[further] = R[src]
        Q = R[src].copy()
        Q[1::2, 0] += np.linspace(0.0, 0.6, m, dtype=np.float32)[1::2]
        Q[RUN_QUERY] = R[RUN_FIRST]
    else:
        raise ValueError(name)
    return _frozen(np.ascontiguousarray(R, dtype=np.float32)), _frozen(np.ascontiguousarray(Q, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def batch(name, k):
    """(R, Q, d float32 [M][N17]): one v0_dist2 per (name, k)."""
    R, Q = rows_and_queries(name, k)
    return R, Q, _frozen(v0_dist2(Q, R, k))


@functools.lru_cache(maxsize=None)
def window(name, k):
    """(first, d float32 [M][N17]): the own-row window WINDOW_FIRST .. + M - 1 and tests.self_oracle.self_dist2 of it (NaN where a row
    meets itself)."""
    R, _ = rows_and_queries(name, k)
    return WINDOW_FIRST, _frozen(self_dist2(R, k, WINDOW_FIRST, M))


def run_rows():
    """The rows of the run of equal rows (lattice, copies)."""
    return np.arange(RUN_FIRST, RUN_FIRST + RUN)


def _near(d, upto):
    fin = np.where(d < INF, d, INF)
    return np.sort(np.partition(fin, upto - 1, axis=1)[:, :upto], axis=1)


def leaving(d, at):
    """uint32 [m]: the rows of every query that hold `at` exactly — those that leave at nextafter(at, 0)."""
    return counts_of(d, at) - counts_of(d, np.nextafter(F32(at), F32(0)))


def choose_at(d, ties=False, need_zero=True, upto=8, room=2 * CAP):
    """The `at` radius of a distance matrix: the j-th nearest distance, j <= upto, of some query, that is positive and at which the
    counts hold a value in 1 .. 63, a zero (need_zero) and none above CAP.  Among those: the one that gives the most queries a hit
    (up to 8), then the most queries none (up to 4), then the first in the order j from `upto` down, the values of one j from their
    median outwards.  ties (lattice): rows of at least two queries hold it exactly, and at least 3 rows of one query leave together
    below it."""
    part = _near(np.asarray(d, dtype=np.float32), room)
    best, best_score = None, -1
    for near in range(upto, 0, -1):
        col = part[:, near - 1]
        held = np.unique(col[(col < INF) & (col > 0)])
        order = np.argsort(np.abs(np.arange(held.size) - held.size // 2), kind="stable")
        for v in held[order]:
            c = (part <= v).sum(axis=1)
            some, none = int(((c >= 1) & (c <= 63)).sum()), int((c == 0).sum())
            if c.max() > CAP or some == 0 or (need_zero and none == 0):
                continue
            gone = (part == v).sum(axis=1)
            if ties and not ((gone > 0).sum() >= 2 and gone.max() >= 3):
                continue
            score = 10 * min(some, 8) + min(none, 4)
            if score > best_score:
                best, best_score = float(v), score
    assert best is not None, "no radius gives a zero and a value in 1 .. 63 (and the ties wanted) among the counts: change the batch"
    return best


def _radii_of(d, name, need_zero=True):
    at = choose_at(d, ties=(name == "lattice"), need_zero=need_zero)
    out = [("at", at), ("below", float(np.nextafter(F32(at), F32(0)))), ("zero", 0.0)]
    if name in TIED:
        out.append(("tiny", TINY))
    for rname, r2 in out:       # the cap is a condition, not a measurement
        assert counts_of(d, r2).max() <= CAP, (name, rname, r2, int(counts_of(d, r2).max()))
    c = counts_of(d, at)
    assert ((c == 0).any() or not need_zero) and ((c >= 1) & (c <= 63)).any() and (leaving(d, at) > 0).any(), (name, at)
    return out


@functools.lru_cache(maxsize=None)
def radii(name, k):
    """[(rname, r2)] of the batch: at, below, zero and, for lattice and copies, tiny."""
    return _radii_of(batch(name, k)[2], name)


@functools.lru_cache(maxsize=None)
def own_radii(name, k):
    """The same from the window's own distances, the own row left out.  (Own rows sit inside their shard: on the lattice of 8
    dimensions every row has a neighbour one step away, so a count of zero is asked for only where some radius gives one.)"""
    d = window(name, k)[1]
    try:
        return _radii_of(d, name)
    except AssertionError:
        return _radii_of(d, name, need_zero=False)


def holder(d, at):
    """The first query with a row that holds `at` exactly."""
    return int(np.flatnonzero(leaving(d, at) > 0)[0])


def each_radii(rs, d, phase, m=M):
    """float32 [m]: a radius per query that cycles through (at, below, 0, NaN, -1) of the radii rs, the cycle placed so that the
    holder of `at` gets `at` (phase 0: radii[q] decides, or a cap below it) or `below` (phase 1: radii[q] alone drops the row)."""
    rs = dict(rs)
    cycle = np.array([rs["at"], rs["below"], 0.0, np.nan, -1.0], dtype=np.float32)
    return cycle[(np.arange(m) - holder(d, rs["at"]) + phase) % cycle.size]


@functools.lru_cache(maxsize=None)
def half_mask(name, k):
    """bool [N17]: a random half of the rows — with the first row that holds the batch's `at` radius exactly admitted, so that the
    boundary of the hit rule is met under the mask too."""
    bits = np.random.default_rng(seed_of(name, k) + 50).random(N17) < 0.5
    d = batch(name, k)[2]
    at = dict(radii(name, k))["at"]
    bits[np.flatnonzero(d[holder(d, at)] == F32(at))[0]] = True
    return _frozen(bits)


@functools.lru_cache(maxsize=None)
def one_per_run_mask(name, k):
    """bool [N17]: exactly one row — a random one — of every run of equal rows (a row without a copy is a run of one)."""
    R, _ = rows_and_queries(name, k)
    _, inverse = np.unique(R, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.random.default_rng(seed_of(name, k) + 51).permutation(N17)
    _, first = np.unique(inverse[order], return_index=True)        # the first of every run in a random order of the rows
    bits = np.zeros(N17, dtype=bool)
    bits[order[first]] = True
    return _frozen(bits)


def masks(name, k):
    """[(mname, bits)]: the random half and, for lattice and copies, one row of every run."""
    return [("half", half_mask(name, k))] + ([("one_per_run", one_per_run_mask(name, k))] if name in TIED else [])


@functools.lru_cache(maxsize=None)
def near(name, k, own=False):
    """(cols int64, d[:, cols], BASE + cols): the columns some query (own: some own row) has within the largest radius handed out.
    A row outside them is a hit of no query at any of the radii, so the suite's oracles, given these distances and these numbers
    as gids, answer what they answer on all N17 columns (tests/test_offcube_rows_logic.py compares the two) — in a fraction of
    the time."""
    d = window(name, k)[1] if own else batch(name, k)[2]
    rmax = max(r2 for _, r2 in (own_radii(name, k) if own else radii(name, k)))
    with np.errstate(invalid="ignore"):
        cols = np.flatnonzero((d <= F32(rmax)).any(axis=0))
    return _frozen(cols), _frozen(np.ascontiguousarray(d[:, cols])), _frozen(cols + BASE)
