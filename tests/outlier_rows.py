"""Rows with many out-of-box rows (test infrastructure, no GPU import): the shard, the queries and the oracle's distances the tests
of the out-of-box launches share — tests/test_outlier_rows_logic.py (CPU), tests/test_outlier_each_gpu.py,
tests/test_outlier_self_gpu.py, tests/test_outlier_blocks_gpu.py.

N17 rows: a tight cluster, 0.45 + 0.1 * random in every coordinate, and ONE contiguous block of P = 640 planted rows (3 blocks of
256 threads, 10 waves of the outlier kernels) from row PLANT_FIRST (no multiple of 64).  A planted row is uniform over
[0.46, 0.54] ([0.47, 0.53] at k = 8) in coordinates 1 .. k - 1 and over [1.48, 1.5] in coordinate 0.  Why there: the filter judges a row by
|x - centre| * sigma <= 1 per coordinate, sigma a power of two with 1 / sigma in [h, 2 h), h the robust box's widest half-width
(at most 12 * 1.4826 * MAD = 0.445 here, so 1 / sigma <= 0.5), and centre within the robust box (below 0.945): a coordinate above
1.445 is outside whichever frame maker built the box, one in [0.98, 1] is inside most of them.  And why a small cloud, not the
unit box: one call has ONE cap, so the "held" radii of queries beside planted rows and of queries inside the cluster must be of
one size (or an "inf" radius under the cap holds the whole cluster and the pass falls back), and a radius that holds 300 planted
rows must stay clear of the cluster (distance^2 >= 0.86 from any planted row) — the cloud is about as dense as the cluster.

Planted rows come in pairs (PLANT_FIRST + 2 i, + 2 i + 1): the second is the first plus 1e-3 * random, every eighth pair an exact
copy (distance 0).  So a planted row's near neighbours are planted rows, and at a list-sized radius every hit of a query beside one
comes from the out-of-box launch.

Expectations: tests.topk_oracle.v0_dist2 for queries, tests.self_oracle.self_dist2 for own rows — the plain oracles in v0's
operation order.  Everything here is made once per dimension; the rows and the distances are handed out read-only."""
import functools

import numpy as np

from tests.self_oracle import self_dist2
from tests.topk_oracle import v0_dist2

N17 = (1 << 17) + 999               # tests/test_within_cells_gpu.py's: the smallest shard that gets a cell-sorted layout
P = 640                             # planted rows: 3 blocks of KNN_BLOCK = 256, 10 waves
PLANT_FIRST = 3021                  # 3021 % 64 == 13
PLANT_END = PLANT_FIRST + P
BASE = 11                           # base_index of every index built on these rows
M_EACH = 96                         # a batch of queries: the first 64 beside planted rows, 32 in the cluster
M_BESIDE = 64
# own-row windows of the self tests
INSIDE_FIRST, WINDOW = PLANT_FIRST + 37, 96     # 3058 % 64 == 50: starts inside a block of 64, lies inside the planted block
STRADDLE_FIRST = PLANT_END - 48                 # 48 planted rows, then 48 rows of the cluster
PASS = 1024                                     # KNN_CELL_BATCH: the queries of one pass
TWO_PASS_FIRST = PLANT_FIRST + 100 - PASS       # the second pass's 96 own rows are PLANT_FIRST + 100 .. + 195: planted

assert PLANT_FIRST % 64 and INSIDE_FIRST % 64 and PLANT_FIRST <= TWO_PASS_FIRST + PASS and TWO_PASS_FIRST + PASS + WINDOW <= PLANT_END


def _frozen(a):
    a.setflags(write=False)
    return a


def planted_range():
    return PLANT_FIRST, PLANT_END


def is_planted(rows):
    rows = np.asarray(rows)
    return (rows >= PLANT_FIRST) & (rows < PLANT_END)


def copy_rows():
    """The rows of the exact-copy pairs (every eighth pair): each has its twin, row ^ 1 relative to PLANT_FIRST, at distance 0."""
    i = np.arange(0, P // 2, 8)
    return np.sort(np.concatenate([PLANT_FIRST + 2 * i, PLANT_FIRST + 2 * i + 1]))


def twin_of(row):
    return PLANT_FIRST + ((row - PLANT_FIRST) ^ 1)


def cloud_width(k):
    """The planted cloud's width in coordinates 1 .. k - 1: about the cluster's density (640 against 131 431 rows) in k dimensions."""
    return 0.08 if k > 8 else 0.06


@functools.lru_cache(maxsize=None)
def rows(k):
    """R float32 [N17][k], read-only."""
    rng = np.random.default_rng(N17 + 7 * k)
    R = (0.45 + 0.1 * rng.random((N17, k))).astype(np.float32)
    half = P // 2
    w = cloud_width(k)
    a = (0.5 - 0.5 * w + w * rng.random((half, k))).astype(np.float32)
    a[:, 0] = (1.48 + 0.02 * rng.random(half)).astype(np.float32)
    b = (a + np.float32(1e-3) * rng.random((half, k), dtype=np.float32)).astype(np.float32)
    b[::8] = a[::8]
    R[PLANT_FIRST:PLANT_END:2] = a
    R[PLANT_FIRST + 1:PLANT_END:2] = b
    return _frozen(R)


def spread_queries(rng, m, k, reach=0.6):
    """tests/test_within_cells_gpu.py's queries (restated here: this module imports no GPU test): inside the unit box and, one after
    the other, up to `reach` outside it along the first axis."""
    Q = rng.random((m, k), dtype=np.float32)
    Q[:, 0] += np.linspace(0.0, reach, m, dtype=np.float32)
    return Q


def _queries(k, m, beside, seed, lo=0, hi=P):
    rng = np.random.default_rng(seed)
    R = rows(k)
    at = PLANT_FIRST + lo + rng.choice(hi - lo, beside, replace=False)
    Qb = (R[at] + np.float32(1e-3) * rng.random((beside, k), dtype=np.float32)).astype(np.float32)
    Qc = (np.float32(0.45) + np.float32(0.1) * spread_queries(rng, m - beside, k)).astype(np.float32)
    return np.concatenate([Qb, Qc]) if m > beside else Qb


@functools.lru_cache(maxsize=None)
def each_batch(k):
    """(Q [96][k], d [96][N17]): 64 queries beside planted rows (row + 1e-3 * random), then 32 spread_queries scaled into the
    cluster (and up to 0.06 beyond it along the first axis)."""
    Q = _queries(k, M_EACH, M_BESIDE, 1000 + k)
    return Q, _frozen(v0_dist2(Q, rows(k), k))


@functools.lru_cache(maxsize=None)
def two_pass_batches(k):
    """(Q1 [64][k], d1, Q2 [96][k], d2): the first pass repeats Q1 (each_batch's first 32 beside planted rows and its 32 in the
    cluster) 16 times, the second pass's 96 queries all sit beside planted rows."""
    Q, d = each_batch(k)
    pick = np.concatenate([np.arange(32), np.arange(M_BESIDE, M_EACH)])
    Q2 = _queries(k, 96, 96, 2000 + k)
    return Q[pick].copy(), _frozen(d[pick].copy()), Q2, _frozen(v0_dist2(Q2, rows(k), k))


@functools.lru_cache(maxsize=None)
def own_dist2(k, first, count):
    """self_dist2 of the own rows first .. first + count - 1 (NaN where a row meets itself), read-only."""
    return _frozen(self_dist2(rows(k), k, first, count))


@functools.lru_cache(maxsize=None)
def centre_batch(k, m=24):
    """(Q [m][k], d): queries in the middle of the planted block's bounding region — coordinate 0 at 1.49, the others at 0.5 plus a
    jitter that grows with the query number (none for query 0, +-0.15 for the last): the first hold hundreds of planted rows
    within a radius that the last hold none in."""
    rng = np.random.default_rng(3000 + k)
    Q = np.full((m, k), 0.5, dtype=np.float32)
    Q[:, 0] = 1.49
    Q[:, 1:] += ((rng.random((m, k - 1)) - 0.5) * np.linspace(0.0, 0.3, m)[:, None]).astype(np.float32)
    return Q, _frozen(v0_dist2(Q, rows(k), k))


def blocks_radius(k):
    """The distance of centre_batch's query 0 to its 320th nearest row: half the planted block, and no row of the cluster."""
    return float(np.sort(centre_batch(k)[1][0])[P // 2 - 1])


def low_cap(r, kinds=9):
    """A cap below some queries' radii: the median of the "held" ones (kind 0 of tests.each_oracle.KINDS, first_kind 0)."""
    return float(np.median(r[0::kinds]))


def bound_of(r, cap):
    """float32 [m]: what a row's distance is compared with — min(r, cap), and -1 (no hit) for a NaN radius."""
    r = np.asarray(r, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(r), np.float32(-1), np.where(r <= np.float32(cap), r, np.float32(cap))).astype(np.float32)


def planted_hits(d, r2):
    """uint32 [m]: planted rows with a finite distance <= float32(r2) (a scalar or one per query)."""
    d = np.asarray(d, dtype=np.float32)
    r = np.broadcast_to(np.asarray(r2, dtype=np.float32).reshape(-1, 1), (d.shape[0], 1))
    with np.errstate(invalid="ignore"):
        return (d[:, PLANT_FIRST:PLANT_END] <= r).sum(axis=1).astype(np.uint32)


def kind_max(r, kind, kinds, first_kind=0):
    """The largest radius of one kind among tests.each_oracle.radii_of's r."""
    return float(r[(kinds.index(kind) - first_kind) % len(kinds)::len(kinds)].max())
