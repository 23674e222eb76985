"""knn_index_self_cluster_within — the shards of tests/test_cluster_forms_gpu.py, test_cluster_grid_walks_gpu.py and
test_cluster_streams_gpu.py (test infrastructure; numpy only, nothing here touches a GPU): what each is for, its radius and min_pts, and the grid a shard of
k <= 4 gets.  tests/test_cluster_rows_logic.py proves without a GPU that every shard is what its GPU test takes it for.  Every
maker is cached and returns READ-ONLY arrays; expectations always come from tests/cluster_oracle.py (want_sheet, want).

  sheet(k)            the exact way's forms, 7 <= k: a 2-D sheet — a uniform half and four gaussian blobs — mapped into k dimensions
                      by a random 2 x k matrix with unit rows, plus a little noise in every coordinate: the distances are sums of k
                      rounded terms (the lattice rows of tests/test_cluster_exact_gpu.py round nothing), the planted block of
                      tests/cluster_helper.py in the middle of the row order.  n = 1300: n % 64 = 20, the core kernel's last wave
                      stores ONE word.  max_dist2 1.0, min_pts 5.
  the grid shards     N = 16384 + 7 rows unless said; (radius, min_pts) in GRID:
    uniform_planted(k)  tests/test_cluster_grid_gpu.py's recipe at k = 2 and 4 (KD 2 and KD 4 of the grid link kernel);
    gradient()          k 3, uniform with coordinate 0 squared: the radius spans 4 rings, the densities 30 to 1, one component of
                        most core rows — the walk past ring 1 under the plain ring limit, and contention on one root;
    column()            k 3, a thin column (axes 1 and 2 times 2^-10): the radius spans 10 rings — past the plain limit 6, inside
                        the 2^15-cell budget, so the plan's rmax is the radius' own ring count — and most components hang on
                        single links;
    blobs()             k 3, 16 gaussian blobs and a uniform tenth: cells of hundreds of rows;
    offset()            k 2, rows in [4096, 4097): the box far from the origin;
    dead_axis()         k 3, coordinate 1 constant: a grid with one cell along that axis;
    strip()             k 2, n = 65536 + 70, axis 1 times 2^-10: the radius spans 149 rings, the batch gives up, and the gated
                        exact sweeps run in TWO chunks of rows."""
import functools

import numpy as np

from tests import cluster_oracle as co
from tests.cluster_helper import planted

N = 16384 + 7
CHUNK = 65536
SHEET_N, SHEET_OFF, SHEET_CAP, SHEET_MIN_PTS = 1300, 500, 1.0, 5
SHEET_KS = (7, 16, 17, 48, 49, 80, 81, 112, 113, 128, 129, 200)       # KC 1 partial, 1, 2, 3, 4, 5, 6, 7, 8 partial, 8, 0, 0
PLANTED_OFF = 9000
PLANTED_SHAPE = {2: (2.0 ** -7, 4), 4: (2.0 ** -4, 4)}
# name -> (radius, min_pts); the call's max_dist2 is radius * radius
GRID = {"uniform_planted2": PLANTED_SHAPE[2], "uniform_planted4": PLANTED_SHAPE[4], "gradient": (2.0 ** -3, 100),
        "column": (2.0 ** -11, 8), "blobs": (2.0 ** -8, 5), "offset": (2.0 ** -7, 4), "dead_axis": (2.0 ** -7, 4),
        "strip": (2.0 ** -10, 120)}


def _ro(a):
    a.setflags(write=False)
    return a


def _ro_names(names):
    return {key: _ro(np.asarray(rows)) for key, rows in names.items()}


@functools.lru_cache(maxsize=None)
def sheet(k, n=SHEET_N):
    """(R float32 [n][k], names, off): see the module's text; seed 5200 + k."""
    rng = np.random.default_rng(5200 + k)
    P, names, _ = planted(k, 1.0, 0.0, 0.0, rng)
    nb = n - len(P)
    half = nb // 2
    flat = 30.0 * rng.random((half, 2))
    centres = 3.0 + np.arange(4)[:, None] * np.array([7.0, 5.0])
    lumps = centres[rng.integers(0, 4, size=nb - half)] + 1.2 * rng.standard_normal((nb - half, 2))
    S = np.concatenate([flat, lumps])
    rng.shuffle(S, axis=0)
    M = rng.standard_normal((2, k))
    M /= np.linalg.norm(M, axis=1, keepdims=True)
    B = (S @ M + rng.standard_normal((nb, k)) * (0.15 / np.sqrt(k))).astype(np.float32)
    B[:, 0] -= np.float32(200.0)                                          # clear of the planted block, which starts at the origin
    R = np.concatenate([B[:SHEET_OFF], P, B[SHEET_OFF:]])
    assert R.shape == (n, k) and R.dtype == np.float32
    return _ro(R), _ro_names(names), SHEET_OFF


@functools.lru_cache(maxsize=None)
def uniform_planted(k):
    """(R float32 [N][k], names, off): tests/test_cluster_grid_gpu.py's shard — uniform rows in the unit cube and, a quarter beyond
    it along axis 0, the planted block in units of the radius."""
    r, _ = PLANTED_SHAPE[k]
    rng = np.random.default_rng(4400 + k)
    P, names, end = planted(k, r, 1.25, 0.5, rng)
    U = rng.random((N - len(P), k), dtype=np.float32)
    R = np.concatenate([U[:PLANTED_OFF], P, U[PLANTED_OFF:]])
    assert R.shape == (N, k) and end < 8.0
    return _ro(R), _ro_names(names), PLANTED_OFF


@functools.lru_cache(maxsize=None)
def gradient():
    R = np.random.default_rng(4600).random((N, 3), dtype=np.float32)
    R[:, 0] *= R[:, 0]
    return _ro(R)


@functools.lru_cache(maxsize=None)
def column():
    """tests/test_cluster_grid_gpu.py's give-up cloud without its far row."""
    R = np.random.default_rng(4700).random((N, 3), dtype=np.float32)
    R[:, 1:] *= np.float32(2.0 ** -10)
    return _ro(R)


@functools.lru_cache(maxsize=None)
def blobs():
    rng = np.random.default_rng(4800)
    centres = 0.1 + 0.8 * rng.random((16, 3))
    nb = N * 9 // 10
    B = centres[rng.integers(0, 16, size=nb)] + 0.01 * rng.standard_normal((nb, 3))
    R = np.concatenate([B, rng.random((N - nb, 3))]).astype(np.float32)
    rng.shuffle(R, axis=0)
    return _ro(R)


@functools.lru_cache(maxsize=None)
def offset():
    return _ro((4096.0 + np.random.default_rng(4900).random((N, 2))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def dead_axis():
    R = np.random.default_rng(4950).random((N, 3), dtype=np.float32)
    R[:, 1] = np.float32(0.375)
    return _ro(R)


@functools.lru_cache(maxsize=None)
def strip():
    R = np.random.default_rng(5000).random((CHUNK + 70, 2), dtype=np.float32)
    R[:, 1] *= np.float32(2.0 ** -10)
    return _ro(R)


def rows_of(name):
    """The rows of the grid shard `name` (a key of GRID)."""
    if name.startswith("uniform_planted"):
        return uniform_planted(int(name[-1]))[0]
    return {"gradient": gradient, "column": column, "blobs": blobs, "offset": offset, "dead_axis": dead_axis, "strip": strip}[name]()


def _frozen(w):
    return {key: _ro(np.asarray(v)) for key, v in w.items()}


@functools.lru_cache(maxsize=None)
def want(name, max_dist2=None, min_pts=None):
    """The oracle's answer on the grid shard `name`, at GRID's radius and min_pts unless given.  Computed once, read-only."""
    R = rows_of(name)
    r, mp = GRID[name]
    return _frozen(co.cluster(R, R.shape[1], r * r if max_dist2 is None else max_dist2, mp if min_pts is None else min_pts))


@functools.lru_cache(maxsize=None)
def want_sheet(k, max_dist2=SHEET_CAP, min_pts=SHEET_MIN_PTS):
    return _frozen(co.cluster(sheet(k)[0], k, max_dist2, min_pts))


def shares(w):
    """(core, border, noise) as fractions of the rows."""
    return float(w["core"].mean()), float(w["border"].mean()), float((w["labels"] < 0).mean())


def largest_cluster(labels):
    lab = np.asarray(labels)
    return int(np.bincount(lab[lab >= 0]).max()) if (lab >= 0).any() else 0


def spanning(labels, at=CHUNK):
    """The clusters with rows on both sides of row `at`."""
    lab = np.asarray(labels)
    lo, hi = np.unique(lab[:at][lab[:at] >= 0]), np.unique(lab[at:][lab[at:] >= 0])
    return np.intersect1d(lo, hi)


@functools.lru_cache(maxsize=None)
def held_radius(k):
    """(row, E4, below): a row of sheet(k) — outside the planted block — whose fourth-nearest other row lies at E4 in (0.9, 1.0),
    and the next float below E4.  At max_dist2 = E4 the row has deg >= 4 and is core under min_pts 5; at `below` it has deg 3 and
    is not (unless a fifth row ties E4, which the pick rules out).  By the oracle's distances alone."""
    from tests.topk_oracle import v0_dist2
    R, names, off = sheet(k)
    n = R.shape[0]
    plen = sum(len(names[s]) for s in ("chain down", "chain mixed", "bridge", "copies", "two copies", "touching", "apart"))
    for i in list(range(off)) + list(range(off + plen, n)):
        d = v0_dist2(R[i:i + 1], R, k)[0]
        d[i] = np.float32(np.inf)
        s = np.sort(d)
        if np.float32(0.9) < s[3] < np.float32(1.0) and s[2] < s[3] < s[4]:
            return i, float(s[3]), float(np.nextafter(s[3], np.float32(0)))
    raise AssertionError("no row of sheet(%d) has its fourth-nearest row in (0.9, 1.0)" % k)


def grid_shape(R, radius):
    """knn_grid_build's arithmetic restated in float64, so that a test can say what its shard is — it never decides a pair:
    dict(live, g, widths [k] (1.0 on a dead axis), cells, max_cell, rings).  rings is knn_grid_radius_rings: ceil(radius /
    the narrowest live width) + 1."""
    R = np.asarray(R, dtype=np.float32)
    n, k = R.shape
    lo, hi = R.min(axis=0).astype(np.float64), R.max(axis=0).astype(np.float64)
    alive = hi > lo
    live = int(alive.sum())
    assert 1 <= k <= 4 and live >= 1
    g = int(np.floor((n / 3.0) ** (1.0 / live)))
    g = min(max(g, 1), {1: 1 << 19, 2: 2048, 3: 160, 4: 45}[live])
    per_axis = np.where(alive, g, 1)
    widths = np.where(alive, (hi - lo) / per_axis, 1.0)
    cell = np.zeros(n, dtype=np.int64)
    stride = 1
    for d in range(k):
        if alive[d]:
            c = np.clip(np.floor((R[:, d].astype(np.float64) - lo[d]) * (g / (hi[d] - lo[d]))).astype(np.int64), 0, g - 1)
            cell += c * stride
        stride *= int(per_axis[d])
    rings = int(np.ceil(radius / widths[alive].min()) + 1.0)
    return dict(live=live, g=g, widths=widths, cells=stride, max_cell=int(np.bincount(cell).max()), rings=rings)
