"""knn_index_self_cluster_within_routed — the shards of tests/test_cluster_routed_cells_gpu.py (test infrastructure; numpy only,
nothing here touches a GPU).  tests/test_cluster_routed_logic.py proves without a GPU that every shard is what its GPU test takes
it for.  Every maker is cached and returns READ-ONLY arrays.

  N17                 2^17 + 999 rows: the smallest shard that gets a cell-sorted layout under `cells` 1; 128 passes of 1024 own rows
                      and a last one of 999.
  planted17(k)        uniform rows in the unit cube and the planted block of tests/cluster_helper.py beyond the cube along axis 0,
                      in units of the radius, in the MIDDLE of the row order from PLANTED_OFF on: it starts 50 rows ahead of row
                      64 * 1024, so the first chain straddles a pass boundary.  The radius is the power of two nearest the
                      shard's median 8th-neighbour distance (RADIUS: 0.270 -> 2^-2 at k 8, 0.700 -> 2^-1 at k 16, 0.891 -> 2^0 at k
                      20; test_cluster_routed_logic re-measures them).  The block starts X0[k] along axis 0: a quarter beyond the
                      cube as tests/cluster_rows.uniform_planted places it where the radius is a quarter, two radii beyond where
                      it is larger — no uniform row may come within the radius of a planted one.  Beyond the cube means outside
                      the layout's robust box: the planted rows are the layout's out-of-box rows.
  long_box()          k 8, uniform rows with axis 0 times 16: tests/cluster_oracle.py's pruning along axis 0 leaves about 5 % of the
                      rows per block, so the oracle finishes on the CPU.  max_dist2 is the median 7th-neighbour distance of the
                      first 512 rows — a median of 6 rows within it —, min_pts LONG_MIN_PTS."""
import functools

import numpy as np

from tests import cluster_oracle as co
from tests.cluster_helper import planted
from tests.topk_oracle import v0_dist2

N17 = (1 << 17) + 999
PASS = 1024
PLANTED_OFF = 64 * PASS - 50
RADIUS = {8: 2.0 ** -2, 16: 2.0 ** -1, 20: 2.0 ** 0}
X0 = {8: 1.25, 16: 2.0, 20: 3.0}
MIN_PTS = {8: 5, 16: 4, 20: 5}
LONG_K, LONG_STRETCH, LONG_KTH, LONG_MIN_PTS = 8, 16.0, 7, 8


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planted17(k):
    """(R float32 [N17][k], names, off, radius, min_pts)."""
    r = RADIUS[k]
    rng = np.random.default_rng(7100 + k)
    P, names, _ = planted(k, r, X0[k], 0.5, rng)
    U = rng.random((N17 - len(P), k), dtype=np.float32)
    R = np.concatenate([U[:PLANTED_OFF], P, U[PLANTED_OFF:]])
    assert R.shape == (N17, k) and R.dtype == np.float32
    return _ro(R), {key: _ro(np.asarray(v)) for key, v in names.items()}, PLANTED_OFF, r, MIN_PTS[k]


def planted_rows(names):
    return int(max(v.max() for v in names.values())) + 1


def kth_neighbour_dist2(R, k, rows, kth):
    """The v0 distance to the kth-nearest OTHER row, for each of `rows`."""
    d = v0_dist2(R[rows], R, k)
    d[np.arange(len(rows)), rows] = np.float32(np.inf)
    return np.partition(d, kth - 1, axis=1)[:, kth - 1]


@functools.lru_cache(maxsize=None)
def long_box():
    """(R float32 [N17][8], max_dist2)."""
    rng = np.random.default_rng(7300)
    R = rng.random((N17, LONG_K), dtype=np.float32)
    R[:, 0] *= np.float32(LONG_STRETCH)
    cap = float(np.median(kth_neighbour_dist2(R, LONG_K, np.arange(512), LONG_KTH)))
    return _ro(R), cap


@functools.lru_cache(maxsize=None)
def want_long_box():
    """The oracle's answer on the long box.  Computed once, read-only."""
    R, cap = long_box()
    return {key: _ro(np.asarray(v)) for key, v in co.cluster(R, LONG_K, cap, LONG_MIN_PTS).items()}


def fallback_rows(k=8):
    """(R, far, bad): uniform rows with one row at 1e6 in the LAST pass — knn_index_last_stats tells of the last pass that ran — and
    one with a NaN coordinate in a pass in the middle: two passes fall back, each on its own."""
    rng = np.random.default_rng(7500 + k)
    R = rng.random((N17, k), dtype=np.float32)
    far, bad = N17 - 700, 70 * PASS + 17
    R[far] = np.float32(1e6)
    R[bad, 3] = np.float32(np.nan)
    return R, far, bad
