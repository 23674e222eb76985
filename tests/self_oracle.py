"""numpy restatement of the queries about a shard's own rows (test infrastructure; include/knn_mi355x.h 2i): the K nearest OTHER
rows, the count of other rows within a radius and the sorted lists of them, for the queries that are rows row_first ..
row_first + rows - 1 of R.

Everything sits on tests.topk_oracle.v0_dist2: the distances of R[window] against all of R, with the entry of (j, row_first + j) —
the pair of a row with ITSELF, by row number — forced to NaN, "never a candidate".  Other copies of the row keep their distance 0.
From there the rules are the plain calls': a candidate has a finite distance <= float32(r2); keys are (distance bits << 32) | global
number; lists are ascending; top-K lists are padded with KEY_INIT."""
import numpy as np

from tests.count_oracle import counts_of
from tests.list_oracle import lists_of
from tests.topk_oracle import KEY_INIT, v0_dist2

INF = np.float32(np.inf)


def self_dist2(R, k, row_first, rows):
    """float32 [rows][n]: v0's distances of rows row_first .. row_first + rows - 1 to every row, NaN where a row meets itself."""
    R = np.asarray(R, dtype=np.float32).reshape(-1, k)
    d = v0_dist2(R[row_first:row_first + rows], R, k)
    d[np.arange(rows), row_first + np.arange(rows)] = np.nan
    return d


def self_lists(d, r2=INF, gids=None, base=0):
    """[rows] arrays of uint64 from self_dist2's matrix: every row's other rows within r2 as packed keys, ascending."""
    return lists_of(d, r2, gids=gids, base=base)


def self_counts(d, r2=INF):
    return counts_of(d, r2)


def self_topk(d, K, r2=INF, gids=None, base=0):
    """uint64 [rows][K] from self_dist2's matrix: the K smallest of self_lists, padded with KEY_INIT."""
    out = np.full((d.shape[0], K), KEY_INIT, dtype=np.uint64)
    for j, keys in enumerate(self_lists(d, r2, gids=gids, base=base)):
        t = min(K, keys.size)
        out[j, :t] = keys[:t]
    return out


def fold(a, b):
    """uint64 [m][K]: the K smallest of two sorted K-lists per row (what a folding call leaves)."""
    K = a.shape[1]
    return np.sort(np.concatenate([a, b], axis=1), axis=1)[:, :K]
