"""numpy restatement of knn_index_list_within (test infrastructure): which rows lie within a radius of each query.

The expected list of a query is the sorted packed keys — (float bits of d << 32) | global number — of the rows that
tests/count_oracle.counts_of counts: d = tests.topk_oracle.v0_dist2 finite and d <= float32(r2).  Also the segments a test hands
the call (exclusive 64-bit prefix sums of counts) and the CPU-side check that a batch proves what it claims: an empty list, one of
1 .. 63 entries and one above 64."""
import numpy as np

INF = np.float32(np.inf)


def lists_of(d, r2, gids=None, base=0):
    """[m] arrays of uint64: every query's hits as packed keys, ascending.  gids[row] (or base + row) is a row's global number."""
    d = np.asarray(d, dtype=np.float32)
    n = d.shape[1]
    g = (np.arange(n, dtype=np.uint64) + np.uint64(base)) if gids is None else np.asarray(gids).astype(np.uint64)
    with np.errstate(invalid="ignore"):
        hit = (d < INF) & (d <= np.float32(r2))
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | g[None, :]
    return [np.sort(keys[j][hit[j]]) for j in range(d.shape[0])]


def lengths(lists):
    return np.array([len(x) for x in lists], dtype=np.uint32)


def offsets_of(counts):
    """uint64 [m + 1]: offsets[0] = 0, offsets[j + 1] = offsets[j] + counts[j]."""
    out = np.zeros(len(counts) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts).astype(np.uint64), out=out[1:])
    return out


def kinds(lists):
    """(some list is empty, some has 1 .. 63 entries, some has more than 64)."""
    c = lengths(lists)
    return bool((c == 0).any()), bool(((c >= 1) & (c <= 63)).any()), bool((c > 64).any())


def holds_every_kind(batches):
    """True when, over the given batches of lists together, there is an empty list, one of 1 .. 63 entries and one above 64."""
    k = np.array([kinds(b) for b in batches])
    return bool(k.any(axis=0).all())
