"""numpy restatement of the calls with a radius per query (test infrastructure; include/knn_mi355x.h 2j), the radii their GPU tests
use, and the CPU-side checks that a batch proves what it claims.

A row is a hit for query j when d = tests.topk_oracle.v0_dist2 is finite, d <= r[j] and d <= cap (float32 compares; a NaN or
negative radius admits nothing).  Radii are made from the oracle's own distances and cycle through KINDS, so that every 64
consecutive queries hold every kind."""
import numpy as np

from tests.list_oracle import lengths

INF = np.float32(np.inf)
F32 = np.float32
KINDS = ("held", "below", "zero", "minus_zero", "inf", "nan", "minus_one", "half_least", "many")
HELD_RANK, MANY_RANK = 5, 80        # "held": the 5th smallest finite distance (1 .. 63 hits); "many": the 80th (> 64 hits)


def hits_of(d, r, cap=INF):
    d = np.asarray(d, dtype=np.float32)
    r = np.asarray(r, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (d < INF) & (d <= r[:, None]) & (d <= np.float32(cap))


def counts_of(d, r, cap=INF):
    return hits_of(d, r, cap).sum(axis=1).astype(np.uint32)


def lists_of(d, r, cap=INF, gids=None, base=0):
    """[m] arrays of uint64: every query's hits as packed keys (distance bits << 32 | global number), ascending."""
    d = np.asarray(d, dtype=np.float32)
    n = d.shape[1]
    g = (np.arange(n, dtype=np.uint64) + np.uint64(base)) if gids is None else np.asarray(gids).astype(np.uint64)
    hit = hits_of(d, r, cap)
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | g[None, :]
    return [np.sort(keys[j][hit[j]]) for j in range(d.shape[0])]


def radii_of(d, first_kind=0, kinds=KINDS):
    """float32 [m]: query j's radius is of kind kinds[(first_kind + j) % len(kinds)], made from row j of d (needs >= MANY_RANK
    finite distances per row that has any)."""
    d = np.asarray(d, dtype=np.float32)
    m = d.shape[0]
    r = np.empty(m, dtype=np.float32)
    for j in range(m):
        fin = np.sort(d[j][d[j] < INF])
        kind = kinds[(first_kind + j) % len(kinds)]
        if fin.size == 0:             # a non-finite query: any radius, no hit
            fin = np.ones(MANY_RANK, dtype=np.float32)
        held = fin[min(HELD_RANK, fin.size) - 1]
        r[j] = {"held": held, "below": np.nextafter(held, F32(0)), "zero": F32(0), "minus_zero": F32(-0.0), "inf": INF,
                "nan": F32(np.nan), "minus_one": F32(-1), "half_least": F32(0.5) * fin[0],
                "many": fin[min(MANY_RANK, fin.size) - 1]}[kind]
    return r


def assert_every_kind_of_count(counts):
    """The expected counts hold a zero, a value in 1 .. 63 and a value above 64."""
    c = np.asarray(counts)
    assert (c == 0).any() and ((c >= 1) & (c <= 63)).any() and (c > 64).any(), c


def assert_no_shared_radius_passes(d, r, cap=INF):
    """In every group of 64 consecutive queries (the groups a wave or a block holds, and the last 64) at least two queries would
    get a different count under each other's radius: a kernel that reads one radius per wave or per block cannot pass."""
    m = d.shape[0]
    own = counts_of(d, r, cap)
    starts = sorted(set(list(range(0, max(m - 63, 1), 64)) + [max(m - 64, 0)]))
    for g0 in starts:
        idx = np.arange(g0, min(g0 + 64, m))
        found = False
        for a in idx:
            under = counts_of(d[idx], np.full(idx.size, r[a], np.float32), cap)     # the group under a's radius
            back = counts_of(d[a:a + 1].repeat(idx.size, axis=0), r[idx], cap)        # a under the others' radii
            if ((under != own[idx]) & (back != own[a])).any():
                found = True
                break
        assert found, g0


def assert_a_stale_pointer_fails(d_second, r_second, r_first, cap=INF):
    """Query j of the second chunk (or pass) would get a different count under the radius of query j of the first: a launch that
    forgets to advance the radii pointer cannot pass."""
    m = d_second.shape[0]
    assert (counts_of(d_second, r_first[:m], cap) != counts_of(d_second, r_second, cap)).any()


__all__ = ["KINDS", "hits_of", "counts_of", "lists_of", "lengths", "radii_of", "assert_every_kind_of_count",
           "assert_no_shared_radius_passes", "assert_a_stale_pointer_fails"]
