"""numpy restatement of knn_index_count_within (test infrastructure): how many rows lie within a radius of each query.

count = ((d < inf) & (d <= float32(r2))).sum(axis=1) on tests.topk_oracle.v0_dist2 — v0's fp32 distance, a finite-distance test and
an fp32 compare with equality inside.  Also the radii a test runs, taken from the oracle's own distances, and the CPU-side checks
that a batch proves what it claims: its expected counts hold a zero, a value in 1 .. 63 and, at the large radius, a value above 64
(more than any top-K list can say)."""
import numpy as np

from tests.topk_oracle import v0_dist2

INF = np.float32(np.inf)


def counts_of(d, r2):
    """uint32 [m]: rows of the distance matrix d [m][n] (float32) that are finite and <= float32(r2)."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return ((d < INF) & (d <= np.float32(r2))).sum(axis=1).astype(np.uint32)


def counts(Q, R, k, r2, chunk=64):
    """uint32 [m] from the rows themselves, `chunk` queries at a time (no [m][n] matrix is kept)."""
    Q = np.asarray(Q, dtype=np.float32).reshape(-1, k)
    return np.concatenate([counts_of(v0_dist2(Q[c0:c0 + chunk], R, k), r2) for c0 in range(0, Q.shape[0], chunk)])


def kinds(d, r2):
    """(some count is 0, some is in 1 .. 63, some is above 64) at this radius."""
    c = counts_of(d, r2)
    return bool((c == 0).any()), bool(((c >= 1) & (c <= 63)).any()), bool((c > 64).any())


def radii(d, near=8, large=100):
    """The radii a test runs, from the oracle's distances d [m][n]: a value some row holds exactly (`at`: the boundary is inside),
    the next float below it (`below`: that row outside), 0, +INF, one below every distance, and one `large` radius at which some
    query's count exceeds 64 — the smallest `large`-th nearest distance among the queries.  `at` is the `near`-th nearest distance
    of some query, picked from the median outwards so that at `at` AND at `below` the expected counts hold a zero and a value in
    1 .. 63; asserted here, on the CPU: a count that is wrong for one kind must not hide behind a batch that has none of it."""
    d = np.asarray(d, dtype=np.float32)
    assert d.shape[1] > large > 64 > near
    fin = np.where(d < INF, d, INF)
    part = np.sort(np.partition(fin, large - 1, axis=1)[:, :large], axis=1)
    held = np.unique(part[:, near - 1][part[:, near - 1] < INF])
    assert held.size, "no query has `near` finite distances"
    order = np.argsort(np.abs(np.arange(held.size) - held.size // 2), kind="stable")
    at = None
    for v in held[order]:
        below = np.nextafter(v, np.float32(0))
        if all(z and p for z, p, _ in (kinds(d, v), kinds(d, below))) and (counts_of(d, v) != counts_of(d, below)).any():
            at = v
            break
    assert at is not None, "no radius gives a zero and a value in 1 .. 63 among the queries' counts: change the batch"
    least = fin.min()
    assert 0 < least < INF, "a query coincides with a row (or none has a finite distance): no radius is below every distance"
    under = np.float32(least * np.float32(0.5))
    assert (counts_of(d, under) == 0).all()
    big = part[:, large - 1].min()
    assert big < INF and kinds(d, big)[2], "no query has more than 64 rows within the large radius"
    return [("at", float(at)), ("below", float(np.nextafter(at, np.float32(0)))), ("zero", 0.0), ("inf", float("inf")),
            ("under_all", float(under)), ("large", float(big))]
