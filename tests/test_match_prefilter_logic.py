"""The match kernel's queue test against its list test, on the CPU (knn_debug_match_tests runs the kernel's own two lines,
knn_cell_queued and knn_cell_listed of knn_common.h).

A block of the match kernel owns 64 cells: one high-table entry and 64 consecutive low-table entries.  Its pass 1 queues a query
iff !(hi + min_l lo[l] > Dup) in fp32; its pass 2 lists the query for cell l iff !(lo[l] + hi > Dup).  fp32 addition does not
decrease when an operand grows, so the queue is exactly the union of the 64 lists: nothing a cell would list is left out, and
nothing is queued that no cell lists.  The cases below are made to sit on that edge: sums one rounding away from Dup, denormal
entries, +INF entries, Dup = 0, Dup = +INF and the padding queries' Dup = -INF."""
import numpy as np
import pytest

import multicore_hw2_amd as pkg

F = np.float32
DENORM = np.array([0.0, 1e-45, 3e-42, 1.1754942e-38, 1.17549435e-38], dtype=F)   # zero, smallest denormals, around the smallest normal


def _cases(rng, n, scale):
    """lo[n][64], hi[n], dup[n]: non-negative tables as the prep kernel writes them (rounded-down sums of squared gaps)."""
    lo = (rng.random((n, 64)) ** 3 * scale).astype(F)
    hi = (rng.random(n) ** 3 * scale).astype(F)
    lo[rng.random((n, 64)) < 0.02] = 0.0                                 # the query's own bin: gap 0
    inf = rng.random((n, 64)) < 0.05
    lo[inf] = np.inf
    lo[rng.random(n) < 0.02] = np.inf                                    # a block nothing of which is reachable
    den = rng.random((n, 64)) < 0.02
    lo[den] = rng.choice(DENORM, size=int(den.sum()))
    hi[rng.random(n) < 0.1] = 0.0
    hi[rng.random(n) < 0.05] = rng.choice(DENORM, size=1)[0]
    hi[rng.random(n) < 0.02] = np.inf
    # Dup on the edge: the rounded sum of one of the 64 entries, or the float next to it on either side
    j = rng.integers(0, 64, size=n)
    with np.errstate(invalid="ignore", over="ignore"):
        edge = (lo[np.arange(n), j] + hi).astype(F)
    kind = rng.integers(0, 8, size=n)
    dup = (rng.random(n) * F(scale)).astype(F)
    dup = np.where(kind == 0, edge, dup)
    dup = np.where(kind == 1, np.nextafter(edge, F(-np.inf)), dup)
    dup = np.where(kind == 2, np.nextafter(edge, F(np.inf)), dup)
    dup = np.where(kind == 3, F(0.0), dup)
    dup = np.where((kind == 4) & (rng.random(n) < 0.2), F(np.inf), dup)
    dup = np.where((kind == 4) & (rng.random(n) < 0.2), F(-np.inf), dup)      # a padding query: never queued, never listed
    dup = np.where((kind == 5) & (rng.random(n) < 0.5), rng.choice(DENORM, size=n), dup)
    return lo, hi, np.ascontiguousarray(dup, dtype=F)


@pytest.mark.parametrize("scale", [1.0, 1e-38, 3e38, 2.0 ** 24], ids=["unit", "denormal", "near_overflow", "2p24"])
def test_queue_is_the_union_of_the_lists(scale):
    rng = np.random.default_rng(20260 + int(np.log2(scale)))
    lo, hi, dup = _cases(rng, 20000, scale)
    queued, listed = pkg.debug_match_tests(lo, hi, dup)
    # the two tests restated in numpy's fp32, one rounding per sum
    with np.errstate(invalid="ignore", over="ignore"):
        want_listed = (~((lo + hi[:, None]).astype(F) > dup[:, None])).sum(axis=1)
        want_queued = ~((lo.min(axis=1) + hi).astype(F) > dup)
    assert (listed == want_listed).all()
    assert (queued == want_queued).all()
    # what the change rests on
    assert (queued == (listed > 0)).all(), np.flatnonzero(queued != (listed > 0))[:8]
    # the cases do sit on both sides, and a good share of the queued ones is listed by few cells only
    assert 0.2 < queued.mean() < 0.9 and (listed[queued] < 8).mean() > 0.05
    assert not queued[dup == -np.inf].any()
    assert queued[dup == np.inf].all()


def test_queue_on_the_high_table_alone_is_a_superset():
    """The queue test on the high table alone, !(hi > Dup), takes everything the test on the group minimum takes (low entries
    are >= 0): it was the complete, but longer, queue."""
    rng = np.random.default_rng(7)
    lo, hi, dup = _cases(rng, 20000, 1.0)
    queued, _ = pkg.debug_match_tests(lo, hi, dup)
    assert (~(hi > dup))[queued].all()


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        pkg.debug_match_tests(np.zeros((3, 63), F), np.zeros(3, F), np.zeros(3, F))
    assert pkg.lib().knn_debug_match_tests(1, None, None, None, None, None) != 0
