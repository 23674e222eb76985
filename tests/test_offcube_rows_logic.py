"""What the GPU tests of the radius family off the unit cube rest on (tests/test_offcube_within_gpu.py, test_offcube_each_gpu.py,
test_offcube_self_gpu.py, test_offcube_masked_gpu.py), asserted from the oracle alone on the batches of tests/offcube_rows.py: the
counts at `at` and `below` are of every kind, the lattice's radius is a tie among rows of several queries, `copies` has hits at
radius 0 and queries with none, `scaled` spans 2^10, no radius holds more than 64 rows, the masks bite, the per-query radii hold
every kind that applies, and a re-rank that is wrong in one of the ways it can be wrong — `<` for `<=`, the own row kept, the mask
not read — would change an expected answer.  Last, the host arithmetic of the radius cap (knn_debug_within_bound at u = +INF,
the count forms' case) on a row whose v0 sum rounded down at every addition.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests import offcube_rows as oc
from tests.count_oracle import counts_of
from tests.list_oracle import lists_of
from tests.masked_routed_helper import assert_mask_bites, want_of
from tests.test_within_logic import _exact_d2, _v0

CASES = [(name, k) for name in oc.NAMES for k in oc.KS]


def differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name,k", CASES)
def test_the_rows_and_queries_are_what_the_module_says(name, k):
    R, Q = oc.rows_and_queries(name, k)
    assert R.shape == (oc.N17, k) and Q.shape == (oc.M, k) and R.dtype == Q.dtype == np.float32
    assert np.isfinite(R).all() and np.isfinite(Q).all() and not R.flags.writeable and not Q.flags.writeable
    if name == "offset":
        assert R.min() >= 4096.0 and R.max() <= 4097.0
    elif name == "lattice":
        assert np.isin(R, [0.0, 0.25, 0.5, 0.75, 1.0]).all() and np.isin(Q * 4, np.arange(8)).all()
        assert (Q[::4, 0] >= 0.75).all() and (Q[:, 0] > 1.0).any() and (Q[:, 1:] <= 1.0).all()
    elif name == "scaled":
        s = oc.scales(k)
        assert s.max() / s.min() >= 2.0 ** 10 and s.max() <= 64.0 and s.min() >= 2.0 ** -6
        assert (np.log2(s) == np.round(np.log2(s))).all() and (R.max(axis=0) <= s).all() and (R.max(axis=0) > 0.99 * s).all()
    elif name == "copies":
        hit = (Q[:, None, :] == R[None, :4096, :]).all(axis=2)          # (the run is among the first rows: enough to see it)
        assert hit[oc.RUN_QUERY, oc.run_rows()].all()
    if name in oc.TIED:
        run = oc.run_rows()
        assert (R[run] == R[oc.WINDOW_FIRST]).all() and run[0] < oc.WINDOW_FIRST < run[-1] and (Q[oc.RUN_QUERY] == R[run[0]]).all()
        assert not (R[run[0] - 1] == R[run[0]]).all() and not (R[run[-1] + 1] == R[run[0]]).all()


@pytest.mark.parametrize("name,k", CASES)
def test_the_radii_give_every_kind_of_count_and_none_above_the_cap(name, k):
    _, _, d = oc.batch(name, k)
    rs = oc.radii(name, k)
    names = [r[0] for r in rs]
    assert names == ["at", "below", "zero"] + (["tiny"] if name in oc.TIED else [])
    r = dict(rs)
    at, below = np.float32(r["at"]), np.float32(r["below"])
    assert at > 0 and below == np.nextafter(at, np.float32(0)) and (d == at).any() and r["zero"] == 0.0
    c_at, c_below = counts_of(d, r["at"]), counts_of(d, r["below"])
    print(f"{name} k {k}: at {r['at']!r} largest count {c_at.max()}, {int((c_at == 0).sum())} queries with none, "
          f"{int((c_at != c_below).sum())} lose {int((c_at - c_below).max())} at most below it; "
          f"{int(counts_of(d, 0.0).sum())} pairs at distance 0")
    assert (c_at == 0).any() and ((c_at >= 1) & (c_at <= 63)).any()
    assert (c_at != c_below).any() and (c_below <= c_at).all()
    for rname, r2 in rs:
        assert counts_of(d, r2).max() <= oc.CAP, (rname, r2)
    # a `<` for the `<=` of the hit rule would answer `below` at `at`: a different list
    assert differ(lists_of(d, r["at"]), lists_of(d, r["below"]))
    zero = counts_of(d, 0.0)
    if name in oc.TIED:
        np.testing.assert_array_equal(counts_of(d, oc.TINY), zero)
        assert 0 < oc.TINY < 1e-44 and zero[oc.RUN_QUERY] >= oc.RUN
    if name == "lattice":
        gone = oc.leaving(d, r["at"])
        assert (gone > 0).sum() >= 2 and gone.max() >= 3, gone              # a tie among rows of several queries, three rows at once
    if name == "copies":
        assert (zero[0::2] >= 2).all() and (zero == 0).any() and zero.sum() >= 2 * (oc.M // 2)     # hits at radius 0, and queries with none
        assert (counts_of(d, r["at"]) > zero).any()
    if name not in oc.TIED:
        assert zero.sum() == 0


@pytest.mark.parametrize("name,k", CASES)
def test_the_masks_bite_and_the_per_query_radii_hold_every_kind(name, k):
    _, _, d = oc.batch(name, k)
    rs = oc.radii(name, k)
    at, below = dict(rs)["at"], dict(rs)["below"]
    ms = oc.masks(name, k)
    assert [m[0] for m in ms] == ["half"] + (["one_per_run"] if name in oc.TIED else [])
    for mname, bits in ms:
        assert bits.shape == (oc.N17,) and bits.dtype == bool
        assert_mask_bites(d, bits, at)
        # a re-rank that does not read the mask would answer the unmasked lists
        assert differ(want_of(d, bits, at)[1], lists_of(d, at)), mname
        # and a `<` for the `<=` would drop an ADMITTED row: the boundary is met under the mask too
        assert differ(want_of(d, bits, at)[1], want_of(d, bits, below)[1]), mname
    if name in oc.TIED:
        R, _ = oc.rows_and_queries(name, k)
        bits = oc.one_per_run_mask(name, k)
        assert bits[oc.run_rows()].sum() == 1
        kept = np.unique(R[bits], axis=0)
        assert kept.shape[0] == bits.sum() == np.unique(R, axis=0).shape[0]           # one row of every run, and every run
        masked = want_of(d, bits, 0.0)[0]
        assert masked[oc.RUN_QUERY] == 1 and (masked <= 1).all()          # at radius 0 a query's hits are ONE run: one row of it is left
    # radii per query: every kind that a list-sized cap leaves room for, the holder of `at` under `at` and under `below`
    h = oc.holder(d, at)
    dn = oc.near(name, k)[1]
    kinds = {"held": np.float32(at), "below": np.float32(below), "zero": np.float32(0), "minus_one": np.float32(-1)}
    assert set(oc.EACH_KINDS) <= set(eo.KINDS)
    for phase, mine in ((0, at), (1, below)):
        r = oc.each_radii(rs, d, phase)
        assert r.shape == (oc.M,) and r[h] == np.float32(mine)
        for kind in oc.EACH_KINDS:
            assert (np.isnan(r).sum() >= oc.M // 5) if kind == "nan" else ((r == kinds[kind]).sum() >= oc.M // 5), kind
        for cap in (at, below):         # (on the columns within `at`: test_the_near_columns_give_the_oracles_what_all_columns_give)
            eo.assert_no_shared_radius_passes(dn, r, cap)
            assert eo.counts_of(dn, r, cap).max() <= oc.CAP
            with np.errstate(invalid="ignore"):
                assert (eo.counts_of(dn, r, cap)[~(r > 0)] <= counts_of(dn, 0.0)[~(r > 0)]).all()
    # the row that holds `at` is listed by radii[q] == at under cap == at alone
    r0, r1 = oc.each_radii(rs, d, 0), oc.each_radii(rs, d, 1)
    full = eo.counts_of(dn, r0, at)[h]
    assert eo.counts_of(dn, r0, below)[h] < full and eo.counts_of(dn, r1, at)[h] < full


@pytest.mark.parametrize("name,k", CASES)
def test_the_own_row_windows_have_neighbours_and_the_run_has_copies(name, k):
    first, d = oc.window(name, k)
    own = first + np.arange(oc.M)
    assert first % 64 != 0 and np.isnan(d[np.arange(oc.M), own]).all() and np.isnan(d).sum() == oc.M
    rs = oc.own_radii(name, k)
    r = dict(rs)
    c = counts_of(d, r["at"])
    print(f"{name} k {k} own rows: at {r['at']!r} largest count {c.max()}, {int((c == 0).sum())} rows with none, "
          f"{int(counts_of(d, 0.0).sum())} pairs at distance 0")
    assert ((c >= 1) & (c <= 63)).any() and (oc.leaving(d, r["at"]) > 0).any()
    assert (c == 0).any() or (name, k) == ("lattice", 8)        # (every row of that lattice has a neighbour one step away)
    for rname, r2 in rs:
        assert counts_of(d, r2).max() <= oc.CAP, (rname, r2)
    # the own row kept (distance 0) would change every list, at every radius
    kept = np.array(d)
    kept[np.arange(oc.M), own] = 0.0
    assert (counts_of(kept, 0.0) == counts_of(d, 0.0) + 1).all()
    if name in oc.TIED:
        run = oc.run_rows()
        inside = run[run >= first]
        assert inside.size == 3 and inside[0] == first
        for row in inside:      # an own row of the run: the four other rows of the run at distance 0, before and behind it
            others = run[run != row]
            assert (d[row - first, others] == 0).all() and (others < first).sum() == 2 and (others >= first).sum() == 2
            assert counts_of(d, 0.0)[row - first] >= oc.RUN - 1
    dn = oc.near(name, k, own=True)[1]
    for phase in (0, 1):
        rr = oc.each_radii(rs, d, phase)
        assert eo.counts_of(dn, rr, r["at"]).max() <= oc.CAP
        eo.assert_no_shared_radius_passes(dn, rr, r["at"])


@pytest.mark.parametrize("name,k", CASES)
def test_the_near_columns_give_the_oracles_what_all_columns_give(name, k):
    """tests.offcube_rows.near: the GPU tests evaluate the oracles on the columns within the largest radius, numbered by gids."""
    for own in (False, True):
        d = oc.window(name, k)[1] if own else oc.batch(name, k)[2]
        rs = oc.own_radii(name, k) if own else oc.radii(name, k)
        cols, dn, gids = oc.near(name, k, own=own)
        assert cols.size < oc.N17 // 8 and (gids == cols + oc.BASE).all() and oc.BASE > 0
        np.testing.assert_array_equal(dn.view(np.uint32), d[:, cols].view(np.uint32))
        for rname, r2 in rs:
            assert not differ(lists_of(dn, r2, gids=gids), lists_of(d, r2, base=oc.BASE)), (own, rname)
        for phase in (0, 1):
            r = oc.each_radii(rs, d, phase)
            cap = dict(rs)["at"]
            assert not differ(eo.lists_of(dn, r, cap, gids=gids), eo.lists_of(d, r, cap, base=oc.BASE)), (own, phase)
        if not own:
            for mname, bits in oc.masks(name, k):
                a, b = want_of(dn, bits[cols], dict(rs)["at"], gids=gids), want_of(d, bits, dict(rs)["at"], base=oc.BASE)
                assert (a[0] == b[0]).all() and not differ(a[1], b[1]), mname


# ---- the radius cap, knn_threshold_within at u = +INF (the count forms of the prep kernel), through knn_debug_within_bound ------

def rounds_down_pair(k, offset):
    """(q, r) float32 [k] whose v0 distance loses as much as fp32 can lose: dimension 0 differs by a (coordinates near `offset`),
    every other dimension by b with b * b just under half an ulp of S = fl(a * a), S just above a power of two — every one of v0's
    k - 1 additions rounds back down to S, so E == S while the exact squared distance is S (1 + (k - 1) 2^-24) nearly: scales
    2^12 apart between the dimensions, as in `scaled`."""
    a = np.float32(0.25) + np.float32(2.0 ** -10)
    S = np.float32(a * a)
    half = np.float32(np.spacing(S)) * np.float32(0.5)
    b = np.float32(np.sqrt(np.float64(half)))
    while np.float32(b * b) >= half:
        b = np.nextafter(b, np.float32(0))
    q = np.zeros(k, dtype=np.float32)
    r = np.full(k, -b, dtype=np.float32)
    q[0], r[0] = np.float32(offset) + a, np.float32(offset)
    assert q[0] - r[0] == a
    return q, r, S


@pytest.mark.parametrize("k", [16, 20, 24, 32])
@pytest.mark.parametrize("log2_sigma", [-6, 0, 9])
@pytest.mark.parametrize("offset", [0.0, 4096.0])
def test_the_radius_alone_bounds_a_row_whose_v0_distance_rounded_down_at_every_addition(k, log2_sigma, offset):
    """The row holds the radius exactly (E == max_dist2) and no seed score stands behind the cap (u = +INF): its exact scaled
    distance D must not exceed the Dup the prep kernel stores, and the re-rank's gate must let E through.  For k >= 24 the exact
    distance is more than 1 + 1e-6 + 2^-23 times E — the factor and the rounding the stored Dup is taken larger by —, so a cap
    without its (1 + g2), sigma^2 max_dist2, is below D."""
    q, r, S = rounds_down_pair(k, offset)
    e = _v0(q, r)
    assert e == S                                        # every addition rounded down
    exact = _exact_d2(q, r)
    lost = float(exact / Fraction(float(e)) - 1)
    assert 0.99 * (k - 1) * 2.0 ** -24 < lost <= (k + 3) * 2.0 ** -24              # nearly g2 = (k + 3) 2^-24, and within it
    if k >= 24:
        assert lost > 1e-6 + 2.0 ** -23
    sigma = 2.0 ** log2_sigma
    mq = 0.3
    for r2 in (float(e), float(np.nextafter(e, np.float32(np.inf)))):
        thr, dup, gate = pkg.debug_within_bound(k, sigma, 1.0, 1.0, float(k), float("inf"), mq, r2)
        assert np.isfinite(thr) and np.isfinite(dup)
        assert exact * Fraction(sigma) ** 2 <= Fraction(dup), (k, r2, float(exact) * sigma * sigma, dup)
        assert gate >= e, (k, r2, gate, float(e))
