"""What the GPU tests of the out-of-box launches rest on (tests/test_outlier_each_gpu.py, tests/test_outlier_self_gpu.py,
tests/test_outlier_blocks_gpu.py), asserted from the oracle alone on the rows of tests/outlier_rows.py: the batches hold every kind
of count, no radius serves a whole wave, the hits of a query beside a planted row ARE planted rows, and a kernel that is wrong in
one of the ways the out-of-box bodies can be wrong — own row kept, cap read for radii[q], base + row for gids[row], a stale own-row
base, one block of 256 rows only, no launch at all — would change an expected list."""
import numpy as np
import pytest

from tests import each_oracle as eo
from tests import outlier_rows as orow

KS = (16, 8)
LOW = np.uint64(0xFFFFFFFF)


def held_cap(r, first_kind=0):
    return orow.kind_max(r, "held", eo.KINDS, first_kind)


def planted_keys(lists, base=0):
    """The keys of planted rows alone (numbers base + row)."""
    return [x[orow.is_planted((x & LOW).astype(np.int64) - base)] for x in lists]


def differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def windows(k):
    """(name, distances, first kind) of every batch and window the GPU tests run."""
    _, d = orow.each_batch(k)
    _, d1, _, d2 = orow.two_pass_batches(k)
    return [("each", d, 0), ("each first pass", d1, 0), ("each second pass", d2, 4),
            ("own inside", orow.own_dist2(k, orow.INSIDE_FIRST, orow.WINDOW), 0),
            ("own straddling", orow.own_dist2(k, orow.STRADDLE_FIRST, orow.WINDOW), 0),
            ("own second pass", orow.own_dist2(k, orow.TWO_PASS_FIRST + orow.PASS, orow.WINDOW), 4)]


@pytest.mark.parametrize("k", KS)
def test_the_rows_are_what_the_module_says(k):
    R = orow.rows(k)
    a, b = orow.planted_range()
    assert R.shape == (orow.N17, k) and b - a == orow.P == 640 and a % 64 != 0
    planted = orow.is_planted(np.arange(orow.N17))
    assert planted.sum() == orow.P
    assert (R[planted, 0] > 1.445).all()                                       # outside any box the filter can make (module docstring)
    assert (R[~planted] >= 0.45).all() and (R[~planted] <= np.float32(0.55)).all()
    first, second = R[a:b:2], R[a + 1:b:2]
    same = (first == second).all(axis=1)
    assert same[::8].all() and not same[np.arange(same.size) % 8 != 0].any()    # every eighth pair is an exact copy, no other
    assert (np.abs(second - first) <= 1.001e-3).all()
    copies = orow.copy_rows()
    assert copies.size == orow.P // 8 and (R[copies] == R[orow.twin_of(copies)]).all() and orow.is_planted(copies).all()
    # the windows: inside a block of 64, inside the planted block, across its end, and a second pass inside it
    assert orow.INSIDE_FIRST % 64 != 0 and orow.is_planted([orow.INSIDE_FIRST, orow.INSIDE_FIRST + orow.WINDOW - 1]).all()
    assert orow.is_planted(orow.STRADDLE_FIRST) and not orow.is_planted(orow.STRADDLE_FIRST + orow.WINDOW - 1)
    second_pass = orow.TWO_PASS_FIRST + orow.PASS + np.arange(orow.WINDOW)
    assert orow.is_planted(second_pass).all() and not orow.is_planted(orow.TWO_PASS_FIRST)
    # more outlier rows than one block (256) and one wave (64) walk, fewer than the filter gives up at (n / 32)
    assert 2 * 256 < orow.P <= orow.N17 // 32


@pytest.mark.parametrize("k", KS)
def test_every_batch_holds_every_kind_of_count_and_no_radius_serves_a_wave(k):
    for name, d, first_kind in windows(k):
        r = eo.radii_of(d, first_kind=first_kind)
        eo.assert_every_kind_of_count(eo.counts_of(d, r))
        eo.assert_no_shared_radius_passes(d, r)
        eo.assert_no_shared_radius_passes(d, r, held_cap(r, first_kind))
    # the second pass under the first pass's radii would count differently: a stale radii pointer cannot pass
    _, d1, _, d2 = orow.two_pass_batches(k)
    r1, r2 = eo.radii_of(d1), eo.radii_of(d2, first_kind=4)
    cap = max(held_cap(r1), held_cap(r2, 4))
    eo.assert_a_stale_pointer_fails(d2, r2, np.tile(r1, 2)[:d2.shape[0]], cap)
    o1 = orow.own_dist2(k, orow.TWO_PASS_FIRST, 64)
    o2 = orow.own_dist2(k, orow.TWO_PASS_FIRST + orow.PASS, orow.WINDOW)
    q1, q2 = eo.radii_of(o1), eo.radii_of(o2, first_kind=4)
    eo.assert_a_stale_pointer_fails(o2, q2, np.tile(q1, 2)[:orow.WINDOW], max(held_cap(q1), held_cap(q2, 4)))


@pytest.mark.parametrize("k", KS)
def test_the_hits_beside_planted_rows_are_planted_rows(k):
    _, d = orow.each_batch(k)
    r = eo.radii_of(d)
    cap = held_cap(r)
    hit = eo.hits_of(d, r, cap)[:orow.M_BESIDE]
    a, b = orow.planted_range()
    planted = int(hit[:, a:b].sum())
    print(f"k {k}: held cap {cap}: {int(hit.sum())} hits of the queries beside planted rows, {planted} of them planted rows")
    assert planted >= orow.P // 2 and planted == int(hit.sum())
    # under the low cap some radii exceed the cap (acc <= cap decides) and some do not (acc <= radii[q] decides)
    low = orow.low_cap(r)
    with np.errstate(invalid="ignore"):
        assert (r[:orow.M_BESIDE] > low).any() and ((r[:orow.M_BESIDE] < low) & (r[:orow.M_BESIDE] > 0)).any()
    assert differ(eo.lists_of(d, r, low), eo.lists_of(d, r, cap)) and int(eo.hits_of(d, r, low)[:orow.M_BESIDE, a:b].sum()) > 0
    # the queries in the cluster get no planted row: their hits are the re-rank's
    assert eo.hits_of(d, r, cap)[orow.M_BESIDE:, a:b].sum() == 0 and eo.counts_of(d, r, cap)[orow.M_BESIDE:].sum() > 0


@pytest.mark.parametrize("k", KS)
def test_own_rows_in_the_planted_block_have_planted_neighbours_and_copies(k):
    a, b = orow.planted_range()
    for first in (orow.INSIDE_FIRST, orow.TWO_PASS_FIRST + orow.PASS):
        d = orow.own_dist2(k, first, orow.WINDOW)
        held = eo.radii_of(d, kinds=("held",))
        assert (orow.planted_hits(d, held) >= 1).all()
        assert (eo.counts_of(d, held) == orow.planted_hits(d, held)).all()        # and nothing else: all from the out-of-box launch
        copies = [c for c in orow.copy_rows() if first <= c < first + orow.WINDOW]
        assert len(copies) >= 4
        for c in copies:
            assert d[c - first, orow.twin_of(c)] == 0 and np.isnan(d[c - first, c])
    # across the block's end: own rows outside the box with planted neighbours, own rows inside it with none but cluster rows
    d = orow.own_dist2(k, orow.STRADDLE_FIRST, orow.WINDOW)
    r = eo.radii_of(d)
    hit = eo.hits_of(d, r, held_cap(r))
    inside = ~orow.is_planted(orow.STRADDLE_FIRST + np.arange(orow.WINDOW))
    assert hit[~inside, a:b].sum() > 0 and hit[~inside].sum() == hit[~inside, a:b].sum()
    assert hit[inside].sum() > 0 and hit[inside, a:b].sum() == 0


@pytest.mark.parametrize("k", KS)
def test_a_wrong_out_of_box_kernel_would_change_an_expected_list(k):
    a, b = orow.planted_range()
    _, d = orow.each_batch(k)
    r = eo.radii_of(d)
    cap = held_cap(r)
    want = eo.lists_of(d, r, cap, base=orow.BASE)
    # no out-of-box launch at all
    assert differ(want, [x[~orow.is_planted((x & LOW).astype(np.int64) - orow.BASE)] for x in want])
    # the cap read in place of radii[q]: among the PLANTED keys (the re-rank has its own compare)
    as_cap = eo.lists_of(d, np.full(d.shape[0], cap, np.float32), cap, base=orow.BASE)
    assert differ(planted_keys(want, orow.BASE), planted_keys(as_cap, orow.BASE))
    # base + row in place of gids[row] (a cell-range shard's rows carry their own numbers)
    gids = 3 * np.arange(orow.N17, dtype=np.int64) + 5
    with_gids = eo.lists_of(d, r, cap, gids=gids)
    numbers = np.concatenate([(x & LOW).astype(np.int64) for x in with_gids])
    assert numbers.size and np.isin(numbers, gids[a:b]).any()
    assert differ(with_gids, eo.lists_of(d, r, cap, base=0))
    # the own row kept: it is a planted row, so only the out-of-box launch can list it
    first = orow.INSIDE_FIRST
    own = orow.own_dist2(k, first, orow.WINDOW)
    ro = eo.radii_of(own)
    kept = np.array(own)
    kept[np.arange(orow.WINDOW), first + np.arange(orow.WINDOW)] = 0.0
    for radii in (ro, np.full(orow.WINDOW, held_cap(ro), np.float32)):
        assert differ(eo.lists_of(own, radii, held_cap(ro)), eo.lists_of(kept, radii, held_cap(ro)))
    # a stale own-row base in the second pass: row first + j is dropped where first + 1024 + j is meant
    first = orow.TWO_PASS_FIRST
    second = orow.own_dist2(k, first + orow.PASS, orow.WINDOW)
    stale = np.array(second)
    stale[np.arange(orow.WINDOW), first + orow.PASS + np.arange(orow.WINDOW)] = 0.0
    stale[np.arange(orow.WINDOW), first + np.arange(orow.WINDOW)] = np.nan
    rs = eo.radii_of(second, first_kind=4)
    assert differ(eo.lists_of(second, rs, held_cap(rs, 4)), eo.lists_of(stale, rs, held_cap(rs, 4)))
    # one block of 256 rows only: some query has more planted hits than one block can see, and all its hits are planted rows
    _, dc = orow.centre_batch(k)
    big = orow.blocks_radius(k)
    assert orow.planted_hits(dc, big).max() >= 300
    assert (eo.counts_of(dc, np.full(dc.shape[0], big, np.float32)) == orow.planted_hits(dc, big)).all()
    assert (eo.counts_of(dc, np.full(dc.shape[0], big, np.float32)) == 0).any()
