"""knn_index_self_count_within_routed and knn_index_self_list_within_routed on the cell-pruned scan (KNN_QUERY_COUNT_CELLS; way 4)
off the unit cube: a window of 64 own rows of every shard of tests/offcube_rows.py — on the lattice and among the copies it starts
inside a run of five equal rows, two of them before the window —, radii from the rows' own distances with the own row left out (a
value some row holds exactly, the next float below it, 0, the smallest subnormal), as one scalar radius and as a radius per row.
Against tests/each_oracle.py over tests/self_oracle.self_dist2, and against the existing self calls.  Bar: exact counts, lists
exact as sorted segments, fill == counts, keys carry base_index, the own row never listed and every exact copy of it listed at
distance 0; knn_index_last_stats()[0] == 4 at every call, [2] == 0 on uniform and offset rows, printed for the others."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests import offcube_rows as oc
from tests.each_helper import dev_f32
from tests.offcube_helper import OPTIONS, assert_base_carried, check_stats, index_on_way_4
from tests.self_routed_helper import assert_own_row_absent, assert_same_answer, existing_pipeline, routed_pipeline, segment_numbers

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def assert_copies_listed(got, name, first, radii, msg):
    """lattice, copies: an own row of the run lists the run's four other rows — two before the window, two own rows of other
    queries — at distance 0 (under any radius >= 0), and not itself (assert_own_row_absent)."""
    if name not in oc.TIED:
        return
    run = oc.run_rows()
    for row in run[run >= first]:
        j = int(row - first)
        with np.errstate(invalid="ignore"):
            if not radii[j] >= 0:
                continue
        numbers, bits = segment_numbers(got, j)
        zero = set(numbers[bits == 0].tolist())
        assert {int(oc.BASE + o) for o in run if o != row} <= zero and int(oc.BASE + row) not in zero, (msg, j, sorted(zero))


@pytest.mark.parametrize("name,layout", oc.PAIRS, ids=oc.PAIR_IDS)
def test_own_rows_under_scalar_and_per_row_radii_are_exact_on_the_pruned_way(name, layout):
    lname, k, _ = layout
    first, d = oc.window(name, k)
    _, dn, gids = oc.near(name, k, own=True)
    rs = oc.own_radii(name, k)
    at = dict(rs)["at"]
    own = oc.BASE + first + np.arange(oc.M)
    with index_on_way_4(name, layout) as ix:
        runs = [(f"scalar {rname}", r2, None) for rname, r2 in rs] + [(f"each phase {p}", at, oc.each_radii(rs, d, p)) for p in (0, 1)]
        for form, cap, rr in runs:
            radii = np.full(oc.M, cap, np.float32) if rr is None else rr
            want = eo.lists_of(dn, radii, cap, gids=gids)
            np.testing.assert_array_equal(eo.lengths(want), eo.counts_of(d, radii, cap))
            r_d = dev_f32(rr) if rr is not None else None
            got = routed_pipeline(ix, first, oc.M, cap, r_d, cells=True)
            check_stats(got[4], name, lname, f"self {form}")
            msg = f"{name} {lname} {form} cap={cap!r}"
            assert_same_answer(got, want, existing_pipeline(ix, first, oc.M, cap, r_d), msg=msg)
            assert_own_row_absent(got, own, msg=msg)
            assert_copies_listed(got, name, first, radii, msg)
            assert_base_carried(got[3], msg)
