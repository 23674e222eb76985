"""knn_index_count_within_each and knn_index_list_within_each on the cell-pruned scan (KNN_QUERY_COUNT_CELLS; way 4) off the unit
cube: the batches of tests/offcube_rows.py with a radius per query that cycles through `at` (a value some row holds exactly),
`below` (the next float towards 0), 0, NaN and -1, once with the cap at `at` and once with the cap at `below` — so the row that
holds `at` is kept by radii[q] == at under cap == at alone, and dropped by radii[q] in one run and by the cap in another.  Against
tests/each_oracle.py.  Bar: exact counts, lists exact as sorted segments, fill == counts, keys carry base_index;
knn_index_last_stats()[0] == 4 at every call, [2] == 0 on uniform and offset rows, printed for the others."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests import offcube_rows as oc
from tests.each_helper import assert_segments, dev_f32, pipeline
from tests.offcube_helper import OPTIONS, assert_base_carried, check_stats, index_on_way_4

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


@pytest.mark.parametrize("name,layout", oc.PAIRS, ids=oc.PAIR_IDS)
def test_a_radius_per_query_under_both_caps_is_exact_on_the_pruned_way(name, layout):
    lname, k, _ = layout
    _, Q, d = oc.batch(name, k)
    _, dn, gids = oc.near(name, k)
    rs = oc.radii(name, k)
    at, below = dict(rs)["at"], dict(rs)["below"]
    h = oc.holder(d, at)
    with index_on_way_4(name, layout) as ix:
        q_d = dev_f32(Q.copy())
        seen = {}
        for phase in (0, 1):
            r = oc.each_radii(rs, d, phase)
            for cname, cap in (("at", at), ("below", below)):
                want = eo.lists_of(dn, r, cap, gids=gids)
                np.testing.assert_array_equal(eo.lengths(want), eo.counts_of(d, r, cap))
                counts, off, fill, keys, stats = pipeline([ix], q_d, dev_f32(r), oc.M, cap=cap, cells=True)
                check_stats(stats, name, lname, f"each phase {phase} cap {cname}")
                msg = f"{name} {lname} phase {phase} cap {cname}={cap!r}"
                np.testing.assert_array_equal(counts, eo.lengths(want), err_msg=msg)
                np.testing.assert_array_equal(fill, counts, err_msg=f"{msg} fill")
                assert_segments(off, keys, want, msg=msg)
                assert_base_carried(keys, msg)
                seen[(phase, cname)] = int(counts[h])
        # the holder's row at `at`: there under radii[q] == cap == at, gone under either `below`
        assert seen[(0, "below")] < seen[(0, "at")] and seen[(1, "at")] < seen[(0, "at")], seen
