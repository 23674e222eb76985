"""knn_index_count_within_masked_routed and knn_index_list_within_masked_routed on the cell-pruned scan (KNN_QUERY_COUNT_CELLS; way
4) off the unit cube: the batches of tests/offcube_rows.py at every radius of theirs under a random half of the rows and — on the
lattice and among the copies — under a mask that admits exactly one row of every run of equal rows, so that of the rows a query
holds at one distance (0 included) some are admitted and some are not.  Against tests/masked_routed_helper.want_of (the oracle's
distances with the masked-out columns at +INF) and against the existing masked calls.  Bar: exact counts, lists exact as sorted
segments, fill == counts, keys carry base_index, no masked-out row listed; knn_index_last_stats()[0] == 4 at every call, [2] == 0
on uniform and offset rows, printed for the others."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import offcube_rows as oc
from tests.each_helper import dev_f32
from tests.masked_routed_helper import assert_same_answer, dev_words, existing_pipeline, routed_pipeline, want_of, words_of
from tests.offcube_helper import OPTIONS, assert_base_carried, check_stats, index_on_way_4

pytestmark = pytest.mark.gpu
LOW = np.uint64(0xFFFFFFFF)


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


@pytest.mark.parametrize("name,layout", oc.PAIRS, ids=oc.PAIR_IDS)
def test_masked_counts_and_lists_are_exact_on_the_pruned_way(name, layout):
    lname, k, _ = layout
    _, Q, d = oc.batch(name, k)
    cols, dn, gids = oc.near(name, k)
    with index_on_way_4(name, layout) as ix:
        q_d = dev_f32(Q.copy())
        for mname, bits in oc.masks(name, k):
            w_d = dev_words(words_of(bits))
            for rname, r2 in oc.radii(name, k):
                want = want_of(dn, bits[cols], r2, gids=gids)
                got = routed_pipeline([ix], q_d, [w_d], oc.M, r2, cells=True)
                check_stats(got[4], name, lname, f"masked {mname} {rname}")
                msg = f"{name} {lname} {mname} {rname} r2={r2!r}"
                assert_same_answer(got, want, existing_pipeline([ix], q_d, [w_d], oc.M, r2), msg=msg)
                assert_base_carried(got[3], msg)
                assert bits[(got[3] & LOW).astype(np.int64) - oc.BASE].all(), msg
