"""knn_index_self_cluster_within on the exact self-scan in EVERY compiled form of knn_cluster_link_kernel<KC> on the GPU against
tests/cluster_oracle.py: k = 7 (KC 1, a partial chunk), 16 (KC 1), 17 (2), 48 (3), 49 (4), 80 (5), 81 (6), 112 (7), 113 (8, a partial
last chunk), 128 (8) and 129, 200 (KC 0, the generic loop).  The rows are tests/cluster_rows.sheet(k): distances that round, so
"E(i, j) == E(j, i) bit for bit" and the border key's order by E's bits are asked of sums of k rounded terms; n = 1300, n % 64 = 20,
the core kernel's last wave stores one word; base_index != 0.  Bar: labels and core mask equal the oracle's exactly."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import cluster_oracle as co
from tests import cluster_rows as cr
from tests.cluster_helper import assert_planted, run_cluster

pytestmark = pytest.mark.gpu
BASE = 5
N = cr.SHEET_N
CAP, MIN_PTS = cr.SHEET_CAP, cr.SHEET_MIN_PTS


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"


def assert_equals(got, words, w):
    np.testing.assert_array_equal(got, w["labels"])
    if words is not None:
        np.testing.assert_array_equal(words, co.core_mask_words(w["core"]))


@pytest.mark.parametrize("k", cr.SHEET_KS)
def test_every_link_kernel_form_gives_the_oracles_labels_and_core_mask(k):
    R, names, off = cr.sheet(k)
    w = cr.want_sheet(k)
    s = cr.shares(w)
    print(f"k={k} (KC {(k + 15) // 16 if k <= 128 else 0}): core {s[0]:.3f} border {s[1]:.3f} noise {s[2]:.3f} of {N} rows, "
          f"{np.unique(w['labels']).size - 1} clusters")
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        labels, words, st = run_cluster(ix, CAP, MIN_PTS)
        assert st == [1, 0, 0, 0], st
        assert_equals(labels, words, w)
        assert_planted(labels, w["core"], names, off, MIN_PTS)
        print(f"k={k}: largest cluster on the GPU {cr.largest_cluster(labels)} rows")
        # again, without a core mask: bit for bit the same
        again, none, st = run_cluster(ix, CAP, MIN_PTS, want_core=False)
        assert none is None and st == [1, 0, 0, 0]
        np.testing.assert_array_equal(again, labels)
        # min_pts = 1: the components of the radius graph, every mask bit below n set
        comp, cw, _ = run_cluster(ix, CAP, 1)
        assert_equals(comp, None, cr.want_sheet(k, CAP, 1))
        np.testing.assert_array_equal(cw, co.core_mask_words(np.ones(N, dtype=bool)))
        # a held radius: the row's fourth-nearest other row lies at E4 exactly — core at E4, not core at the next float below
        row, e4, below = cr.held_radius(k)
        at, aw, _ = run_cluster(ix, e4, MIN_PTS)
        assert_equals(at, aw, cr.want_sheet(k, e4, MIN_PTS))
        under, uw, _ = run_cluster(ix, below, MIN_PTS)
        assert_equals(under, uw, cr.want_sheet(k, below, MIN_PTS))
        assert (aw[row >> 5] >> np.uint32(row & 31)) & 1 == 1 and (uw[row >> 5] >> np.uint32(row & 31)) & 1 == 0
    finally:
        ix.close()


@pytest.mark.parametrize("k", [129, 17])
def test_the_host_form_numbers_the_same_clusters(k):
    R, _, _ = cr.sheet(k)
    w = cr.want_sheet(k)
    lab, core, border = w["labels"], w["core"], w["border"]
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        hl, hc, info = ix.self_cluster_within_host(CAP, MIN_PTS)
        np.testing.assert_array_equal(hl, co.renumber(lab))
        np.testing.assert_array_equal(hc, core)
        assert info == dict(clusters=np.unique(lab).size - 1, core=int(core.sum()), border=int(border.sum()), noise=int((lab < 0).sum()))
    finally:
        ix.close()
