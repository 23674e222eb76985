"""One workspace slot's top-K scratch across calls (knn_topk_scratch_plan) on the GPU against the numpy
restatement of v0 (tests/topk_oracle.py): the buffers grow from a small call to a large one, a radius call adds the list
scratch, a small call reuses what is there, and another way then runs on the same buffers.  Bar: bit-exact keys every time."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.topk_oracle import KEY_INIT, keys_dist2, topk_keys
from tests.within_helper import clip, dev_keys, plain, within

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in ("path", "cells"):
        pkg.set_option(name, 0)


def test_a_slots_scratch_grows_and_serves_two_ways():
    rng = np.random.default_rng(70016)
    k, n, base = 16, 70000, 5
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((40, k), dtype=np.float32)
    want = topk_keys(Q, R, k, 64, base=base)
    r2 = float(np.median(keys_dist2(want[:, 0])))   # the median 1-NN distance: about half the lists stay empty
    assert (clip(want, r2)[:, 0] == KEY_INIT).any() and (clip(want, r2)[:, 0] != KEY_INIT).any()
    pkg.set_option("path", 2)
    pkg.set_option("cells", 2)
    ix = pkg.KnnIndex(k, R, base_index=base)
    try:
        for path in (2, 1):   # the dense filter way, then the exact way, on the same slot's buffers
            pkg.set_option("path", path)
            # 1: a small call writes its keys
            small = plain(ix, Q[:8], 2)
            assert ix.last_stats()[0] == path, ix.last_stats()
            np.testing.assert_array_equal(small, want[:8, :2], err_msg=f"path {path} step 1")
            # 2: a larger, deeper call folds into them (padded to K; the other queries hold nothing): every buffer grows
            held = np.full((40, 64), KEY_INIT, dtype=np.uint64)
            held[:8, :2] = small
            got = plain(ix, Q, 64, keys=dev_keys(40, 64, fill=held), init=False)
            assert ix.last_stats()[0] == path, ix.last_stats()
            np.testing.assert_array_equal(got, np.sort(np.concatenate([held, want], axis=1), axis=1)[:, :64],
                                          err_msg=f"path {path} step 2")
            # 3: a radius call writes (the filter way clips behind: the list scratch appears)
            got = within(ix, Q, 64, r2)
            assert ix.last_stats()[0] == path, ix.last_stats()
            np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"path {path} step 3")
            # 4: the small call again, in buffers sized for the large ones
            np.testing.assert_array_equal(plain(ix, Q[:8], 2), want[:8, :2], err_msg=f"path {path} step 4")
            assert ix.last_stats()[0] == path, ix.last_stats()
    finally:
        ix.close()
