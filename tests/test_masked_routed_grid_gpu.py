"""knn_index_count_within_masked_routed and knn_index_list_within_masked_routed on the uniform-grid index (KNN_QUERY_COUNT_GRID) on
the GPU against tests/each_oracle.py over tests/topk_oracle.v0_dist2 with the masked-out columns at +INF, and against the existing
masked calls.  Bar: exact counts and sorted lists under every mask at every radius; knn_index_last_stats tells the way (3) and
that no batch gave up ([2] == 0) — but for the one designated give-up case, where the gated masked scan answers once.

The radii are the finite ones of tests/test_count_grid_gpu.py (tests/count_oracle.radii: at, below, zero, under_all, large).  +INF
is left out of the routed masked radii: it spans no rings the plan can size the walk by, so on a shard of this size every +INF
batch gives up — a third fallback path beside the two designated ones, which these tests are not to have.  The gated masked scan
that would answer it is the one the give-up case below runs."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.count_helper import count, dev_counts, host_counts
from tests.count_oracle import radii
from tests.each_helper import dev_f32
from tests.list_helper import PAD, check_list, dev_u64, host_u64
from tests.masked_routed_helper import (assert_mask_bites, assert_same_answer, dev_words, existing_pipeline, routed_pipeline, scalar,
                                        under, want_of, words_of)
from tests.test_within_grid_gpu import rows_and_queries
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
BASE = 11
N = 16384 + 7                     # the smallest shard that gets a grid index, and a few rows: the last mask word holds 7 rows
M = 96
INF = float("inf")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    pkg.set_option("path", 0)


def masks(n, seed):
    """(name, bits [n], the last word's bits beyond n, whether some query must lose a hit and keep one)."""
    rng = np.random.default_rng(seed)
    half = rng.random(n) < 0.5
    rng_bits = np.zeros(n, dtype=bool)
    rng_bits[5003:12345] = True                      # starts at bit 11 of a word, ends at bit 25 of another
    assert 5003 % 32 not in (0, 31) and 12345 % 32 not in (0, 31)
    edge = np.zeros(n, dtype=bool)                   # bits 31 and 0 of alternating words: the rows either side of a word boundary
    w = np.arange(n) // 32
    edge[((np.arange(n) % 32 == 31) & (w % 2 == 0)) | ((np.arange(n) % 32 == 0) & (w % 2 == 1))] = True
    return [("half", half, 0, True), ("ones", np.ones(n, dtype=bool), 0, None), ("zero", np.zeros(n, dtype=bool), 0, False),
            ("range", rng_bits, 0, True), ("edges", edge, 0, True), ("beyond", rng.random(n) < 0.5, 1, True)]


ROW_SEED = {1: 8324, 2: 8302, 3: 8303, 4: 8304}   # (k = 1: under 8301 a query coincides with a row in fp32, and `under_all` needs none)


@pytest.mark.parametrize("k", [2, 3, 1, 4])
def test_every_mask_at_every_radius_is_exact_on_the_grid(k):
    R, Q = rows_and_queries(k, N, M, ROW_SEED[k])
    d = v0_dist2(Q, R, k)
    rad = [(name, r2) for name, r2 in radii(d) if r2 != INF]
    assert [name for name, _ in rad] == ["at", "below", "zero", "under_all", "large"]
    large = dict(rad)["large"]
    cases = masks(N, 8310 + k)
    for name, bits, _, keeps in cases:               # on the CPU, before the GPU is touched
        if keeps is not None:
            assert_mask_bites(d, bits, large, keeps=keeps)
    assert words_of(cases[-1][1], 1)[-1] >> 7 == (1 << 25) - 1 and N % 32 == 7
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        q_d = dev_f32(Q)
        for name, bits, beyond, _ in cases:
            w_d = dev_words(words_of(bits, beyond))
            for rname, r2 in rad:
                msg = f"k={k} mask {name} radius {rname}"
                want = want_of(d, bits, r2, base=BASE)
                got = routed_pipeline([ix], q_d, [w_d], M, r2, grid=True)
                assert all(st[:3] == [3, 0, 0] for st in got[4]), (msg, got[4])
                assert_same_answer(got, want, existing_pipeline([ix], q_d, [w_d], M, r2), msg=msg)
                if name == "ones":                   # what the unmasked grid call gives
                    np.testing.assert_array_equal(count(ix, Q, r2, grid=True), got[0], err_msg=msg)
                    check_list(ix, Q, r2, want[1], msg=msg, grid=True)
        # without a routing flag, with the cell flag (no cell layout here) and under option path = 1: the exact masked scan
        name, bits, _, _ = cases[0]
        w_d = dev_words(words_of(bits))
        want = want_of(d, bits, large, base=BASE)
        for flags in (dict(), dict(cells=True)):
            got = routed_pipeline([ix], q_d, [w_d], M, large, **flags)
            assert all(st == [1, 0, 0, 0] for st in got[4]), (flags, got[4])
            assert_same_answer(got, want, msg=f"k={k} {flags}")
        pkg.set_option("path", 1)
        got = routed_pipeline([ix], q_d, [w_d], M, large, grid=True)
        assert all(st == [1, 0, 0, 0] for st in got[4]), got[4]
        assert_same_answer(got, want, msg=f"k={k} path 1")
    finally:
        ix.close()


def test_a_fold_adds_and_a_short_segment_shows_in_fill():
    k = 3
    R, Q = rows_and_queries(k, N, M, 8303)
    d = v0_dist2(Q, R, k)
    r2 = dict(radii(d))["large"]
    bits = np.random.default_rng(8320).random(N) < 0.5
    assert_mask_bites(d, bits, r2)
    cnt, lists = want_of(d, bits, r2, base=BASE)
    assert (cnt > 1).any()
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        q_d, w_d = dev_f32(Q), dev_words(words_of(bits))
        # a fold without the init flag adds to the counts and appends behind the cursor
        held = (np.arange(M, dtype=np.uint32) * 3)
        counts = dev_counts(M, fill=held)
        ix.count_within_masked_routed(M, q_d.data_ptr(), r2, w_d.data_ptr(), counts.data_ptr(), grid=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[:3] == [3, 0, 0]
        np.testing.assert_array_equal(host_counts(counts), held + cnt)
        ahead = (np.arange(M, dtype=np.uint32) % 4)
        off = eo_offsets(cnt.astype(np.uint64) + ahead)
        fill, keys = dev_counts(M, fill=ahead), dev_u64(np.full(int(off[-1]), PAD))
        ix.list_within_masked_routed(M, q_d.data_ptr(), r2, w_d.data_ptr(), dev_u64(off).data_ptr(), fill.data_ptr(), keys.data_ptr(),
                                     grid=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[:3] == [3, 0, 0]
        np.testing.assert_array_equal(host_counts(fill), ahead + cnt)
        hk = host_u64(keys)
        for j in range(M):
            assert (hk[int(off[j]):int(off[j]) + int(ahead[j])] == PAD).all()
            np.testing.assert_array_equal(np.sort(hk[int(off[j]) + int(ahead[j]):int(off[j + 1])]), lists[j])
        # a segment with less room than hits: fill is the count, the key behind the segment keeps its sentinel
        rooms = np.where(cnt > 0, cnt - 1, 0).astype(np.uint64)
        off = np.concatenate([[np.uint64(1)], np.uint64(1) + np.cumsum(rooms)]).astype(np.uint64)
        fill, keys = dev_counts(M, fill=0xDEADBEEF), dev_u64(np.full(int(off[-1]) + 1, PAD))
        ix.list_within_masked_routed(M, q_d.data_ptr(), r2, w_d.data_ptr(), dev_u64(off).data_ptr(), fill.data_ptr(), keys.data_ptr(),
                                     init=True, grid=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host_counts(fill), cnt)
        hk = host_u64(keys)
        assert hk[0] == PAD and hk[-1] == PAD
        for j in range(M):
            seg = hk[int(off[j]):int(off[j + 1])]
            assert np.isin(seg, lists[j]).all() and np.unique(seg).size == seg.size, j
    finally:
        ix.close()


def eo_offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)


def test_a_walk_past_the_cell_budget_gives_up_and_the_gated_masked_scan_answers_once():
    """The k = 1 construction of tests/test_list_grid_gpu.py: a query 20 box widths out whose radius — its fourth nearest ADMITTED
    row — spans more rings than the 2^15-cell budget gives up ([2] == 1); the other queries' walks have by then counted and
    reserved in the scratch.  The gated masked scan answers the batch from the untouched counts and fill: exact, not doubled.  The
    next batch on the slot is back on the grid."""
    rng = np.random.default_rng(5)
    k, n = 1, 16384
    R = (0.5 + 0.5 * rng.random((n, k))).astype(np.float32)
    R[0] = 0.0
    lo, width = float(R.min()), float(R.max() - R.min())
    Q = (0.6 + 0.3 * rng.random((21, k))).astype(np.float32)
    Q[11] = lo - 2.0 * width
    Q[12] = lo - 20.0 * width
    bits = rng.random(n) < 0.5
    d = v0_dist2(Q, R, k)
    far = float(np.sort(under(d, bits)[12])[3])
    cnt, lists = want_of(d, bits, far, base=300)
    assert cnt[12] == 4 and (cnt > 64).any()
    plain = eo.counts_of(d, scalar(21, far))
    assert ((cnt < plain) & (cnt > 0)).any()
    rings = int(np.sqrt(far) / (width / 5000))
    assert rings > 16383
    assert pkg.debug_count_plan(k=k, m=21, n=n, radius_finite=1, flag_grid=1, flag_cells=0, has_grid=1, has_cells=0, centred=0,
                                rows_u8=0, bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=rings)["rmax"] == \
        pkg.debug_grid_topk_plan(k=k, K=1, m=21, has_grid=1, path=0, flag=1)["rmax"]
    inside = float(np.median(np.sort(d[:11], axis=1)[:, 4]))
    ix = pkg.KnnIndex(k, R, base_index=300)
    try:
        q_d, w_d = dev_f32(Q), dev_words(words_of(bits))
        got = routed_pipeline([ix], q_d, [w_d], 21, far, grid=True)
        assert all(st[:3] == [3, 0, 1] for st in got[4]), got[4]
        assert_same_answer(got, (cnt, lists), existing_pipeline([ix], q_d, [w_d], 21, far), msg="gave up")
        # folding calls: the held counts and cursor stay, the batch is added once
        held = np.full(21, 1000, np.uint32)
        counts = dev_counts(21, fill=held)
        ix.count_within_masked_routed(21, q_d.data_ptr(), far, w_d.data_ptr(), counts.data_ptr(), grid=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[:3] == [3, 0, 1]
        np.testing.assert_array_equal(host_counts(counts), held + cnt)
        # the next batch on the slot finds its word cleared
        got = routed_pipeline([ix], dev_f32(Q[:11]), [w_d], 11, inside, grid=True)
        assert all(st[:3] == [3, 0, 0] for st in got[4]), got[4]
        assert_same_answer(got, want_of(d[:11], bits, inside, base=300), msg="the next batch")
    finally:
        ix.close()
