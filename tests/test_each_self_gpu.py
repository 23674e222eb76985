"""knn_index_self_count_within_each and knn_index_self_list_within_each on the GPU against tests/each_oracle.py over
tests/self_oracle.self_dist2, and the pipeline the calls exist for: self_topk -> knn_keys_column_dist2 -> the two calls, with
nothing copied to the host in between."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.count_helper import dev, dev_counts, host_counts
from tests.each_helper import assert_segments, dev_f32, pipeline
from tests.list_helper import host_u64
from tests.self_oracle import self_dist2, self_topk
from tests.topk_oracle import KEY_INIT

pytestmark = pytest.mark.gpu
N, FIRST, ROWS, BASE = 3149, 2090, 150, 11
INF = np.float32(np.inf)


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


def rows_of(k, seed, n=N):
    rng = np.random.default_rng(seed)
    R = rng.random((n, k), dtype=np.float32)
    R[5, 0] = np.nan
    R[6, k - 1] = np.inf
    R[7] = 3e38
    return R


def self_pipeline(ix, first, rows, r_d, cap=float("inf")):
    def count(ix, counts, init):
        ix.self_count_within_each(first, rows, r_d.data_ptr(), counts.data_ptr(), cap=cap, init=init)

    def lst(ix, off, fill, keys, init):
        ix.self_list_within_each(first, rows, r_d.data_ptr(), off.data_ptr(), fill.data_ptr(), keys.data_ptr(), cap=cap, init=init)

    return pipeline([ix], None, r_d, rows, count=count, lst=lst)


@pytest.mark.parametrize("k", [3, 16])
def test_oracle_radii_never_list_self_and_list_a_duplicate_at_distance_zero(k):
    R = rows_of(k, 9500 + k)
    R[FIRST + 2] = R[50]            # a "zero" and a "minus_zero" query with a copy elsewhere in the shard,
    R[FIRST + 3] = R[51]
    R[FIRST + 11] = R[FIRST + 20]   # and a "zero" query with a copy inside its own block of 64
    d = self_dist2(R, k, FIRST, ROWS)
    r = eo.radii_of(d)
    assert eo.KINDS[2] == "zero" and eo.KINDS[3] == "minus_zero" and eo.KINDS[11 % 9] == "zero"
    lists = eo.lists_of(d, r, base=BASE)
    want = eo.lengths(lists)
    assert want[2] == 1 and want[3] == 1 and want[11] == 1 and (lists[11] & np.uint64(0xFFFFFFFF))[0] == BASE + FIRST + 20
    eo.assert_every_kind_of_count(want)
    eo.assert_no_shared_radius_passes(d, r)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        for cap in (float("inf"), float(np.sort(r[(r > 0) & (r < INF)])[ROWS // 4])):
            lists = eo.lists_of(d, r, cap, base=BASE)
            counts, off, fill, keys, stats = self_pipeline(ix, FIRST, ROWS, dev_f32(r), cap=cap)
            assert all(st == [1, 0, 0, 0] for st in stats), stats
            np.testing.assert_array_equal(counts, eo.lengths(lists))
            np.testing.assert_array_equal(fill, counts)
            assert_segments(off, keys, lists, msg=f"k={k} cap={cap}")
            own = np.uint64(BASE + FIRST) + np.arange(ROWS, dtype=np.uint64)
            for j in range(ROWS):      # self is never a hit
                assert not ((keys[int(off[j]):int(off[j + 1])] & np.uint64(0xFFFFFFFF)) == own[j]).any(), j
        # a fold adds
        held = dev_counts(ROWS, fill=np.arange(ROWS, dtype=np.uint32) * 7)
        ix.self_count_within_each(FIRST, ROWS, dev_f32(r).data_ptr(), held.data_ptr(), init=False)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host_counts(held), np.arange(ROWS, dtype=np.uint32) * 7 + want)
    finally:
        ix.close()


@pytest.mark.parametrize("k", [3, 16])
def test_everything_within_the_kth_neighbours_distance_without_leaving_the_device(k):
    K = 8
    R = rows_of(k, 9600 + k)
    R[FIRST + 9] = R[7]             # a 3e38 row among the queries: every distance overflows but the one to its copy, row 7 — a
                                    # padded list, radius +INF from the padding, and one hit: the only other row at a finite distance
    R[FIRST + 30] = R[FIRST + 31]   # a tie at distance 0
    d = self_dist2(R, k, FIRST, ROWS)
    top = self_topk(d, K, base=BASE)
    kth = (top[:, K - 1] >> np.uint64(32)).astype(np.uint32).view(np.float32)        # +INF where the list is padded
    assert top[9, 0] == np.uint64(BASE + 7) and (top[9, 1:] == KEY_INIT).all() and np.isinf(kth[9])
    assert (kth[np.arange(ROWS) != 9] < INF).all()
    lists = eo.lists_of(d, kth, base=BASE)
    want = eo.lengths(lists)
    eo.assert_no_shared_radius_passes(d, kth)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        keys8 = torch.empty(ROWS * K, dtype=torch.int64, device=dev())
        r_d = torch.empty(ROWS, dtype=torch.float32, device=dev())
        ix.self_topk(FIRST, ROWS, K, keys8.data_ptr(), init_keys=True)
        pkg.keys_column_dist2(keys8.data_ptr(), ROWS, K, K - 1, r_d.data_ptr())
        counts, off, fill, keys, _ = self_pipeline(ix, FIRST, ROWS, r_d)
        got8 = host_u64(keys8).reshape(ROWS, K)
        np.testing.assert_array_equal(got8, top)
        np.testing.assert_array_equal(r_d.cpu().numpy().view(np.uint32), kth.view(np.uint32))
        np.testing.assert_array_equal(counts, want)
        assert (counts >= (got8 != KEY_INIT).sum(axis=1)).all() and counts[9] == 1
        assert_segments(off, keys, lists)
        for j in range(ROWS):          # the first K keys of every sorted segment are the top-K keys, bit for bit
            t = int((got8[j] != KEY_INIT).sum())
            np.testing.assert_array_equal(keys[int(off[j]):int(off[j]) + t], got8[j, :t], err_msg=str(j))
        # every column
        for col in (0, 3):
            pkg.keys_column_dist2(keys8.data_ptr(), ROWS, K, col, r_d.data_ptr())
            torch.cuda.synchronize()
            np.testing.assert_array_equal(r_d.cpu().numpy().view(np.uint32), (top[:, col] >> np.uint64(32)).astype(np.uint32))
    finally:
        ix.close()


def test_a_padded_list_gives_radius_inf_and_lists_every_other_finite_row():
    """Seven rows, one of them NaN, K = 8: every finite row has five other finite rows — a padded list, radius +INF from the padding
    — and lists exactly those five."""
    k, K, n = 3, 8, 7
    R = np.random.default_rng(9700).random((n, k), dtype=np.float32)
    R[4, 1] = np.nan
    d = self_dist2(R, k, 0, n)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        keys8 = torch.empty(n * K, dtype=torch.int64, device=dev())
        r_d = torch.empty(n, dtype=torch.float32, device=dev())
        ix.self_topk(0, n, K, keys8.data_ptr(), init_keys=True)
        pkg.keys_column_dist2(keys8.data_ptr(), n, K, K - 1, r_d.data_ptr())
        counts, off, fill, keys, _ = self_pipeline(ix, 0, n, r_d)
        assert np.isinf(r_d.cpu().numpy()).all()
        lists = eo.lists_of(d, np.full(n, INF), base=BASE)
        np.testing.assert_array_equal(counts, [5, 5, 5, 5, 0, 5, 5])
        assert_segments(off, keys, lists)
    finally:
        ix.close()


def test_two_chunks_of_rows_advance_the_radii():
    """rows = 65536 + 70 from row 100: the oracle is evaluated for the second chunk; the first chunk's radii are the second's finite
    ones, shifted by one query, so a stale radii pointer shows."""
    k, n, first, m1, m2 = 3, 70000, 100, 65536, 70
    R = rows_of(k, 9800, n=n)
    d2 = self_dist2(R, k, first + m1, m2)
    r2 = eo.radii_of(d2)
    small = np.roll(r2, -1)[~np.isinf(np.roll(r2, -1))]         # (+INF for a ninth of 65536 rows would list 5e8 keys)
    r1 = np.tile(small, m1 // small.size + 1)[:m1]
    r = np.concatenate([r1, r2])
    lists = eo.lists_of(d2, r2, base=BASE)
    eo.assert_every_kind_of_count(eo.lengths(lists))
    eo.assert_no_shared_radius_passes(d2, r2)
    eo.assert_a_stale_pointer_fails(d2, r2, r1)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        counts, off, fill, keys, _ = self_pipeline(ix, first, m1 + m2, dev_f32(r))
        np.testing.assert_array_equal(counts[m1:], eo.lengths(lists))
        np.testing.assert_array_equal(fill, counts)
        assert_segments(off[m1:], keys, lists, msg="second chunk")
    finally:
        ix.close()
