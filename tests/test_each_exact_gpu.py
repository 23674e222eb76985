"""knn_index_count_within_each and knn_index_list_within_each on the exact scans (the default way) on the GPU against
tests/each_oracle.py: forms of knn_exact_count_each_kernel<KC> / knn_exact_list_each_kernel<KC> (KC 1, 2, 0), several slices, a second
(clamped) wave of queries, rows that are NaN, +INF and 3e38, every kind of radius, the cap, folds, overflowing segments, two chunks
of queries, index-range and cell-range shards."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests.count_helper import count, dev, dev_counts
from tests.each_helper import assert_segments, count_each, dev_f32, list_each, pipeline
from tests.list_helper import PAD, dev_u64
from tests.list_oracle import offsets_of
from tests.shards_helper import Shards
from tests.topk_oracle import v0_dist2

pytestmark = pytest.mark.gpu
N, M, BASE = 3149, 70, 11                      # several slices; a second wave of 6 queries, its lanes clamped
INF = float("inf")


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


def batch(k, seed, n=N, m=M):
    rng = np.random.default_rng(seed)
    R = rng.random((n, k), dtype=np.float32)
    R[5, 0] = np.nan
    R[6, k - 1] = np.inf
    R[7] = 3e38
    Q = rng.random((m, k), dtype=np.float32)
    Q[:, 0] += np.linspace(0.0, 1.5 if k <= 16 else 4.0, m, dtype=np.float32)
    return R, Q


@pytest.mark.parametrize("k", [1, 3, 16, 17, 129])
def test_counts_and_lists_at_every_kind_of_radius(k):
    R, Q = batch(k, 9000 + k)
    d = v0_dist2(Q, R, k)
    r = eo.radii_of(d)
    want = eo.counts_of(d, r)
    eo.assert_every_kind_of_count(want)
    eo.assert_no_shared_radius_passes(d, r)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        np.testing.assert_array_equal(count_each(ix, Q, r), want)
        assert ix.last_stats()[:3] == [1, 0, 0], ix.last_stats()
        # a fold adds to held counts
        held = np.arange(M, dtype=np.uint32) * 1000
        np.testing.assert_array_equal(count_each(ix, Q, r, counts=dev_counts(M, fill=held), init=False), held + want)
        # one radius for all: the scalar call's counts, through the radii and through the cap
        rr = float(r[eo.KINDS.index("many")])
        scalar = count(ix, Q, rr)
        np.testing.assert_array_equal(count_each(ix, Q, np.full(M, rr, np.float32)), scalar)
        np.testing.assert_array_equal(count_each(ix, Q, np.full(M, np.inf, np.float32), cap=rr), scalar)
        # a cap between the radii clips exactly the larger ones
        pos = np.sort(r[(r > 0) & (r < np.inf)])
        cap = float(pos[pos.size // 2])
        clipped = eo.counts_of(d, r, cap)
        assert (clipped < want).any() and (clipped[(r <= cap)] == want[(r <= cap)]).all()
        np.testing.assert_array_equal(clipped, eo.counts_of(d, np.minimum(r, np.float32(cap))))   # (NaN stays NaN: no hit)
        np.testing.assert_array_equal(count_each(ix, Q, r, cap=cap), clipped)
        # the pipeline count -> offsets -> list -> sort: the oracle's keys bit for bit
        for c in (INF, cap):
            lists = eo.lists_of(d, r, c, base=BASE)
            counts, off, fill, keys, _ = pipeline([ix], dev_f32(Q), dev_f32(r), M, cap=c)
            np.testing.assert_array_equal(counts, eo.lengths(lists))
            np.testing.assert_array_equal(fill, counts)
            np.testing.assert_array_equal(off, offsets_of(counts))
            assert_segments(off, keys, lists, msg=f"k={k} cap={c}")
        np.testing.assert_array_equal(ix.count_within_each_host(Q, r, cap=cap), clipped)
        o, ind, d2 = ix.list_within_each_host(Q, r)
        lists = eo.lists_of(d, r, base=BASE)
        np.testing.assert_array_equal(o, offsets_of(want).astype(np.int64))
        np.testing.assert_array_equal(ind.view(np.uint32), np.concatenate(lists).astype(np.uint32))
        np.testing.assert_array_equal(d2.view(np.uint32), (np.concatenate(lists) >> np.uint64(32)).astype(np.uint32))
    finally:
        ix.close()


@pytest.mark.parametrize("k", [3, 17])
def test_rooms_cut_short_show_in_the_cursor_and_guard_words_stay(k):
    """Even queries: segments one entry short of their count; odd queries: a NaN radius and a segment of one guard word — a word in
    front of and behind every even segment —, one more guard in front of the first segment and behind the last."""
    R, Q = batch(k, 9100 + k)
    d = v0_dist2(Q, R, k)
    r = eo.radii_of(d)
    r[1::2] = np.nan
    lists = eo.lists_of(d, r, base=BASE)
    want = eo.lengths(lists)
    assert (want[0::2] > 64).any() and (want[0::2] > 0).sum() > 8 and (want[1::2] == 0).all()
    room = np.where(np.arange(M) % 2 == 0, np.maximum(want.astype(np.int64) - 1, 0), 1)
    off = offsets_of(room) + np.uint64(1)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        fill, keys = list_each(ix, Q, r, off, keys=dev_u64(np.full(int(off[M]) + 1, PAD)))
        np.testing.assert_array_equal(fill, want)                     # every hit counted, stored or not
        assert (fill[0::2][want[0::2] > 0] > room[0::2][want[0::2] > 0]).all()
        assert keys[0] == PAD and keys[int(off[M])] == PAD
        for j in range(M):
            seg = keys[int(off[j]):int(off[j + 1])]
            if j % 2:
                assert seg.size == 1 and seg[0] == PAD, j
            else:
                assert np.unique(seg).size == seg.size == room[j] and np.isin(seg, lists[j]).all(), j
    finally:
        ix.close()


def test_two_chunks_of_queries_advance_the_radii():
    """m = 65536 + 70: the first chunk's queries are 1024 copies of 64, so the oracle is evaluated for those 64 and for the second
    chunk; the second chunk's kinds start elsewhere in the cycle."""
    k, n, m1, m2 = 3, 1100, 65536, 70
    R, Qa = batch(k, 9200, n=n, m=64 + m2)
    Q1, Q2 = Qa[:64], Qa[64:]
    d1, d2 = v0_dist2(Q1, R, k), v0_dist2(Q2, R, k)
    r1, r2 = eo.radii_of(d1), eo.radii_of(d2, first_kind=4)
    Q = np.concatenate([np.tile(Q1, (m1 // 64, 1)), Q2])
    r = np.concatenate([np.tile(r1, m1 // 64), r2])
    eo.assert_every_kind_of_count(eo.counts_of(d2, r2))
    eo.assert_no_shared_radius_passes(d1, r1)
    eo.assert_no_shared_radius_passes(d2, r2)
    eo.assert_a_stale_pointer_fails(d2, r2, r[:m2])
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        counts, off, fill, keys, _ = pipeline([ix], dev_f32(Q), dev_f32(r), m1 + m2)
        w1, w2 = eo.lists_of(d1, r1, base=BASE), eo.lists_of(d2, r2, base=BASE)
        np.testing.assert_array_equal(counts[:m1].reshape(-1, 64), np.tile(eo.lengths(w1), (m1 // 64, 1)))
        np.testing.assert_array_equal(counts[m1:], eo.lengths(w2))
        np.testing.assert_array_equal(fill, counts)
        assert_segments(off, keys, w1, msg="first chunk")
        assert_segments(off[m1 - 64:], keys, w1, msg="end of the first chunk")
        assert_segments(off[m1:], keys, w2, msg="second chunk")
    finally:
        ix.close()


def test_two_index_range_shards_fold_into_one_count_array_and_one_key_buffer():
    k = 16
    R, Q = batch(k, 9300)
    d = v0_dist2(Q, R, k)
    r = eo.radii_of(d, first_kind=2)
    lists = eo.lists_of(d, r, base=BASE)
    eo.assert_every_kind_of_count(eo.lengths(lists))
    a, b = pkg.KnnIndex(k, R[:1500], base_index=BASE), pkg.KnnIndex(k, R[1500:], base_index=BASE + 1500)
    try:
        counts, off, fill, keys, _ = pipeline([a, b], dev_f32(Q), dev_f32(r), M)
        np.testing.assert_array_equal(counts, eo.lengths(lists))
        np.testing.assert_array_equal(fill, counts)
        assert_segments(off, keys, lists)
    finally:
        a.close()
        b.close()


def test_a_cell_range_shard_pair_folds_and_its_keys_carry_gids():
    rng = np.random.default_rng(9400)
    k, n, m = 16, (1 << 19) + 5, 40
    R = rng.random((n, k), dtype=np.float32)
    Q = rng.random((m, k), dtype=np.float32)
    Q[:, 0] += np.linspace(0.0, 1.5, m, dtype=np.float32)
    d = v0_dist2(Q, R, k)
    r = eo.radii_of(d, kinds=[x for x in eo.KINDS if x != "inf"])   # (no list of half a million keys to sort)
    lists = eo.lists_of(d, r)          # the keys carry global row numbers: the ranks' gids
    eo.assert_every_kind_of_count(eo.lengths(lists))
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=False)
    try:
        counts, off, fill, keys, stats = pipeline(sh.idx, dev_f32(Q), dev_f32(r), m)
        assert all(st[0] == 1 for st in stats), stats
        np.testing.assert_array_equal(counts, eo.lengths(lists))
        np.testing.assert_array_equal(fill, counts)
        assert_segments(off, keys, lists)
    finally:
        sh.close()
