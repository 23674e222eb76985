"""knn_index_count_within_masked_routed and knn_index_list_within_masked_routed on the cell-pruned scan (KNN_QUERY_COUNT_CELLS) on
the GPU against tests/each_oracle.py over tests/topk_oracle.v0_dist2 with the masked-out columns at +INF, and against the existing
masked calls.  Bar: exact counts and sorted lists; "pruned" means knn_index_last_stats()[0] == 4 and [2] == 0 — but for the one
designated fallback case (a far-away query), where the gated masked scan answers."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import each_oracle as eo
from tests import outlier_rows as orow
from tests.count_helper import dev, dev_counts, host_counts
from tests.count_oracle import radii
from tests.each_helper import dev_f32
from tests.masked_routed_helper import (assert_mask_bites, assert_same_answer, dev_words, existing_pipeline, routed_pipeline, scalar,
                                        under, want_of, words_of)
from tests.shards_helper import Shards
from tests.test_within_cells_gpu import BINS, FP16, MATRIX, N17, OPTIONS, spread_queries
from tests.topk_oracle import topk_keys, v0_dist2
from tests.within_helper import plain

pytestmark = pytest.mark.gpu
BASE = 11
M = 96
LOW = np.uint64(0xFFFFFFFF)
NIF = [c for c in MATRIX if c[0] == "nif_k20_fixed"][0]
CASES = [("fp16_k16", 16, FP16), ("bins_k16", 16, BINS), ("fp16_k8", 8, FP16), NIF]


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


def half_and_range(n, seed):
    rng_bits = np.zeros(n, dtype=bool)
    rng_bits[n // 4 + 5:3 * (n // 4) + 9] = True
    return [("half", np.random.default_rng(seed).random(n) < 0.5), ("range", rng_bits)]


@functools.lru_cache(maxsize=None)
def data(k):
    """The shard of a dimension, 96 queries, the oracle's distances and the list-sized radius: made once, left unchanged."""
    rng = np.random.default_rng(N17 + 7 * k)
    R = rng.random((N17, k), dtype=np.float32)
    Q = spread_queries(rng, M, k)
    d = v0_dist2(Q, R, k)
    for a in (R, Q, d):
        a.setflags(write=False)
    return R, Q, d, radii(d)[0][1]


def pruned(stats):
    return all(st[0] == 4 and st[2] == 0 for st in stats)


@pytest.mark.parametrize("name,k,opts", CASES, ids=[c[0] for c in CASES])
def test_every_layout_is_exact_and_pruned_under_a_random_and_a_contiguous_mask(name, k, opts):
    R, Q, d, r2 = data(k)
    cases = half_and_range(N17, 8400 + k)
    for _, bits in cases:
        assert_mask_bites(d, bits, r2)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        q_d = dev_f32(Q.copy())
        for mname, bits in cases:
            w_d = dev_words(words_of(bits))
            got = routed_pipeline([ix], q_d, [w_d], M, r2, cells=True)
            assert pruned(got[4]), (name, mname, got[4])
            assert_same_answer(got, want_of(d, bits, r2, base=BASE), existing_pipeline([ix], q_d, [w_d], M, r2), msg=f"{name} {mname}")
        # without the flag: the exact masked scan, the launches of the existing call (under the random half)
        half = cases[0][1]
        got = routed_pipeline([ix], q_d, [dev_words(words_of(half))], M, r2)
        assert all(st == [1, 0, 0, 0] for st in got[4]), got[4]
        assert_same_answer(got, want_of(d, half, r2, base=BASE), msg=f"{name} no flag")
    finally:
        ix.close()


def test_two_passes_share_one_mask():
    """m = 1024 + 96: the second pass's queries are queries 1024 .. 1119, the mask is the rows' and stays where it is.  Checked on
    the CPU first: under a mask advanced with the queries (1024 words, 32768 rows) the second pass would answer differently."""
    k, m0 = 16, 96
    R, Q0, d, r2 = data(k)
    m = 1024 + m0
    rep = np.arange(m) % m0
    bits = np.random.default_rng(8450).random(N17) < 0.5
    assert_mask_bites(d, bits, r2)
    cnt, lists = want_of(d, bits, r2, base=BASE)
    shifted = np.zeros(N17, dtype=bool)
    shifted[:N17 - 32768] = bits[32768:]
    second = rep[1024:]
    assert (want_of(d, shifted, r2)[0][second] != cnt[second]).any()
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        q_d, w_d = dev_f32(Q0[rep]), dev_words(words_of(bits))
        got = routed_pipeline([ix], q_d, [w_d], m, r2, cells=True)
        assert pruned(got[4]), got[4]
        assert_same_answer(got, (cnt[rep], [lists[j] for j in rep]), existing_pipeline([ix], q_d, [w_d], m, r2), msg="two passes")
    finally:
        ix.close()


def test_out_of_box_rows_are_listed_once_and_only_when_admitted():
    """The shard of tests/outlier_rows.py: 640 planted rows outside the filter's robust box, in pairs, every eighth pair an exact
    copy.  The mask admits the first row of every planted pair and drops the second (and admits a random half of the cluster).
    Queries beside planted rows get their hits from the out-of-box launch alone.  Query 0 sits exactly on the admitted row of a copy
    pair, query 1 exactly on the dropped row of another: each lists the admitted twin alone at distance 0."""
    k = 16
    R = orow.rows(k)
    Q0, d0 = orow.each_batch(k)
    copies = orow.copy_rows()
    on_admitted, on_dropped = int(copies[0]), int(copies[3])
    first, end = orow.planted_range()
    assert (on_admitted - first) % 2 == 0 and (on_dropped - first) % 2 == 1
    Q = Q0.copy()
    Q[0], Q[1] = R[on_admitted], R[on_dropped]
    d = np.array(d0, copy=True)
    d[:2] = v0_dist2(Q[:2], R, k)
    bits = np.random.default_rng(8460).random(N17) < 0.5
    bits[first:end:2] = True
    bits[first + 1:end:2] = False
    r2 = orow.kind_max(eo.radii_of(d0), "held", eo.KINDS)
    assert_mask_bites(d, bits, r2)
    hit = eo.hits_of(d, scalar(M, r2))[:, first:end]           # the planted hits hold admitted and dropped rows
    assert hit[:, 0::2].any() and hit[:, 1::2].any() and (hit[:orow.M_BESIDE].sum(axis=1) > 0).all()
    cnt, lists = want_of(d, bits, r2, base=BASE)
    for j, twin in ((0, on_admitted), (1, orow.twin_of(on_dropped))):
        zero = lists[j][(lists[j] >> np.uint64(32)) == 0]
        assert zero.size == 1 and int(zero[0] & LOW) == BASE + twin, (j, zero)
    _set(FP16)
    ix = pkg.KnnIndex(k, R, base_index=BASE)
    try:
        q_d, w_d = dev_f32(Q.copy()), dev_words(words_of(bits))
        got = routed_pipeline([ix], q_d, [w_d], M, r2, cells=True)
        assert pruned(got[4]) and all(st[3] > 0 for st in got[4]), got[4]      # ([3]: rows outside the robust box)
        assert_same_answer(got, (cnt, lists), existing_pipeline([ix], q_d, [w_d], M, r2), msg="out-of-box rows")
        numbers = (got[3] & LOW).astype(np.int64) - BASE
        planted = numbers[orow.is_planted(numbers)]
        assert planted.size and ((planted - first) % 2 == 0).all()
    finally:
        ix.close()


@pytest.mark.parametrize("opts", [FP16, BINS], ids=["fp16", "bins"])
def test_a_far_away_query_falls_back_to_the_gated_masked_scan_and_the_next_batch_is_pruned_again(opts):
    """The batch of tests/test_count_cells_gpu.py: a query at 1e6 that nothing bounds (and one with a NaN) raises FALLBACK; the
    pass's scratch is not committed and the gated masked scan answers, exactly and once."""
    rng = np.random.default_rng(45)
    k, m = 16, 70
    R = rng.random((N17, k), dtype=np.float32)
    R[10, 3] = np.nan
    R[20, 0] = np.inf
    R[30] = 3e38
    Q = spread_queries(rng, m, k)
    Qfar = Q.copy()
    Qfar[1] = 1e6
    Qfar[2, 5] = np.nan
    d, dfar = v0_dist2(Q, R, k), v0_dist2(Qfar, R, k)
    r2 = radii(d)[0][1]
    bits = rng.random(N17) < 0.5
    bits[[10, 20, 30]] = True
    assert_mask_bites(d, bits, r2)
    assert_mask_bites(dfar, bits, r2)
    _set(opts)
    ix = pkg.KnnIndex(k, R, base_index=4)
    try:
        w_d = dev_words(words_of(bits))
        qf_d, q_d = dev_f32(Qfar), dev_f32(Q)
        got = routed_pipeline([ix], qf_d, [w_d], m, r2, cells=True)
        assert all(st[0] == 4 and st[2] == 1 for st in got[4]), got[4]
        assert_same_answer(got, want_of(dfar, bits, r2, base=4), existing_pipeline([ix], qf_d, [w_d], m, r2), msg="fell back")
        assert got[0][1] == 0 and got[0][2] == 0
        # a folding count on the falling batch adds once
        held = np.full(m, 40, np.uint32)
        counts = dev_counts(m, fill=held)
        ix.count_within_masked_routed(m, qf_d.data_ptr(), r2, w_d.data_ptr(), counts.data_ptr(), cells=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 1
        np.testing.assert_array_equal(host_counts(counts), held + got[0])
        got = routed_pipeline([ix], q_d, [w_d], m, r2, cells=True)
        assert pruned(got[4]), got[4]
        assert_same_answer(got, want_of(d, bits, r2, base=4), msg="the next batch")
    finally:
        ix.close()


def test_a_cell_range_shard_pair_takes_local_masks_carries_gids_and_folds_to_the_global_answer():
    rng = np.random.default_rng(26)
    k, n, m = 16, (1 << 19) + 5, 40
    R = rng.random((n, k), dtype=np.float32)
    Q = spread_queries(rng, m, k)
    d = v0_dist2(Q, R, k)
    r2 = radii(d)[0][1]
    gbits = rng.random(n) < 0.5                          # the mask over the GLOBAL rows
    assert_mask_bites(d, gbits, r2)
    want = want_of(d, gbits, r2)
    sh = Shards(k, torch.from_numpy(R).to(dev()), 2, attach=True)
    try:
        gids = [g.cpu().numpy().astype(np.int64) for g in sh.gids]
        local = [gbits[g] for g in gids]                 # each rank's mask, in its LOCAL row order
        assert all(not np.array_equal(g, np.arange(g.size)) for g in gids[1:])      # a gid is not the local row number
        assert not np.array_equal(local[1], gbits[:local[1].size])
        masks_d = [dev_words(words_of(b)) for b in local]
        q_d = dev_f32(Q.copy())
        got = routed_pipeline(sh.idx, q_d, masks_d, m, r2, cells=True)
        assert pruned(got[4]), got[4]
        assert_same_answer(got, want, existing_pipeline(sh.idx, q_d, masks_d, m, r2), msg="shard pair")
        # each rank alone: its own admitted rows, numbered by gid
        for rank, ix in enumerate(sh.idx):
            alone = routed_pipeline([ix], q_d, [masks_d[rank]], m, r2, cells=True)
            assert_same_answer(alone, want_of(d[:, gids[rank]], local[rank], r2, gids=gids[rank]), msg=f"rank {rank}")
    finally:
        sh.close()


def test_one_call_of_every_kind_in_turn_on_one_slot():
    k, K, slot = 16, 8, 3
    R, Q, d, r2 = data(k)
    bits = np.random.default_rng(8470).random(N17) < 0.5
    assert_mask_bites(d, bits, r2)
    cnt, lists = want_of(d, bits, r2)
    want_keys = topk_keys(Q, R, k, K)
    _set(FP16)
    pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R)
    q_d, w_d = dev_f32(Q.copy()), dev_words(words_of(bits))

    def one_nn():
        keys = torch.empty(M, dtype=torch.int64, device=dev())
        ix.query_keys(M, q_d.data_ptr(), keys.data_ptr(), slot=slot, init_keys=True)
        torch.cuda.synchronize()
        assert ix.last_stats()[0] == 4, ix.last_stats()
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), want_keys[:, 0])

    def top_k():
        np.testing.assert_array_equal(plain(ix, Q, K, slot=slot), want_keys)
        assert ix.last_stats()[0] == 4 and ix.last_stats()[2] == 0, ix.last_stats()

    def masked_exact():
        got = existing_pipeline([ix], q_d, [w_d], M, r2, slot=slot)
        assert all(st == [1, 0, 0, 0] for st in got[4]), got[4]
        assert_same_answer(got, (cnt, lists), msg="masked exact")

    def masked_routed():
        got = routed_pipeline([ix], q_d, [w_d], M, r2, cells=True, slot=slot)
        assert pruned(got[4]), got[4]
        assert_same_answer(got, (cnt, lists), msg="masked routed")

    try:
        for call in (one_nn, top_k, masked_exact, masked_routed, one_nn, masked_routed, top_k, masked_exact):
            call()
    finally:
        ix.close()
