"""Every compiled way the filters discard a row, with rows inside the error margin and queries out at the filters' reach.

A filter form is correct only if its threshold admits every row v0 could rank first (or within the first K): the error-bound
argument of knn_threshold / knn_bound_consts (knn_filter_dev.h) and its restatements for per-cell frames, 8-bit rows and bin
frames.  tests/test_parity_gpu.py checks that argument on raw scores for the dense row-order filter only; the other forms expose no
scores, so they are tested here through the public API against the CPU oracle, on the two input families of tests/margin_cases.py:

A. shells of 24 near-equidistant rows around each query (radii 1e-5 apart, fp16 score errors hundreds of times that): the order by
   score is scrambled against the order by v0 distance, so the true winner — and each member of the true top-K — must pass a
   threshold drawn from ANOTHER row's lower score.  The guard shares (v0 winner is not the score minimum; v0 top-8 is not the 8
   lowest scores) are asserted on the inputs actually used, so the family cannot go trivial unnoticed.
B. a ladder of query distances, offset h 2^e from the box middle for e = 0 .. 20 and two rungs past fp32, in four directions: the
   stretch up to and across kAmaxLimit, where a query's fp16 rounding is hundreds of cells wide and thresholds pass nearly
   everything.  Answers bit-exact on every rung; e <= 8 is in reach (no whole-shard fallback), e >= 13 out of it (fallback).

POWER, as measured (a check made once with two deliberately wrong builds of the library, not part of the suite).  Random rounding
reaches only part of the worst case the bound allows for: the v0 winner's score sits a median 10 % (k 3) to 1 % (k 600), at most
45 %, of the allowance 2 eta d above its shell's minimum.
  * Build 1: every eta term removed from knn_threshold, cell_centred_operand and knn_u8_bin_threshold.  21 of the 219 tests here
    fail: family B on the cells forms at k 3 and 5, per-cell frames at k 16 and every 8-bit form (1-NN ladder, top-K ladder, the
    mixed batch, the 1324-query call); family A on the 8-bit rows in cell frames only.
  * Build 2: only the 2 eta sqrt(Dup) term removed.  8 fail, all on the 8-bit forms (family B and the 1324-query call).
  * What passes both: the dense forms — their threshold comes from a SAMPLED row, far outside any shell, so a shell's winner
    passes whatever the margin is — and the fp16 forms in the shard's frame at k >= 16: there rho, the allowance for the matrix
    core's accumulation (about 1e-4 in frame units, itself 2^4 .. 2^10 above the measured worst case), is larger than the
    shells' random excess (at most 2e-5 at d = 0.03), so it stands in for the missing eta.
So: family A pins the answers where near-ties are decided under scrambled scores (the re-rank, the tie-break, the top-K
selection, record hand-over on every form) and catches a missing margin on 8-bit rows; against a missing or undersized eta on
fp16 rows it has NO power at these radii, and none of this catches a margin that is 1 % short.  Family B catches wrong answers
and faults of queries the filter must give up on, a give-up rule that fires in reach or fails to fire out of it, and — through
the large eta of far queries — a missing margin on the cells forms; it says nothing about how tight the thresholds are.  A test
with power over eta on fp16 rows needs rows whose rounding is adversarial, which needs the library's exact frame: see
tests/test_parity_gpu.py for the one form that exposes it.

Every dense and cells form holds "stats[2] == 0 on shells (fp16 rows), != 1 in reach, == 1 out of reach" for 1-NN; where top-K
differs it is said at _assert_reach, with the code that makes it so.  Bar everywhere: bit-exact indices and keys, no query left
out."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests import margin_cases as mc
from tests.shards_helper import Shards
from tests.test_cells_gpu import _query
from tests.test_shard_topk_gpu import _topk as _topk_flagged
from tests.test_topk_gpu import _host, _keys, _topk
from tests.topk_oracle import KEY_INIT, topk_keys

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
BASE = 1000          # index-range forms carry a non-zero base (cell-range shards carry global row numbers)
TOPK_KS = (8, 17)    # 17 crosses the 16-lane group of the selection network
FORMS = {f["name"]: f for f in mc.FORMS}


def _set(opts):
    for o, v in opts.items():
        pkg.set_option(o, v)


def _reset():
    for name in mc.OPTIONS:
        pkg.set_option(name, 0)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert os.path.exists(pkg.lib_path), "libknn_mi355x.so not built (no CPU fallback exists)"
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    _reset()
    _data.cache_clear()


def _topk_oracle(Q, R, k, K, base=0):
    """tests/topk_oracle.topk_keys over ALL rows (far queries tie over thousands of rows: no candidate set would do), the queries
    in chunks over a few threads (numpy releases the GIL)."""
    Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, k)
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda c0: topk_keys(Q[c0:c0 + 4], R, k, K, base=base, chunk=4), range(0, Q.shape[0], 4)))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=1)
def _data(k, n):
    """What the forms of one (k, rows) share: the shell case, the ladder's batches and, filled as tests ask, the oracle's answers
    for them (computed once, never changed)."""
    case = mc.make_shells(k, n, seed=1000 + k)
    rng = np.random.default_rng(77 * k + n % 1000)
    box = rng.random((64, k), dtype=np.float32)
    batches = {e: mc.rung_batch(k, e, box, rng) for e in mc.RUNGS_ALL + mc.PAST_FP32}
    mixed = np.ascontiguousarray(np.concatenate([mc.rung_queries(k, e, rng) for e in range(mc.RUNG_IN_REACH + 1)] + [box[:48]]))
    return dict(case=case, R=case["R"], box=box, batches=batches, mixed=mixed, rng=rng, want1={}, wantk={})


class Ctx:
    """One form: its options set, its index (or two cell-range shards) built, queried the way its kind is queried."""

    def __init__(self, form, oracle, base=BASE):
        self.f, self.oracle, self.k, self.n = form, oracle, form["k"], form["n"]
        self.kind = form["kind"]
        self.d = _data(self.k, self.n)
        self.R, self.case = self.d["R"], self.d["case"]
        self.apply()
        self.sh = self.ix = None
        if self.kind == "shards":
            self.base = 0
            self.sh = Shards(self.k, torch.from_numpy(self.R).to(torch.device("cuda:0")), 2, seed_tiles=1)
        else:
            self.base = base
            self.ix = pkg.KnnIndex(self.k, self.R, base_index=base)

    def apply(self):
        _reset()
        _set(self.f["opts"])
        pkg.set_option("topk_cells", 1)

    def close(self):
        (self.sh or self.ix).close()
        _reset()

    # -- batches: the LDS-tiled scan at k 128 needs 16 query tiles; a smaller batch is repeated up to 512 queries ------------------
    def _padded(self, Q):
        Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, self.k)
        m = Q.shape[0]
        if self.f["m_shell"] > m:
            Q = np.ascontiguousarray(np.resize(Q, (self.f["m_shell"], self.k)))
        return Q, m

    def one_nn(self, Q):
        """(int32 [m] indices as the device wrote them, the statistics of every index asked)."""
        Qp, m = self._padded(Q)
        if self.sh:
            got, _, stats = self.sh.query(Qp)
        else:
            got, st = _query(self.ix, Qp)
            stats = [st]
        np.testing.assert_array_equal(got, np.resize(got[:m], got.shape))     # (the repeats answer alike)
        return got[:m], stats

    def topk(self, Q, K):
        """(uint64 [m][K] keys — the ranks' flagged lists merged, on shards —, statistics)."""
        Qp, m = self._padded(Q)
        if self.sh:
            lists, stats = [], []
            for ix in self.sh.idx:
                lists.append(_topk_flagged(ix, Qp, K, partial=True))
                stats.append(ix.last_stats())
            a, b = _keys(Qp.shape[0], K, fill=lists[0]), _keys(Qp.shape[0], K, fill=lists[1])
            pkg.keys_topk_merge(a.data_ptr(), b.data_ptr(), Qp.shape[0], K)
            torch.cuda.synchronize()
            got = _host(b, Qp.shape[0], K)
        else:
            got = _topk(self.ix, Qp, K)
            stats = [self.ix.last_stats()]
        np.testing.assert_array_equal(got, np.resize(got[:m], got.shape).reshape(got.shape))
        return got[:m], stats

    # -- the oracle, once per (k, rows) and batch ----------------------------------------------------------------------------------
    def want_one_nn(self, name, Q):
        """v0's index per query of batch `name` (no base)."""
        w = self.d["want1"]
        if name not in w:
            w[name] = self.oracle.v0(self.k, Q, self.R, threads=THREADS)
        return w[name]

    def want_topk(self, name, Q):
        """The oracle's max(TOPK_KS) smallest keys per query of batch `name`, base 0."""
        w = self.d["wantk"]
        if name not in w:
            w[name] = _topk_oracle(Q, self.R, self.k, max(TOPK_KS))
        return w[name]

    def rebased(self, keys):
        """Oracle keys (base 0) as this form numbers its rows; (+INF, 0) stays what it is."""
        out = keys + np.uint64(self.base)
        out[keys == KEY_INIT] = KEY_INIT
        return out


@pytest.fixture(scope="module", params=mc.FORM_NAMES)
def ctx(request, oracle):
    c = Ctx(FORMS[request.param], oracle)
    yield c
    c.close()


# Where the contract differs from "in reach: stats[2] != 1".  A TOP-K batch has one more way into stats[2] == 1: more candidates
# than its buffers hold raise the same word (include/knn_mi355x.h, 2c: "a batch the filter cannot serve (a query nothing bounds,
# fewer than K sampled blocks with a real row, more candidates than the buffers hold) raises [2] = 1"; knn_exact.hip, "candidates
# dropped: the gated exact top-K answers the batch", and knn_cells.hip at knn_cells_records_kernel: "An over-full pass ends in
# KNN_CTL_FALLBACK there ... not in the tail kernel's listed-pairs evaluation, which is a 1-NN fold").  From rung 4 on the
# thresholds of a rung's queries pass a sizeable part of the shard, so a top-K batch in reach may end either way; its answers are
# held to the oracle all the same, and a top-K batch can never report 2.  The 1-NN claims hold for every dense and cells form.


def _paths_ok(c, stats, want_way, what):
    for st in stats:
        assert st[0] == want_way, (c.f["name"], what, st)


def _assert_reach(c, stats, e, what, topk=False):
    """The path claims: e <= 8 in reach (never the whole-shard fallback), e >= 13 out of it (always)."""
    if c.kind == "grid" or (topk and c.f["topk"] == 1):
        return      # the grid's give-up rule has its own tests; the exact top-K scan has no filter to give up
    exp = mc.expected_fallback(e)
    for st in stats:
        if topk:
            assert st[2] in (0, 1), (c.f["name"], what, e, st)      # (see above: over-full candidates raise 1 as well)
        elif exp is False:
            assert st[2] != 1, (c.f["name"], what, e, st)
        if exp is True:
            assert st[2] == 1, (c.f["name"], what, e, st)


# ---- family A ----------------------------------------------------------------------------------------------------------------------

def test_shells_one_nn(ctx):
    c = ctx
    c.apply()
    case = c.case
    if c.f["fp16"]:
        not_min, differs = mc.guard_shares(case)
        print(c.f["name"], "guard shares", not_min, differs)
        assert not_min >= mc.WINNER_NOT_MIN_FLOOR and differs >= mc.TOP8_DIFFERS_FLOOR, (not_min, differs)
    want = mc.shell_topk_keys(case, 1)[:, 0]
    want_idx = (want & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.isin(want_idx, case["members"]).all()
    got, stats = c.one_nn(case["Q"])
    print(c.f["name"], "shells 1-NN", stats)
    np.testing.assert_array_equal(got.astype(np.int64) - c.base, want_idx, err_msg=f"{c.f['name']} stats={stats}")
    _paths_ok(c, stats, c.f["one_nn"], "shells 1-NN")
    if c.kind != "grid":
        for st in stats:
            if c.f["fp16"]:
                assert st[2] == 0, (c.f["name"], st)      # a shell 16 fp16 steps wide is not "tighter than the fp16 step"
            else:
                assert st[2] != 1, (c.f["name"], st)      # (8-bit rows: coarser codes, the listed-pairs evaluation is allowed)


def test_shells_topk(ctx):
    c = ctx
    c.apply()
    want = c.rebased(mc.shell_topk_keys(c.case, max(TOPK_KS)))
    for K in TOPK_KS:
        got, stats = c.topk(c.case["Q"], K)
        print(c.f["name"], "shells top-K", K, stats)
        np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{c.f['name']} K={K} stats={stats}")
        _paths_ok(c, stats, c.f["topk"], f"shells K={K}")
        if c.f["topk"] != 1:
            # no fallback, 8-bit bin frames included: a query's candidates are its 24 shell rows and the few background rows a
            # margin of some 2 eta d adds — thousands of records in a room of 2^22 (the only way into [2] == 1 near the box)
            for st in stats:
                assert st[2] == 0 and (st[1] > 0 or c.kind == "shards"), (c.f["name"], K, st)


# ---- family B ----------------------------------------------------------------------------------------------------------------------

def test_ladder_one_nn(ctx):
    c = ctx
    c.apply()
    for e in c.f["rungs"]:
        Q = c.d["batches"][e]
        want = c.want_one_nn(("rung", e), Q)
        got, stats = c.one_nn(Q)
        print(c.f["name"], "rung", e, stats)
        np.testing.assert_array_equal(got.astype(np.int64) - c.base, want, err_msg=f"{c.f['name']} rung {e} stats={stats}")
        _paths_ok(c, stats, c.f["one_nn"], f"rung {e}")
        _assert_reach(c, stats, e, "1-NN")


def test_ladder_topk(ctx):
    c = ctx
    c.apply()
    for e in mc.RUNGS_FEW:
        Q = c.d["batches"][e]
        want = c.rebased(c.want_topk(("rung", e), Q))
        for K in TOPK_KS:
            got, stats = c.topk(Q, K)
            print(c.f["name"], "rung", e, "K", K, stats)
            np.testing.assert_array_equal(got, want[:, :K], err_msg=f"{c.f['name']} rung {e} K={K} stats={stats}")
            _paths_ok(c, stats, c.f["topk"], f"rung {e} K={K}")
            _assert_reach(c, stats, e, f"K={K}", topk=True)


def test_every_rung_in_reach_in_one_batch(ctx):
    c = ctx
    c.apply()
    Q = c.d["mixed"]
    got, stats = c.one_nn(Q)
    print(c.f["name"], "mixed", stats)
    np.testing.assert_array_equal(got.astype(np.int64) - c.base, c.want_one_nn("mixed", Q), err_msg=f"{c.f['name']} stats={stats}")
    _paths_ok(c, stats, c.f["one_nn"], "mixed")
    _assert_reach(c, stats, mc.RUNG_IN_REACH, "mixed 1-NN")
    want = c.rebased(c.want_topk("mixed", Q))
    got, stats = c.topk(Q, 8)
    print(c.f["name"], "mixed K 8", stats)
    np.testing.assert_array_equal(got, want[:, :8], err_msg=f"{c.f['name']} stats={stats}")
    _assert_reach(c, stats, mc.RUNG_IN_REACH, "mixed K=8", topk=True)


def test_past_fp32_rungs_answer_index_zero(ctx, oracle):
    """Offsets 1e20 (v0's squared difference overflows to +INF) and 3e38: no finite distance, v0 keeps index 0 — so these rungs run
    on an index with base 0, as tests/test_parity_gpu.py::test_nan_inf_and_overflow_semantics does.  The queries inside the box of
    the same batch are answered as ever."""
    c0 = ctx if ctx.kind == "shards" else Ctx(ctx.f, oracle, base=0)
    try:
        for off in mc.PAST_FP32:
            Q = c0.d["batches"][off]
            far = 4 * len(mc.directions(c0.k))
            want = c0.want_one_nn(("rung", off), Q)
            assert (want[:far] == 0).all() and len(set(want[far:])) > 40
            got, stats = c0.one_nn(Q)
            print(c0.f["name"], "offset", off, stats)
            np.testing.assert_array_equal(got, want, err_msg=f"{c0.f['name']} offset {off} stats={stats}")
            _paths_ok(c0, stats, c0.f["one_nn"], f"offset {off}")
            _assert_reach(c0, stats, off, "1-NN")
            wantk = c0.want_topk(("rung", off), Q)
            assert (wantk[:far] == KEY_INIT).all()
            gotk, stats = c0.topk(Q, 8)
            np.testing.assert_array_equal(gotk, wantk[:, :8], err_msg=f"{c0.f['name']} offset {off} K=8 stats={stats}")
            _assert_reach(c0, stats, off, "K=8", topk=True)
    finally:
        if c0 is not ctx:
            c0.close()
        ctx.apply()


def test_one_query_out_of_reach_in_the_first_pass_only(ctx):
    """1024 + 300 queries, only query 5 out of reach (rung 14).  The cell-pruned forms run passes of 1024: pass 1 falls back, pass 2
    must not — the fallback word is reset between passes — and statistics are the LAST pass's.  The dense forms run one launch
    and their give-up rule is batch-wide (knn_thr_kernel: amax is the batch's), so their call falls back as a whole; the deep-K
    forms get a shorter call (the oracle over k >= 128 is what costs)."""
    c = ctx
    c.apply()
    m = 1024 + 300 if c.k <= 32 else 130
    name = ("long", m)
    if name not in c.d["batches"]:
        rng = np.random.default_rng(c.k + 9)
        Q = rng.random((m, c.k), dtype=np.float32)
        Q[5] = mc.rung_queries(c.k, 14, rng, per_direction=1)[0]
        c.d["batches"][name] = Q
    Q = c.d["batches"][name]
    got, stats = c.one_nn(Q)
    print(c.f["name"], "long call", stats)
    np.testing.assert_array_equal(got.astype(np.int64) - c.base, c.want_one_nn(name, Q), err_msg=f"{c.f['name']} stats={stats}")
    _paths_ok(c, stats, c.f["one_nn"], "long call")
    for st in stats:
        if c.kind in ("cells", "shards"):
            assert st[2] == 0, (c.f["name"], st)
        elif c.kind == "dense":
            assert st[2] == 1, (c.f["name"], st)


@pytest.mark.parametrize("k", [20, 30])
def test_norm_in_fragment_near_the_limit_floods_and_recovers(oracle, k):
    """16 < k <= 30: the norm rides in the fragment, and a padding or out-of-box position scores the finite 65504.  For a query
    near kAmaxLimit the threshold can exceed that, so such positions become records (which the re-rank ignores: perm = ~0) and the
    slices may flood — the batch then ends in the exact evaluation of its listed pairs (stats[2] == 2), never in a wrong answer and
    never in the whole-shard fallback; the next batch of box queries is back on the filter."""
    f = FORMS[f"cells_nif_k{k}"]
    c = Ctx(f, oracle)
    try:
        box = c.d["box"]
        for e in (8, 9):
            Q = c.d["batches"][e]
            got, stats = c.one_nn(Q)
            print(f["name"], "rung", e, stats)
            np.testing.assert_array_equal(got.astype(np.int64) - c.base, c.want_one_nn(("rung", e), Q), err_msg=f"rung {e} {stats}")
            assert stats[0][0] == 4 and stats[0][2] in (0, 2), stats
            got, stats = c.one_nn(box)
            np.testing.assert_array_equal(got.astype(np.int64) - c.base, c.want_one_nn("box", box))
            assert stats[0][0] == 4 and stats[0][2] == 0, stats
    finally:
        c.close()
