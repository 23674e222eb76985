"""The match kernel's queue on the group minima: the lists it writes, entry for entry, and the answers behind them.

Pass 1 of knn_cells_match_kernel queues a query for a block of 64 cells iff the smallest of the block's 64 low-table entries passes
the list test; pass 2, the list test itself, is what it was.  So every list must be what the list test alone gives: here each
batch's lists are fetched from the slot (knn_debug_cells_fetch) and compared with the lists worked out in numpy from the tables
the launch read — `!(lo[q][l] + hi[h][q] > Dup_q)` in fp32.  A list follows the block's queue, and the queue takes the waves' chunks of the batch in
the order the waves reach its LDS counter: the ORDER of a list is not fixed from launch to launch, its members are.  So a list
within its room is compared as a sorted set; a list over its room (the scan then scores the cell against the whole batch and
reads only the length) must hold `room` distinct listed queries.  The group minima are checked against the low table they were
taken from.

Answers: 1-NN against the CPU oracle (tests/oracle_lib.py), bit-exact.  The oracle library has no top-K and no count: those two
calls are held to the numpy restatement of its v0 arithmetic (tests/topk_oracle.py, tests/count_oracle.py), whose first column is
checked against the oracle's own keys here.

Shapes: n = 2^17 rows is the smallest shard with a cell-sorted layout (512 cells: the 16-wave form of the kernel, a low table of
more than one group); m = 1024 fills every chunk of pass 1, m = 77 leaves a ragged second chunk; 2^23 rows give 2^15 cells, the
8-wave form; rank 1 of two cell-range shards has a cell_base that is not zero and part of the high table only."""
import os

import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import count
from tests.count_oracle import counts_of
from tests.shards_helper import Shards
from tests.topk_oracle import keys_dist2, v0_dist2
from tests.within_helper import plain

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
K16, N17, M = 16, 1 << 17, 1024
# a one-frame fp16 layout from 2^17 rows, lists from the match launch (one batch at a time on few cells the scan would list its own)
OPTIONS = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2, "cells_lists": 1, "topk_cells": 1}
F = np.float32


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    for o, v in OPTIONS.items():
        pkg.set_option(o, v)
    yield
    for o in OPTIONS:
        pkg.set_option(o, 0)


def _batch(dist):
    rng = np.random.default_rng(len(dist) + 170)
    if dist == "uniform":
        R, Q = rng.random((N17, K16), dtype=F), rng.random((M, K16), dtype=F)
    elif dist == "gaussian":          # most rows and queries in the middle bins: long lists, cells with more queries than room
        R, Q = rng.normal(0, 1, (N17, K16)).astype(F), rng.normal(0, 1, (M, K16)).astype(F)
    elif dist == "copies":            # 1024 copies of one query: the cells that list it list the whole batch
        R, Q = rng.random((N17, K16), dtype=F), np.tile(rng.random((1, K16), dtype=F), (M, 1))
    else:
        raise ValueError(dist)
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


_REF = {}


def _reference(dist, oracle):
    """Per distribution, once: the batch, the oracle's 1-NN keys and, from the numpy restatement, the 8 nearest keys of every query
    and a radius (the median 8-th nearest distance) with its counts.  Read-only."""
    if dist not in _REF:
        Q, R = _batch(dist)
        nn = oracle.v0_keys(K16, Q, R, threads=THREADS)
        top = np.empty((M, 8), dtype=np.uint64)
        d8 = []
        for c0 in range(0, M, 64):
            d = v0_dist2(Q[c0:c0 + 64], R, K16)
            keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N17, dtype=np.uint64)[None, :]
            top[c0:c0 + 64] = np.sort(np.partition(keys, 7, axis=1)[:, :8], axis=1)
            d8.append(d)
        r2 = float(np.median(keys_dist2(top[:, 7])))
        cnt = np.concatenate([counts_of(d, r2) for d in d8])
        np.testing.assert_array_equal(top[:, 0], nn)          # the restatement agrees with the oracle where the oracle speaks
        for a in (Q, R, nn, top, cnt):
            a.setflags(write=False)
        _REF[dist] = dict(Q=Q, R=R, nn=nn, top=top, r2=r2, cnt=cnt)
    return _REF[dist]


def _nearest(ix, Q):
    Qf = np.array(Q, dtype=F).reshape(-1)      # (a copy: the reference batches are read-only)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to("cuda:0")
    keys = torch.empty(m, dtype=torch.int64, device="cuda:0")
    ix.query_keys(m, q_d.data_ptr(), keys.data_ptr(), init_keys=True)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


def _check_lists(ix, m, what):
    """The slot's lists against the list test alone, worked out from the tables the match launch read; the group minima against
    the low table.  Returns what was fetched."""
    t = ix.debug_cells_fetch(m, tables=True)
    ncells, cap, nl = t["ncells"], t["cap"], t["nl"]
    lo, hi, dup = t["lo"][:m], t["hi"][:, :m], t["dup"][:m]
    np.testing.assert_array_equal(t["lo_min"][:, :m], lo.reshape(m, nl // 64, 64).min(axis=2).T, err_msg=f"{what}: group minima")
    cells = np.arange(ncells)
    with np.errstate(invalid="ignore", over="ignore"):
        listed = ~((lo[:, cells & (nl - 1)].T + hi[cells // nl]).astype(F) > dup[None, :])      # [cell][query]
    np.testing.assert_array_equal(t["counts"], listed.sum(axis=1), err_msg=f"{what}: list lengths")
    for c in np.flatnonzero(t["counts"]):
        keep = min(int(t["counts"][c]), cap)
        got = np.sort(t["lists"][c, :keep])
        if keep == t["counts"][c]:
            np.testing.assert_array_equal(got, np.flatnonzero(listed[c]), err_msg=f"{what}: list of cell {c}")
        else:
            assert (np.diff(got.astype(np.int64)) > 0).all() and listed[c][got].all(), f"{what}: cut list of cell {c}"
    assert t["counts"].any(), what
    return t


@pytest.mark.parametrize("dist", ["uniform", "gaussian", "copies"])
def test_lists_and_answers(oracle, dist):
    ref = _reference(dist, oracle)
    Q, R = ref["Q"], ref["R"]
    ix = pkg.KnnIndex(K16, R)
    try:
        for m in (M, 77):
            got = _nearest(ix, Q[:m])
            st = ix.last_stats()
            assert st[0] == 4, st
            np.testing.assert_array_equal(got, ref["nn"][:m], err_msg=f"{dist} m={m} 1-NN {st}")
            t = _check_lists(ix, m, f"{dist} m={m} 1-NN")
            print(f"{dist} m={m}: {t['ncells']} cells, room {t['cap']}, low table {t['nl']}; list length mean {t['counts'].mean():.1f} "
                  f"max {t['counts'].max()}; cells over their room {(t['counts'] > t['cap']).sum()}; stats {st}")
        # top-K (K = 8) and a count within the median 8-th nearest distance: other prep forms in front of the same match launch
        np.testing.assert_array_equal(plain(ix, Q, 8), ref["top"], err_msg=f"{dist} top-8")
        assert ix.last_stats()[0] == 4, ix.last_stats()
        _check_lists(ix, M, f"{dist} top-8")
        np.testing.assert_array_equal(count(ix, Q, ref["r2"], cells=True), ref["cnt"], err_msg=f"{dist} count")
        assert ix.last_stats()[0] == 4, ix.last_stats()
        _check_lists(ix, M, f"{dist} count")
    finally:
        ix.close()


def test_cell_range_shard(oracle):
    """Rank 1 of two cell-range shards of 2^18 rows: its cells start at a cell_base that is not zero and its high table is a part
    of the grid's, so a group index taken from the wrong cell number shows here."""
    rng = np.random.default_rng(18)
    k, n, m = 16, 1 << 18, 600
    R = rng.random((n, k), dtype=F)
    Q = rng.random((m, k), dtype=F)
    want = oracle.v0(k, Q, R, threads=THREADS)
    sh = Shards(k, torch.from_numpy(R).to("cuda:0"), 2)
    try:
        got, _, stats = sh.query(Q)                     # (the minimum over both ranks' keys)
        np.testing.assert_array_equal(got, want)
        assert all(st[0] == 4 for st in stats), stats
        t = _check_lists(sh.idx[1], m, "rank 1 of 2")
        assert t["cell_base"] != 0 and t["cell_base"] % t["nl"] == 0 and t["nh"] * t["nl"] == t["ncells"], t["cell_base"]
        assert t["nh"] * t["nl"] < sh.geom.first_cell(2), (t["nh"], t["nl"])
    finally:
        sh.close()


def test_eight_wave_form(oracle):
    """2^23 rows: 2^15 cells, the 8-wave form of the kernel (every wave takes two chunks of pass 1), a ragged batch."""
    k, n, m = 16, 1 << 23, 333
    r_d = torch.empty(n * k, dtype=torch.float32, device="cuda:0")
    pkg.synth_fill_device(r_d.data_ptr(), n * k, 2301)
    Q = oracle.synth(m * k, 2300).reshape(m, k)
    ix = pkg.KnnIndex(k, r_d.data_ptr(), n_local=n, refs_on_device=True)
    try:
        got = _nearest(ix, Q)
        st = ix.last_stats()
        assert st[0] == 4 and st[2] == 0, st
        t = _check_lists(ix, m, "2^23 rows")
        assert t["ncells"] > 16384, t["ncells"]
        want = oracle.v0_keys(k, Q[:48], oracle.synth(n * k, 2301), threads=THREADS)
        np.testing.assert_array_equal(got[:48], want)
    finally:
        ix.close()
