#!/usr/bin/env python3
"""Index-resident top-K step (knn_index_query_topk) against the 1-NN step on the same index, timed with device events.

Workloads (fp32 rows from knn_synth_fill_device, seeds 1001 / 1000 as bench.py):
  c3_fullscan  k 16, m 1024, n 2^24, option cells = 2 (1-NN: the MFMA filter's full scan)
  c3_default   the same shape, library policy (1-NN: the cell-pruned scan over 8-bit rows)
  c5           k 128, m = n = 65536 (1-NN: the deep-K filter)
  c3_exact     the C3 shape with option path = 1 (1-NN: the exact kernels)
  c3_fp16      the C3 shape with option cells_rows = 1 (the fp16 cell-sorted layout)
  k20          k 20, m 1024, n 2^24, library policy
A top-K call takes the cell-pruned scan (path 4) on cell-sorted layouts in the shard's frame when option topk_cells allows it,
the MFMA filter (path 2) on the dense layouts and on fp16 cell-sorted ones otherwise, the exact top-K scan (path 1) on per-cell
frames; "rec/q" is knn_index_last_stats()[1] / m (records of 16 rows re-ranked), "fb" its [2] (1: the batch fell back to the
exact top-K).  --topk-cells V sets that option (a library without it — KNN_MI355X_LIB naming an older build — is left alone).
usage: topk_timing.py [--reps R] [--only NAME ...] [--topk-cells V] [--ks K ...]"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import torch  # noqa: E402

import multicore_hw2_amd as pkg  # noqa: E402

WORKLOADS = {
    "c3_fullscan": (16, 1024, 1 << 24, {"cells": 2}),
    "c3_default": (16, 1024, 1 << 24, {}),
    "c5": (128, 65536, 65536, {}),
    "c3_exact": (16, 1024, 1 << 24, {"path": 1}),
    "c3_fp16": (16, 1024, 1 << 24, {"cells_rows": 1}),
    "k20": (20, 1024, 1 << 24, {}),
}
KS = (1, 8, 32, 64)


def _time(fn, reps):
    s = torch.cuda.current_stream()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def run(name, reps, ks=KS):
    k, m, n, opts = WORKLOADS[name]
    for o in ("path", "cells", "cells_rows"):
        pkg.set_option(o, 0)
    for o, v in opts.items():
        pkg.set_option(o, v)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    Q = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(Q.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    rows = []
    try:
        keys1 = torch.empty(m, dtype=torch.int64, device=dev)
        one_med, one_min = _time(lambda: ix.query_keys(m, Q.data_ptr(), keys1.data_ptr(), stream=stream, init_keys=True), reps)
        one_stats = ix.last_stats()
        for K in ks:
            keys = torch.empty(m * K, dtype=torch.int64, device=dev)
            med, mn = _time(lambda: ix.query_topk(m, K, Q.data_ptr(), keys.data_ptr(), stream=stream, init_keys=True), reps)
            st = ix.last_stats()
            assert (keys.view(-1, K)[:, 0] == keys1).all().item(), "top-K column 0 differs from the 1-NN keys"
            rows.append(dict(workload=name, k=k, m=m, n=n, K=K, topk_ms=round(med, 4), topk_min_ms=round(mn, 4),
                             one_nn_ms=round(one_med, 4), one_nn_min_ms=round(one_min, 4), one_nn_path=one_stats[0],
                             one_nn_records_per_query=round(one_stats[1] / m, 2),
                             topk_path=st[0], topk_records_per_query=round(st[1] / m, 2), topk_fallback=st[2],
                             ratio=round(med / one_med, 2)))
            print(json.dumps(rows[-1]), flush=True)
    finally:
        ix.close()
        for o in ("path", "cells", "cells_rows"):
            pkg.set_option(o, 0)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--topk-cells", type=int, default=None)
    ap.add_argument("--ks", type=int, nargs="*", default=None)
    a = ap.parse_args()
    if a.topk_cells is not None and pkg.get_option("topk_cells") >= 0:
        pkg.set_option("topk_cells", a.topk_cells)
    out = []
    for name in (a.only or list(WORKLOADS)):
        out += run(name, a.reps, tuple(a.ks) if a.ks else KS)
    print("%-12s %4s %10s %5s %9s %3s %10s %6s %5s %9s" % ("workload", "K", "top-K ms", "path", "rec/q", "fb", "1-NN ms",
                                                         "x1-NN", "path", "rec/q"))
    for r in out:
        print("%-12s %4d %10.4f %5d %9.2f %3d %10.4f %6.2f %5d %9.2f" % (
            r["workload"], r["K"], r["topk_ms"], r["topk_path"], r["topk_records_per_query"], r["topk_fallback"], r["one_nn_ms"],
            r["ratio"], r["one_nn_path"], r["one_nn_records_per_query"]))


if __name__ == "__main__":
    main()
