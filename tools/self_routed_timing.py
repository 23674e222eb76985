#!/usr/bin/env python3
"""The radius graph on the grid and cell-pruned ways (knn_index_self_count_within_routed, knn_index_self_list_within_routed) against
the existing self calls and against the plain routed calls on the SAME index and the same build, ms per call, timed with stream
events around windows of calls.

Cases (n = 2^20, uniform rows, knn_synth_fill_device with seed 1001 as bench.py; rows = 1024 and 65536 from local row 4099):
  fp16   k 16, options cells 1, cells_rows 1, cells_centre 2: the fp16 one-frame layout, KNN_QUERY_COUNT_CELLS
  bins   k 16, options cells 1, cells_rows 2, cells_u8_frame 2: 8-bit rows in bin frames (the 8-bit layout the plain cell way
         serves), KNN_QUERY_COUNT_CELLS
  grid   k 3, KNN_QUERY_COUNT_GRID: the grid index
The radius is made by the library itself, on the device: knn_index_self_topk (K = 16) of the first 1024 rows ->
knn_keys_column_dist2 (column 15), its median — a mean of about 16 hits per row, the h16 class of profiles/list_within_timing.txt.
Three forms per (case, rows), count and list each, alternating in one process:
  routed   the routed self calls with the case's flag
  self     knn_index_self_count_within / knn_index_self_list_within, the exact self-scan: tools/isa_same.py shows these kernels
           unchanged from the parent commit, so this column is the parent's figure
  plain    knn_index_count_within / knn_index_list_within with the same flag and the same rows as queries (the resident rows'
           own address): the floor — every row counts and lists itself too, the self forms add only the drop
Per form: warm-ups, then `reps` windows of `calls` calls; median, minimum and the spread (largest - smallest window) / median.
`same` = the routed counts and fills equal the self form's, and the plain counts are exactly one more per row (the row itself).
Every case runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: self_routed_timing.py [--reps R] [--calls C] [--warmup W] [--cases fp16 ...] [--rows 1024 65536] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

LOG2N, K, FIRST = 20, 16, 4099
CASES = {
    "fp16": (16, {"cells": 1, "cells_rows": 1, "cells_centre": 2}, {"cells": True}),
    "bins": (16, {"cells": 1, "cells_rows": 2, "cells_u8_frame": 2}, {"cells": True}),
    "grid": (3, {}, {"grid": True}),
}


def step(case, rows, reps, calls, warmup):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    k, opts, flag = CASES[case]
    n, m = 1 << LOG2N, rows
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    torch.cuda.synchronize()
    for o, v in opts.items():
        pkg.set_option(o, v)
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    q_ptr = R.data_ptr() + FIRST * k * 4          # the window's rows as the plain calls' queries

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        for _ in range(calls):
            fn()
        b.record(ts)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    def timed(forms):
        for _ in range(warmup):
            for f in forms:
                f()
        torch.cuda.synchronize()
        t, stats = [[] for _ in forms], [None for _ in forms]
        for _ in range(reps):
            for g, f in enumerate(forms):
                t[g].append(window(f))
                stats[g] = ix.last_stats()
        return [(round(float(np.median(x)), 4), round(min(x), 4), round((max(x) - min(x)) / float(np.median(x)), 3)) for x in t], stats

    def i32(count):
        return torch.empty(count, dtype=torch.int32, device=dev)

    try:
        keys = torch.empty(1024 * K, dtype=torch.int64, device=dev)
        kth = torch.empty(1024, dtype=torch.float32, device=dev)
        ix.self_topk(FIRST, 1024, K, keys.data_ptr(), stream=stream, init_keys=True)
        pkg.keys_column_dist2(keys.data_ptr(), 1024, K, K - 1, kth.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        r2 = float(kth.median().item())
        c = [i32(m) for _ in range(3)]
        count_forms = [lambda: ix.self_count_within_routed(FIRST, m, c[0].data_ptr(), cap=r2, stream=stream, init=True, **flag),
                       lambda: ix.self_count_within(FIRST, m, r2, c[1].data_ptr(), stream=stream, init=True),
                       lambda: ix.count_within(m, q_ptr, r2, c[2].data_ptr(), stream=stream, init=True, **flag)]
        ct, cstats = timed(count_forms)
        off = [torch.empty(m + 1, dtype=torch.int64, device=dev) for _ in range(3)]
        for g in range(3):
            pkg.counts_to_offsets(c[g].data_ptr(), m, off[g].data_ptr(), stream=stream)
        torch.cuda.synchronize()
        total = [int(o[m].item()) for o in off]
        fill = [i32(m) for _ in range(3)]
        buf = [torch.empty(max(t, 1), dtype=torch.int64, device=dev) for t in total]
        list_forms = [lambda: ix.self_list_within_routed(FIRST, m, off[0].data_ptr(), fill[0].data_ptr(), buf[0].data_ptr(), cap=r2,
                                                         stream=stream, init=True, **flag),
                      lambda: ix.self_list_within(FIRST, m, r2, off[1].data_ptr(), fill[1].data_ptr(), buf[1].data_ptr(),
                                                  stream=stream, init=True),
                      lambda: ix.list_within(m, q_ptr, r2, off[2].data_ptr(), fill[2].data_ptr(), buf[2].data_ptr(), stream=stream,
                                             init=True, **flag)]
        lt, lstats = timed(list_forms)
        cr, cs, cp = (x.cpu().numpy().view(np.uint32) for x in c)
        fr, fs, fp = (x.cpu().numpy().view(np.uint32) for x in fill)
        same = bool((cr == cs).all() and (fr == cr).all() and (fs == cs).all() and (cp == cs + 1).all() and (fp == cp).all())
        print(json.dumps(dict(case=case, k=k, n=n, rows=m, radius=r2, hits=round(float(cs.mean()), 2), count=ct, list=lt, total=total,
                              count_stats=cstats, list_stats=lstats, same=same)), flush=True)
    finally:
        ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per form")
    ap.add_argument("--calls", type=int, default=10, help="calls per window at 1024 rows (65536 rows: a fifth of that, at least 2)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--rows", nargs="*", type=int, default=[1024, 65536])
    ap.add_argument("--limit", type=int, default=240, help="seconds a case's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--step-rows", type=int, default=1024, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.step_rows, a.reps, a.calls, a.warmup)
    rows, rc = [], 0
    for case, m in [(c, m) for c in a.cases for m in a.rows]:   # one child at a time, each under its own limit; a failure ends the run
        calls = a.calls if m <= 1024 else max(2, a.calls // 5)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", case, "--step-rows", str(m), "--reps",
               str(a.reps), "--calls", str(calls), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("case %s rows %d ended with status %d: stopping" % (case, m, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/self_routed_timing.py: n = 2^%d, uniform rows, one MI355X, one call at a time, ms per call: median / minimum / spread"
             " ((largest - smallest) / median) of %d windows of %d calls (65536 rows: %d), %d warm-ups, events around the window"
             % (LOG2N, a.reps, a.calls, max(2, a.calls // 5), a.warmup),
             "# radius = the median %d-th neighbour distance of rows %d .. %d (knn_index_self_topk -> knn_keys_column_dist2): hits ="
             " the mean count per row" % (K, FIRST, FIRST + 1023),
             "# routed = knn_index_self_count_within_routed / _list_within_routed with the case's flag; self = knn_index_self_count_within /"
             " _list_within (the exact self-scan: kernels unchanged from the parent commit, so the parent's figure);",
             "# plain = knn_index_count_within / _list_within with the same flag and the same rows as queries (the floor: each row lists"
             " itself too).  stats = knn_index_last_stats of the routed list call ([0] the way, [2] != 0: gave up / fell back)",
             "%-5s %2s %6s %11s %6s | %-24s %-24s %-24s | %-24s %-24s %-24s | %-16s %4s" % (
                 "case", "k", "rows", "radius", "hits", "count routed", "count self", "count plain", "list routed", "list self",
                 "list plain", "stats", "same")]
    fmt = lambda t: "%.4f / %.4f / %.3f" % tuple(t)   # noqa: E731
    for r in rows:
        lines.append("%-5s %2d %6d %11.6g %6.2f | %-24s %-24s %-24s | %-24s %-24s %-24s | %-16s %4s" % (
            r["case"], r["k"], r["rows"], r["radius"], r["hits"], fmt(r["count"][0]), fmt(r["count"][1]), fmt(r["count"][2]),
            fmt(r["list"][0]), fmt(r["list"][1]), fmt(r["list"][2]), str(r["list_stats"][0]), "yes" if r["same"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if all(r["same"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
