#!/usr/bin/env python3
"""Counts and lists within a radius over a subset of the rows on the cell-pruned scan and on the grid index
(knn_index_count_within_masked_routed, knn_index_list_within_masked_routed) against the exact masked scan and against the unmasked
pruned calls on the SAME index in the same run, ms per call, timed with stream events around windows of calls.

Cases (n = 2^20 uniform rows, m = 1024 queries, knn_synth_fill_device with seeds 1001 / 1000 as bench.py):
  cells  k 16, options cells 1, cells_rows 1, cells_centre 2: the fp16 one-frame layout, KNN_QUERY_COUNT_CELLS
  grid   k 3, KNN_QUERY_COUNT_GRID: the grid index
The radius is made by the library itself, on the device: knn_index_query_topk (K = 20) -> knn_keys_column_dist2 (column 19), its
median — about 20 unmasked hits a query.
Masks: all ones; a random half; a random 1/16; one contiguous range of 1/16 of the rows starting at an odd row.
Three forms per (case, mask), count and list each, alternating in one process:
  exact     knn_index_count_within_masked / knn_index_list_within_masked: the exact masked scan, what a masked range query cost
  routed    the routed masked calls with the case's flag
  unmasked  knn_index_count_within / knn_index_list_within with the same flag: the same walk without the bit test (it answers
            another question — the hits among ALL rows — and its time does not depend on the mask)
Per form: warm-ups, then `reps` windows of `calls` calls; median, minimum and the spread (largest - smallest window) / median.
ratio = routed median / unmasked median, to be read beside the unmasked form's spread.  `same` = the routed counts and fills equal
the exact masked form's and, after knn_keys_sort_segments on both (outside the timed windows), so do the listed keys.  stats =
knn_index_last_stats of the routed list call ([0] the way, [2] != 0: gave up / fell back).
Every case runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: masked_routed_timing.py [--reps R] [--calls C] [--warmup W] [--cases cells grid] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

LOG2N, M, K = 20, 1024, 20
CASES = {
    "cells": (16, {"cells": 1, "cells_rows": 1, "cells_centre": 2}, {"cells": True}),
    "grid": (3, {}, {"grid": True}),
}
MASKS = ("ones", "random 1/2", "random 1/16", "range 1/16")


def step(case, reps, calls, warmup):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    k, opts, flag = CASES[case]
    n, m = 1 << LOG2N, M
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    Q = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(Q.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    for o, v in opts.items():
        pkg.set_option(o, v)
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    rng = np.random.default_rng(21)

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

    def bits_of(name):
        bits = np.zeros(n, dtype=bool)
        if name == "ones":
            bits[:] = True
        elif name.startswith("random"):
            bits[rng.permutation(n)[:n // int(name.split("/")[1])]] = True
        else:
            T = n // 16
            start = (n - T) // 3 | 1
            bits[start:start + T] = True
        return bits

    try:
        keys = torch.empty(m * K, dtype=torch.int64, device=dev)
        kth = torch.empty(m, dtype=torch.float32, device=dev)
        ix.query_topk(m, K, Q.data_ptr(), keys.data_ptr(), stream=stream, init_keys=True)
        pkg.keys_column_dist2(keys.data_ptr(), m, K, K - 1, kth.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        r2 = float(kth.median().item())
        q = Q.data_ptr()
        for name in MASKS:
            bits = bits_of(name)
            words = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy()).to(dev)
            w = words.data_ptr()
            c = [i32(m) for _ in range(3)]
            count_forms = [lambda: ix.count_within_masked(m, q, r2, w, c[0].data_ptr(), stream=stream, init=True),
                           lambda: ix.count_within_masked_routed(m, q, r2, w, c[1].data_ptr(), stream=stream, init=True, **flag),
                           lambda: ix.count_within(m, q, r2, c[2].data_ptr(), stream=stream, init=True, **flag)]
            ct, _ = timed(count_forms)
            off = [torch.empty(m + 1, dtype=torch.int64, device=dev) for _ in range(3)]
            for g in range(3):
                pkg.counts_to_offsets(c[g].data_ptr(), m, off[g].data_ptr(), stream=stream)
            torch.cuda.synchronize()
            total = [int(o[m].item()) for o in off]
            fill = [i32(m) for _ in range(3)]
            buf = [torch.empty(max(t, 1), dtype=torch.int64, device=dev) for t in total]
            list_forms = [lambda: ix.list_within_masked(m, q, r2, w, off[0].data_ptr(), fill[0].data_ptr(), buf[0].data_ptr(),
                                                        stream=stream, init=True),
                          lambda: ix.list_within_masked_routed(m, q, r2, w, off[1].data_ptr(), fill[1].data_ptr(), buf[1].data_ptr(),
                                                               stream=stream, init=True, **flag),
                          lambda: ix.list_within(m, q, r2, off[2].data_ptr(), fill[2].data_ptr(), buf[2].data_ptr(), stream=stream,
                                                 init=True, **flag)]
            lt, lstats = timed(list_forms)
            ce, cr, cu = (x.cpu().numpy().view(np.uint32) for x in c)
            fe, fr, fu = (x.cpu().numpy().view(np.uint32) for x in fill)
            for g in range(2):   # the exact and the routed lists, sorted: the same keys in every segment
                pkg.keys_sort_segments(m, off[g].data_ptr(), fill[g].data_ptr(), buf[g].data_ptr(), stream=stream)
            torch.cuda.synchronize()
            keys_same = total[0] == total[1] and bool((buf[0][:total[0]] == buf[1][:total[1]]).all().item())
            same = bool((cr == ce).all() and (fr == cr).all() and (fe == ce).all() and (fu == cu).all() and (cr <= cu).all() and keys_same)
            print(json.dumps(dict(case=case, k=k, mask=name, admitted=int(bits.sum()), radius=r2, hits=round(float(cu.mean()), 2),
                                  kept=round(float(cr.mean()), 2), count=ct, list=lt, stats=lstats[1], same=same)), flush=True)
    finally:
        ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per form")
    ap.add_argument("--calls", type=int, default=10, help="calls per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--limit", type=int, default=240, help="seconds a case's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.calls, a.warmup)
    rows, rc = [], 0
    for case in a.cases:   # one child at a time, each under its own limit; a failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", case, "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("case %s ended with status %d: stopping" % (case, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/masked_routed_timing.py: n = 2^%d, m = %d, uniform rows, one MI355X, one call at a time, ms per call: median /"
             " minimum / spread ((largest - smallest) / median) of %d windows of %d calls, %d warm-ups, events around the window"
             % (LOG2N, M, a.reps, a.calls, a.warmup),
             "# radius = the median %d-th neighbour distance of the queries (knn_index_query_topk -> knn_keys_column_dist2): hits = the"
             " mean unmasked count per query, kept = the mean masked count" % K,
             "# exact = knn_index_count_within_masked / _list_within_masked (the exact masked scan); routed ="
             " knn_index_count_within_masked_routed / _list_within_masked_routed with the case's flag;",
             "# unmasked = knn_index_count_within / _list_within with the same flag (the same walk without the bit test).  ratio ="
             " routed / unmasked medians, count and list; read it beside the unmasked spread.  stats = knn_index_last_stats of the"
             " routed list call",
             "%-5s %2s %-11s %8s %11s %6s %6s | %-24s %-24s %-24s | %-24s %-24s %-24s | %-11s | %-14s %4s" % (
                 "case", "k", "mask", "admitted", "radius", "hits", "kept", "count exact", "count routed", "count unmasked", "list exact",
                 "list routed", "list unmasked", "ratio", "stats", "same")]
    fmt = lambda t: "%.4f / %.4f / %.3f" % tuple(t)   # noqa: E731
    for r in rows:
        lines.append("%-5s %2d %-11s %8d %11.6g %6.2f %6.2f | %-24s %-24s %-24s | %-24s %-24s %-24s | %.3f %.3f | %-14s %4s" % (
            r["case"], r["k"], r["mask"], r["admitted"], r["radius"], r["hits"], r["kept"], fmt(r["count"][0]), fmt(r["count"][1]),
            fmt(r["count"][2]), fmt(r["list"][0]), fmt(r["list"][1]), fmt(r["list"][2]), r["count"][1][0] / r["count"][2][0],
            r["list"][1][0] / r["list"][2][0], str(r["stats"]), "yes" if r["same"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if rows and all(r["same"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
