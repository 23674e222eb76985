#!/usr/bin/env python3
"""A radius per query (knn_index_count_within_each, knn_index_list_within_each) against the scalar calls on the SAME index and the same
build, ms per call, timed with stream events around windows of calls.

Cases (m = 1024, n = 2^20, uniform rows, knn_synth_fill_device with seeds 1001 / 1000 as bench.py):
  exact   k 16, no flag: the exact count and list scans
  cells   k 16, option `cells` 1, KNN_QUERY_COUNT_CELLS: the cell-pruned way
  grid    k 3, KNN_QUERY_COUNT_GRID: the grid index
  kth     k 16, no flag: the case no scalar call answers — every query's own 8th-neighbour distance as its radius
Every radius comes from the library itself: knn_index_query_topk (K = 8) -> knn_keys_column_dist2 (column 7) on the device.
exact / cells / grid: r = the median of those distances; the scalar count and list at r against the each-calls with all radii equal
to r and cap = r — same hits, same way, so the difference is what reading the radius per query costs.
kth: the each-calls with the per-query radii (cap +INF) against what a caller does today, the scalar calls at the LARGEST of the
radii (and then filters); both total list lengths are recorded.
Per case: warm-ups of each form, then `reps` windows of `calls` calls each, the forms alternating in the same process; median and
minimum ms per call.  `same` = the each-form's counts equal the scalar form's (exact / cells / grid), or every per-query count is at
least 8 and at most the scalar count at the largest radius (kth).
Every case runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: each_radius_timing.py [--reps R] [--calls C] [--warmup W] [--cases exact ...] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

M, LOG2N, K = 1024, 20, 8
CASES = {
    "exact": (16, {}, {}),
    "cells": (16, {"cells": 1}, {"cells": True}),
    "grid": (3, {}, {"grid": True}),
    "kth": (16, {}, {}),
}


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
        return [(round(float(np.median(x)), 4), round(min(x), 4)) for x in t], stats

    def i32(count):
        return torch.empty(count, dtype=torch.int32, device=dev)

    try:
        # the radii, on the device: every query's K-th neighbour distance
        keys = torch.empty(m * K, dtype=torch.int64, device=dev)
        kth = torch.empty(m, dtype=torch.float32, device=dev)
        ix.query_topk(m, K, Q.data_ptr(), keys.data_ptr(), stream=stream, init_keys=True)
        pkg.keys_column_dist2(keys.data_ptr(), m, K, K - 1, kth.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        if case == "kth":
            r_scalar, radii, cap = float(kth.max().item()), kth, float("inf")
        else:
            r_scalar = float(kth.median().item())
            radii, cap = torch.full((m,), r_scalar, dtype=torch.float32, device=dev), r_scalar
        c = [i32(m), i32(m)]
        count_forms = [lambda: ix.count_within(m, Q.data_ptr(), r_scalar, c[0].data_ptr(), stream=stream, init=True, **flag),
                       lambda: ix.count_within_each(m, Q.data_ptr(), radii.data_ptr(), c[1].data_ptr(), cap=cap, stream=stream,
                                                    init=True, **flag)]
        ct, cstats = timed(count_forms)
        # the segments of each form's own counts, then the lists into them
        off = [torch.empty(m + 1, dtype=torch.int64, device=dev) for _ in range(2)]
        for g in range(2):
            pkg.counts_to_offsets(c[g].data_ptr(), m, off[g].data_ptr(), stream=stream)
        torch.cuda.synchronize()
        total = [int(o[m].item()) for o in off]
        fill = [i32(m), i32(m)]
        buf = [torch.empty(max(t, 1), dtype=torch.int64, device=dev) for t in total]
        list_forms = [lambda: ix.list_within(m, Q.data_ptr(), r_scalar, off[0].data_ptr(), fill[0].data_ptr(), buf[0].data_ptr(),
                                             stream=stream, init=True, **flag),
                      lambda: ix.list_within_each(m, Q.data_ptr(), radii.data_ptr(), off[1].data_ptr(), fill[1].data_ptr(),
                                                  buf[1].data_ptr(), cap=cap, stream=stream, init=True, **flag)]
        lt, lstats = timed(list_forms)
        cs, ce = (x.cpu().numpy().view(np.uint32) for x in c)
        fs, fe = (x.cpu().numpy().view(np.uint32) for x in fill)
        if case == "kth":
            same = bool((ce >= K).all() and (ce <= cs).all() and (fe == ce).all() and (fs == cs).all())
        else:
            same = bool((ce == cs).all() and (fe == ce).all() and (fs == cs).all())
        print(json.dumps(dict(case=case, k=k, n=n, m=m, radius=r_scalar, count_scalar=ct[0], count_each=ct[1], list_scalar=lt[0],
                              list_each=lt[1], total_scalar=total[0], total_each=total[1], stats_scalar=lstats[0], stats_each=lstats[1],
                              count_stats_each=cstats[1], same=same)), flush=True)
    finally:
        ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per form")
    ap.add_argument("--calls", type=int, default=10, help="calls per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--limit", type=int, default=180, help="seconds a case's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.calls, a.warmup)
    rows, rc = [], 0
    for case in a.cases:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", case, "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("case %s ended with status %d: stopping" % (case, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/each_radius_timing.py: m = %d, n = 2^%d, uniform rows, one MI355X, one call at a time, ms per call (median / minimum"
             " of %d windows of %d calls, %d warm-ups), events around the window" % (M, LOG2N, a.reps, a.calls, a.warmup),
             "# scalar = knn_index_count_within / knn_index_list_within at `radius`; each = the _each calls on the same index, alternating."
             "  exact / cells / grid: all radii = radius = the median %d-th neighbour distance, cap = radius." % K,
             "# kth: radii = every query's own %d-th neighbour distance (top-K -> knn_keys_column_dist2), cap +INF; scalar at the largest"
             " of them (what a caller does today, then filters).  keys = the total list length of the batch." % K,
             "# stats = knn_index_last_stats of the list calls, scalar / each ([0] the way, [2] != 0: gave up / fell back)",
             "%-6s %2s %12s | %-17s %-17s | %-17s %-17s | %10s %10s | %-18s %-18s %5s" % (
                 "case", "k", "radius", "count scalar", "count each", "list scalar", "list each", "keys scal.", "keys each",
                 "stats scalar", "stats each", "same")]
    fmt = lambda t: "%.4f / %.4f" % tuple(t)   # noqa: E731
    for r in rows:
        lines.append("%-6s %2d %12.6g | %-17s %-17s | %-17s %-17s | %10d %10d | %-18s %-18s %5s" % (
            r["case"], r["k"], r["radius"], fmt(r["count_scalar"]), fmt(r["count_each"]), fmt(r["list_scalar"]), fmt(r["list_each"]),
            r["total_scalar"], r["total_each"], str(r["stats_scalar"]), str(r["stats_each"]), "yes" if r["same"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if all(r["same"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
