#!/usr/bin/env python3
"""knn_index_count_within: the grid way and the cell-pruned way against the exact count scan on the SAME index, ms per call, timed
with stream events around windows of calls.

Cases (m = 1024, uniform rows, knn_synth_fill_device with seeds 1001 / 1000 as bench.py):
  grid20 / grid24   k 3, n 2^20 / 2^24: KNN_QUERY_COUNT_GRID against no flag
  fp16 / bins       k 16, n 2^24 on the fp16 one-frame layout (cells_rows 1, cells_centre 2) and on 8-bit rows in bin frames
                    (cells_rows 2, cells_u8_frame 2): KNN_QUERY_COUNT_CELLS against no flag
Radii, taken over the first 32 queries from v0's arithmetic restated with torch's element-wise float32 kernels on the device (a
2^24-row oracle on the host takes minutes): the median 1-NN distance ("1nn") and the medians of the 10th and of the 100th nearest
distance ("c10", "c100": the radii at which the median query's count is about 10 and about 100).
Per (case, radius): warm-ups of each form, then `reps` windows of `calls` calls each, the two forms alternating in the same process;
the table gives each form's median and minimum ms per call, knn_index_last_stats of the fast form (records per query = [1] / m,
[2] != 0: the batch gave up / fell back), and whether the two forms' counts are equal and equal the restatement's on the 32 queries.
Every case runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: count_within_timing.py [--reps R] [--calls C] [--warmup W] [--cases grid20 ...] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

M = 1024
QUANT = 32   # queries the radii are taken from
CASES = {
    "grid20": (3, 20, {}, "grid"),
    "grid24": (3, 24, {}, "grid"),
    "fp16": (16, 24, {"cells_rows": 1, "cells_centre": 2}, "cells"),
    "bins": (16, 24, {"cells_rows": 2, "cells_u8_frame": 2}, "cells"),
}


def _nearest_and_counts(torch, q, r, k, T, radii=None, chunk=1 << 20):
    """The T smallest v0 distances of each query (float32 [m][T], ascending) — one rounding per operation, never fused — or, with
    `radii`, the counts [len(radii)][m] of rows with a finite distance <= each radius."""
    best = torch.full((q.shape[0], T), float("inf"), dtype=torch.float32, device=q.device)
    cnt = torch.zeros((len(radii or ()), q.shape[0]), dtype=torch.int64, device=q.device)
    for r0 in range(0, r.shape[0], chunk):
        rc = r[r0:r0 + chunk]
        d = torch.zeros((q.shape[0], rc.shape[0]), dtype=torch.float32, device=q.device)
        for j in range(k):
            diff = q[:, j:j + 1] - rc[None, :, j]
            sq = diff * diff
            d = d + sq
        d[~(d < float("inf"))] = float("inf")
        if radii is None:
            part = torch.topk(d, min(T, rc.shape[0]), dim=1, largest=False).values
            best = torch.sort(torch.cat([best, part], dim=1), dim=1).values[:, :T]
        else:
            for i, r2 in enumerate(radii):
                cnt[i] += ((d < float("inf")) & (d <= r2)).sum(dim=1)
        del d
    return best if radii is None else cnt


def step(case, reps, calls, warmup):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    k, log2n, opts, way = CASES[case]
    n, m = 1 << log2n, M
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
    flag = dict(grid=True) if way == "grid" else dict(cells=True)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        for _ in range(calls):
            fn()
        b.record(ts)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    try:
        near = _nearest_and_counts(torch, Q.view(m, k)[:QUANT], R.view(n, k), k, 128).cpu().numpy()
        radii = [("1nn", float(np.median(near[:, 0]))), ("c10", float(np.median(near[:, 9]))), ("c100", float(np.median(near[:, 99])))]
        want = _nearest_and_counts(torch, Q.view(m, k)[:QUANT], R.view(n, k), k, 0, radii=[r2 for _, r2 in radii]).cpu().numpy()
        for i, (label, r2) in enumerate(radii):
            out = [torch.empty(m, dtype=torch.int32, device=dev) for _ in range(2)]
            forms = [lambda: ix.count_within(m, Q.data_ptr(), r2, out[0].data_ptr(), stream=stream, init=True),
                     lambda: ix.count_within(m, Q.data_ptr(), r2, out[1].data_ptr(), stream=stream, init=True, **flag)]
            for _ in range(warmup):
                for f in forms:
                    f()
            torch.cuda.synchronize()
            t = [[], []]
            stats = [None, None]
            for _ in range(reps):
                for g in range(2):
                    t[g].append(window(forms[g]))
                    stats[g] = ix.last_stats()
            c = [o.cpu().numpy().view(np.uint32) for o in out]
            row = dict(case=case, k=k, n=n, m=m, way=way, radius=label, max_dist2=r2,
                       exact_ms=round(float(np.median(t[0])), 4), exact_min_ms=round(min(t[0]), 4),
                       fast_ms=round(float(np.median(t[1])), 4), fast_min_ms=round(min(t[1]), 4),
                       exact_way=stats[0][0], stats=stats[1], records_per_query=round(stats[1][1] / m, 2),
                       median_count=float(np.median(c[0])), equal=bool((c[0] == c[1]).all()),
                       oracle_equal=bool((c[1][:QUANT].astype(np.int64) == want[i]).all()))
            print(json.dumps(row), flush=True)
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
    for case in a.cases:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", case, "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("case %s ended with status %d: stopping" % (case, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/count_within_timing.py: m = %d, uniform rows, one MI355X, one call at a time, ms per call (median / minimum of %d"
             " windows of %d calls, %d warm-ups), events around the window" % (M, a.reps, a.calls, a.warmup),
             "# exact = knn_index_count_within without a flag (way 1), fast = the same call with KNN_QUERY_COUNT_GRID / _CELLS on the same"
             " index, alternating; radius: 1nn = the median 1-NN distance, c10 / c100 = the median query counts about 10 / 100 rows",
             "# stats = knn_index_last_stats of the fast form ([2] != 0: gave up / fell back); rec/q = records re-ranked per query;"
             " equal = both forms' counts agree, and agree with the torch restatement of v0 on the first %d queries" % QUANT,
             "%-7s %2s %9s %6s %12s %7s %9s %9s %9s %9s %-22s %8s %5s" % (
                 "case", "k", "n", "radius", "max_dist2", "count", "exact ms", "exact min", "fast ms", "fast min", "stats", "rec/q",
                 "equal")]
    for r in rows:
        ok = r["equal"] and r["oracle_equal"]
        lines.append("%-7s %2d %9d %6s %12.6g %7.0f %9.4f %9.4f %9.4f %9.4f %-22s %8.2f %5s" % (
            r["case"], r["k"], r["n"], r["radius"], r["max_dist2"], r["median_count"], r["exact_ms"], r["exact_min_ms"], r["fast_ms"],
            r["fast_min_ms"], str(r["stats"]), r["records_per_query"], "yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if all(r["equal"] and r["oracle_equal"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
