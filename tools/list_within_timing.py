#!/usr/bin/env python3
"""knn_index_list_within: what the writes cost over the count, per way, and the whole count -> offsets -> list -> sort sequence, ms
per call, timed with stream events around windows of calls.

Cases (m = 1024, uniform rows, knn_synth_fill_device with seeds 1001 / 1000 as bench.py):
  k3     k 3,  n 2^20: the exact way and the grid way (KNN_QUERY_COUNT_GRID)
  k16    k 16, n 2^22 on the fp16 one-frame layout (cells 1, cells_rows 1, cells_centre 2): the exact way and the cell-pruned way
         (KNN_QUERY_COUNT_CELLS)
Radii: three, giving a mean of about 1, 16 and 256 hits per query ("h1", "h16", "h256"), taken on the CPU from a sample — every
(n / 2^18)-th row against the first 64 queries with v0's arithmetic in numpy: the radius is the (hits * 64 * sample / n)-th smallest
of the pooled distances.  The table gives the mean the product then counted over all m queries.
Per (case, radius, way) the forms alternate in one process: the count call, the list call on offsets made from that count, and the
sequence count -> offsets -> list -> sort on one stream into a key buffer of the known total (a caller reads the total between
offsets and list to size that buffer: the one synchronisation of the scheme is not in the figure).  --parent-lib FILE: a second
child process per case loads that build of the library (the parent commit's, through KNN_MI355X_LIB) and times its count call on
the same shape and radii: the list's cost over THAT count is the price of the writes.  Without it the column repeats this build's
count.  Checked per row: fill equals the counts, and the fast way's sorted keys equal the exact way's.
Every case runs in child processes of its own under a time limit, one after the other; the first that fails ends the run.
usage: list_within_timing.py [--reps R] [--calls C] [--warmup W] [--cases k3 k16] [--parent-lib FILE] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, ".")

M = 1024
QUANT = 64          # queries the radii are taken from
SAMPLE = 1 << 18    # rows of the CPU sample
HITS = (1, 16, 256)
CASES = {
    "k3": (3, 20, {}, "grid"),
    "k16": (16, 22, {"cells": 1, "cells_rows": 1, "cells_centre": 2}, "cells"),
}


def sample_radii(np, Q, Rs, k, n):
    """The radii at which the mean number of hits per query is about HITS, from the sampled rows Rs (numpy, v0's arithmetic)."""
    d = np.zeros((Q.shape[0], Rs.shape[0]), dtype=np.float32)
    for j in range(k):
        diff = Q[:, j:j + 1] - Rs[None, :, j]
        d = d + diff * diff
    pooled = np.sort(d.reshape(-1))
    out = []
    for h in HITS:
        rank = int(round(h * Q.shape[0] * Rs.shape[0] / n))
        out.append(("h%d" % h, float(pooled[max(rank, 1) - 1])))
    return out


def step(case, reps, calls, warmup, count_only):
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
        stride = max(1, n // SAMPLE)
        radii = sample_radii(np, Q.view(m, k)[:QUANT].cpu().numpy(), R.view(n, k)[::stride].cpu().numpy(), k, n)
        for label, r2 in radii:
            for name, fl in (("exact", {}), (way, flag)):
                counts = torch.empty(m, dtype=torch.int32, device=dev)
                fill = torch.empty(m, dtype=torch.int32, device=dev)
                offsets = torch.empty(m + 1, dtype=torch.int64, device=dev)

                def count():
                    ix.count_within(m, Q.data_ptr(), r2, counts.data_ptr(), stream=stream, init=True, **fl)

                count()
                torch.cuda.synchronize()
                count_way = ix.last_stats()
                c = counts.cpu().numpy().view(np.uint32)
                row = dict(case=case, k=k, n=n, m=m, way=name, radius=label, max_dist2=r2, mean_hits=round(float(c.mean()), 2),
                           max_hits=int(c.max()), count_stats=count_way)
                forms = {"count": count}
                if not count_only:
                    pkg.counts_to_offsets(counts.data_ptr(), m, offsets.data_ptr(), stream=stream)
                    torch.cuda.synchronize()
                    total = int(offsets[m].item())
                    keys = torch.empty(max(total, 1), dtype=torch.int64, device=dev)

                    def listed():
                        ix.list_within(m, Q.data_ptr(), r2, offsets.data_ptr(), fill.data_ptr(), keys.data_ptr(), stream=stream,
                                       init=True, **fl)

                    def sequence():
                        count()
                        pkg.counts_to_offsets(counts.data_ptr(), m, offsets.data_ptr(), stream=stream)
                        listed()
                        pkg.keys_sort_segments(m, offsets.data_ptr(), fill.data_ptr(), keys.data_ptr(), stream=stream)

                    forms.update(list=listed, sequence=sequence)
                for _ in range(warmup):
                    for f in forms.values():
                        f()
                torch.cuda.synchronize()
                t = {f: [] for f in forms}
                for _ in range(reps):
                    for f, fn in forms.items():
                        t[f].append(window(fn))
                        if f == "list":
                            row["list_stats"] = ix.last_stats()
                for f in forms:
                    row[f + "_ms"] = round(float(np.median(t[f])), 4)
                    row[f + "_min_ms"] = round(min(t[f]), 4)
                if not count_only:   # (the last window was a sequence: the keys are sorted)
                    row["fill_equal"] = bool((fill.cpu().numpy().view(np.uint32) == c).all())
                    row["keys"] = keys.cpu().numpy()[:total].tobytes().hex() if total <= 64 else None
                    row["keys_sum"] = [int(total), int(keys[:total].sum().item()) if total else 0,
                                       int((keys[:total] * torch.arange(1, total + 1, device=dev)).sum().item()) if total else 0]
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
    ap.add_argument("--parent-lib", default="", help="the parent commit's libknn_mi355x.so: its count call is timed in a process of its own")
    ap.add_argument("--limit", type=int, default=240, help="seconds a case's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    ap.add_argument("--count-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.calls, a.warmup, a.count_only)
    rows, parent, rc = [], {}, 0
    for case in a.cases:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", case, "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup)]
        runs = [(cmd, dict(os.environ), rows.append)]
        if a.parent_lib:
            env = dict(os.environ, KNN_MI355X_LIB=os.path.abspath(a.parent_lib))
            runs.append((cmd + ["--count-only"], env, lambda r: parent.__setitem__((r["case"], r["radius"], r["way"]), r)))
        for c, env, keep in runs:
            p = subprocess.run(c, stdout=subprocess.PIPE, text=True, env=env)
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    keep(json.loads(line))
            rc = p.returncode
            if rc != 0:
                print("case %s ended with status %d: stopping" % (case, rc), file=sys.stderr)
                break
        if rc != 0:
            break
    lines = ["# tools/list_within_timing.py: m = %d, uniform rows, one MI355X, one call at a time, ms per call (median / minimum of %d"
             " windows of %d calls, %d warm-ups), events around the window" % (M, a.reps, a.calls, a.warmup),
             "# radius h1 / h16 / h256: a mean of about 1 / 16 / 256 hits per query by a CPU sample of %d rows and %d queries; hits ="
             " the mean and the largest count over the m queries" % (SAMPLE, QUANT),
             "# parent count = knn_index_count_within of %s; count, list = this build's calls; list - parent = the price of the writes;"
             % ("the parent commit's library, a process of its own" if a.parent_lib else "THIS build (no --parent-lib given)"),
             "# seq = count -> offsets -> list -> sort on one stream into a buffer of the known total; stats = knn_index_last_stats of"
             " the list call ([2] != 0: gave up / fell back); ok = fill equals the counts and the way's sorted keys equal the exact way's",
             "%-4s %2s %8s %-6s %5s %11s %8s %6s %12s %9s %9s %9s %9s %9s %9s %-20s %3s" % (
                 "case", "k", "n", "way", "rad", "max_dist2", "hits", "max", "parent count", "count", "list", "list min", "list-par",
                 "seq", "seq min", "stats", "ok")]
    exact = {(r["case"], r["radius"]): r for r in rows if r["way"] == "exact"}
    bad = False
    for r in rows:
        par = parent.get((r["case"], r["radius"], r["way"]), r)["count_ms"]
        e = exact[(r["case"], r["radius"])]
        ok = r["fill_equal"] and r["keys_sum"] == e["keys_sum"] and r["keys"] == e["keys"]
        bad = bad or not ok
        lines.append("%-4s %2d %8d %-6s %5s %11.6g %8.2f %6d %12.4f %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f %-20s %3s" % (
            r["case"], r["k"], r["n"], r["way"], r["radius"], r["max_dist2"], r["mean_hits"], r["max_hits"], par, r["count_ms"],
            r["list_ms"], r["list_min_ms"], r["list_ms"] - par, r["sequence_ms"], r["sequence_min_ms"], str(r["list_stats"]),
            "yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (1 if bad else 0)


if __name__ == "__main__":
    sys.exit(main())
