#!/usr/bin/env python3
"""Radius-bounded top-K (knn_index_query_topk_within) against the plain knn_index_query_topk of the SAME flags on the SAME index —
the parent's code path —, ms per call, timed with stream events around the call.

Shapes: "grid" = k 3, n 2^20, m 1024 on the grid index (both calls carry KNN_QUERY_TOPK_GRID); "cells" = the default C3-shape
index (k 16, n 2^24, m 1024: 8-bit rows in bin frames) under option topk_cells = 1.  K = 8 and 64.  Uniform rows
(knn_synth_fill_device, seeds 1001 / 1000 as bench.py).  Radii: the medians, over the first 32 queries, of the distance to the
1st, the (K/2)-th and the (4K)-th nearest row — the radii at which a query has about 1, K/2 and 4K rows inside — and +INF.  They
are taken from v0's arithmetic restated with torch's element-wise float32 kernels on the device (tests/test_cells_topk_gpu.py's
restatement: a 2^24-row oracle on the host takes minutes); on the grid shape the first 8 queries' lists are also compared with
tests/topk_oracle.py, clipped.
Per (shape, K, radius): 3 warm-ups of each call, then 20 timed windows of one call each, the two calls alternating; the table
gives each call's median and minimum, knn_index_last_stats of the radius call (and [1], [2] of the plain one), and the share of
the radius call's lists that are shorter than K.  With +INF the two calls' keys are compared.
Every shape runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: within_timing.py [--reps R] [--warmup W] [--shapes grid cells] [--ks K ...] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

M = 1024
KS = (8, 64)
SHAPES = {"grid": (3, 20), "cells": (16, 24)}
QUANT = 32   # queries the radii are taken from


def _torch_dist2_topk(torch, q, r, k, T, chunk=1 << 20):
    """The T smallest v0 distances of each query (float32 [m][T], ascending): one rounding per operation, never fused."""
    best = torch.full((q.shape[0], T), float("inf"), dtype=torch.float32, device=q.device)
    for r0 in range(0, r.shape[0], chunk):
        rc = r[r0:r0 + chunk]
        d = torch.zeros((q.shape[0], rc.shape[0]), dtype=torch.float32, device=q.device)
        for j in range(k):
            diff = q[:, j:j + 1] - rc[None, :, j]
            sq = diff * diff
            d = d + sq
        d[~(d < float("inf"))] = float("inf")
        part = torch.topk(d, min(T, rc.shape[0]), dim=1, largest=False).values
        best = torch.sort(torch.cat([best, part], dim=1), dim=1).values[:, :T]
        del d
    return best


def step(shape, ks, reps, warmup):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg
    from tests.topk_oracle import KEY_INIT, keys_dist2, topk_keys

    k, log2n = SHAPES[shape]
    n, m = 1 << log2n, M
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    Q = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(Q.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    flags = dict(grid=True) if shape == "grid" else {}
    if shape == "cells":
        pkg.set_option("topk_cells", 1)
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        fn()
        b.record(ts)
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    try:
        near = _torch_dist2_topk(torch, Q.view(m, k)[:QUANT], R.view(n, k), k, 4 * max(ks)).cpu().numpy()
        for K in ks:
            radii = [("1", float(np.median(near[:, 0]))), ("K/2", float(np.median(near[:, K // 2 - 1]))),
                     ("4K", float(np.median(near[:, 4 * K - 1]))), ("inf", float("inf"))]
            for label, r2 in radii:
                keys = [torch.empty(m * K, dtype=torch.int64, device=dev) for _ in range(2)]
                calls = [lambda: ix.query_topk(m, K, Q.data_ptr(), keys[0].data_ptr(), stream=stream, init_keys=True, **flags),
                         lambda: ix.query_topk_within(m, K, Q.data_ptr(), r2, keys[1].data_ptr(), stream=stream, init_keys=True,
                                                      **flags)]
                for _ in range(warmup):
                    for f in calls:
                        f()
                torch.cuda.synchronize()
                t = [[], []]
                stats = [None, None]
                for _ in range(reps):
                    for g in range(2):
                        t[g].append(timed(calls[g]))
                        stats[g] = ix.last_stats()
                got = keys[1].cpu().numpy().view(np.uint64).reshape(m, K)
                full = keys[0].cpu().numpy().view(np.uint64).reshape(m, K)
                clipped = full.copy()
                clipped[keys_dist2(full) > np.float32(r2)] = KEY_INIT
                row = dict(shape=shape, k=k, n=n, m=m, K=K, radius=label, max_dist2=r2,
                           plain_ms=round(float(np.median(t[0])), 4), plain_min_ms=round(min(t[0]), 4),
                           within_ms=round(float(np.median(t[1])), 4), within_min_ms=round(min(t[1]), 4),
                           stats=stats[1], plain_records=stats[0][1], plain_fallback=stats[0][2],
                           short_lists=round(float((got[:, K - 1] == KEY_INIT).mean()), 4),
                           equal=bool((got == clipped).all()))   # the radius call against the plain call's keys, clipped
                if shape == "grid" and label == "K/2":
                    want = topk_keys(Q.cpu().numpy()[:8 * k], R.cpu().numpy(), k, K, chunk=8)
                    want[keys_dist2(want) > np.float32(r2)] = KEY_INIT
                    row["oracle_equal"] = bool((got[:8] == want).all())
                print(json.dumps(row), flush=True)
    finally:
        ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, tuple(a.ks), a.reps, a.warmup)
    rows, rc = [], 0
    for shape in a.shapes:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", shape, "--reps", str(a.reps), "--warmup",
               str(a.warmup), "--ks"] + [str(K) for K in a.ks]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("shape %s ended with status %d: stopping" % (shape, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/within_timing.py: m = %d, uniform rows, one MI355X, one call at a time, ms per call (median / minimum of %d windows,"
             " %d warm-ups), events around the call" % (M, a.reps, a.warmup),
             "# plain = knn_index_query_topk, within = knn_index_query_topk_within, the same flags on the same index, alternating;"
             " radius = rows a query has inside, about",
             "# stats = knn_index_last_stats of the radius call; plain rec / fb = [1], [2] of the plain call; short = share of lists"
             " shorter than K; equal = the radius call's keys are the plain call's, clipped",
             "%-5s %2s %9s %3s %6s %12s %9s %9s %10s %10s %-22s %9s %3s %6s %5s" % (
                 "shape", "k", "n", "K", "radius", "max_dist2", "plain ms", "plain min", "within ms", "within min", "stats",
                 "plain rec", "fb", "short", "equal")]
    for r in rows:
        ok = r["equal"] and r.get("oracle_equal", True)
        lines.append("%-5s %2d %9d %3d %6s %12.6g %9.4f %9.4f %10.4f %10.4f %-22s %9d %3d %6.3f %5s" % (
            r["shape"], r["k"], r["n"], r["K"], r["radius"], r["max_dist2"], r["plain_ms"], r["plain_min_ms"], r["within_ms"],
            r["within_min_ms"], str(r["stats"]), r["plain_records"], r["plain_fallback"], r["short_lists"], "yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if all(r["equal"] and r.get("oracle_equal", True) for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
