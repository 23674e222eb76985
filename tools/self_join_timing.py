#!/usr/bin/env python3
"""knn_index_self_topk against what a caller had before it, ms per call, timed on one MI355X.

Shapes (uniform rows, knn_synth_fill_device with seed 1001 as bench.py; the call's rows are rows 300000 .. 301023 of the shard):
  k 16, n 2^20, rows 1024, K 8 and K 63
  k 3,  n 2^20, rows 1024, K 8 (the index has a grid index)
Sides, on the same device in the same process, their windows alternating (around, self, around', ...):
  self     knn_index_self_topk with K on the exact self-scan (option path 1; knn_index_last_stats [0] = 1)
  around   what a caller did without the call: knn_index_query_topk_within with K + 1 under option path 1 and the rows' device
           address as queries (its host-side removal of self is not timed).  It is timed in TWO interleaved series, one before
           and one after every self window: `spread` is the largest minus the smallest of all its windows — what repeated runs of
           one and the same thing differ by here
  route    knn_index_self_topk under the library's own route (option path 0): the way it took is printed (2: the MFMA filter, or
           4, through the plain call for K + 1 and the drop; 1: the self-scan again)
  grid     k 3 only: knn_index_self_topk with KNN_QUERY_TOPK_GRID (way 3), and the caller's K + 1 call with the same flag
ok: self <= around + spread (medians): the self-scan keeps K keys where the caller kept K + 1 and does the same row work.
equal: every side's keys equal `around`'s K + 1 keys with self removed (the last entry where self is not among them).
Every shape runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: self_join_timing.py [--reps R] [--calls C] [--warmup W] [--limit SECONDS] [--out FILE] [--title TEXT]
The library under test is the package's own, or the one KNN_MI355X_LIB names (another build of the same C-ABI)."""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

LOG2N, ROWS, FIRST = 20, 1024, 300000
SHAPES = ((16, 8), (16, 63), (3, 8))


def step(k, K, reps, calls, warmup):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    n, rows, first = 1 << LOG2N, ROWS, FIRST
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    torch.cuda.synchronize()
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    q_ptr = R.data_ptr() + first * k * 4
    inf = float("inf")

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        for _ in range(calls):
            fn()
        b.record(ts)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    keys = {name: torch.empty(rows * (K + 1 if name.startswith("around") else K), dtype=torch.int64, device=dev)
            for name in ("self", "around", "route", "grid", "around_grid")}

    def under(path, fn):
        def run():
            pkg.set_option("path", path)
            fn()
        return run

    sides = {
        "self": under(1, lambda: ix.self_topk(first, rows, K, keys["self"].data_ptr(), stream=stream, init_keys=True)),
        "around": under(1, lambda: ix.query_topk_within(rows, K + 1, q_ptr, inf, keys["around"].data_ptr(), stream=stream, init_keys=True)),
        "route": under(0, lambda: ix.self_topk(first, rows, K, keys["route"].data_ptr(), stream=stream, init_keys=True)),
    }
    if k <= 4:
        sides["grid"] = under(0, lambda: ix.self_topk(first, rows, K, keys["grid"].data_ptr(), stream=stream, init_keys=True, grid=True))
        sides["around_grid"] = under(0, lambda: ix.query_topk_within(rows, K + 1, q_ptr, inf, keys["around_grid"].data_ptr(), stream=stream,
                                                                     init_keys=True, grid=True))
    order = ["around", "self", "around"] + [s for s in sides if s not in ("around", "self")]
    try:
        ways = {}
        for _ in range(warmup):
            for name, fn in sides.items():
                fn()
                torch.cuda.synchronize()
                ways[name] = ix.last_stats()[0]
        t = {name: [] for name in sides}
        for _ in range(reps):
            for name in order:
                t[name].append(window(sides[name]))
        # every side against `around` with self removed
        kw = keys["around"].view(rows, K + 1)
        own = torch.arange(first, first + rows, device=dev).view(rows, 1)
        is_self = ((kw & 0xFFFFFFFF) == own) & ((kw >> 32) < 0x7F800000)
        pos = torch.where(is_self.any(dim=1), is_self.int().argmax(dim=1), torch.full((rows,), K, device=dev)).view(rows, 1)
        col = torch.arange(K, device=dev).view(1, K)
        want = torch.gather(kw, 1, col + (col >= pos).long())
        equal = all(bool((keys[name].view(rows, K) == want).all().item()) for name in sides if not name.startswith("around"))
        med = {name: float(np.median(v)) for name, v in t.items()}
        spread = max(t["around"]) - min(t["around"])
        row = dict(k=k, K=K, ways=ways, equal=equal, spread_ms=round(spread, 4), ok=bool(med["self"] <= med["around"] + spread))
        for name in sides:
            row[name + "_ms"] = round(med[name], 4)
            row[name + "_min_ms"] = round(min(t[name]), 4)
        print(json.dumps(row), flush=True)
    finally:
        ix.close()
        pkg.set_option("path", 0)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per side (`around` gets twice as many)")
    ap.add_argument("--calls", type=int, default=5, help="calls per window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds a shape's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--title", default="", help="a first comment line that names the build under test")
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step[0], a.step[1], a.reps, a.calls, a.warmup)
    rows, rc = [], 0
    for k, K in SHAPES:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", str(k), str(K), "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("k %d K %d ended with status %d: stopping" % (k, K, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = (["# " + a.title] if a.title else []) + ["# tools/self_join_timing.py: n = 2^%d uniform rows, the call's rows = rows %d .. %d, no radius, one MI355X, one call at a time"
             % (LOG2N, FIRST, FIRST + ROWS - 1),
             "# ms per call: median (minimum) of %d windows of %d calls, %d warm-ups, events around the window, the sides alternating"
             % (a.reps, a.calls, a.warmup),
             "# self = knn_index_self_topk with K on the exact self-scan (option path 1); around = knn_index_query_topk_within with K + 1"
             " under option path 1, the rows as queries (%d windows, before and after every self window); spread = the largest minus the"
             " smallest of around's windows; ok = self <= around + spread" % (2 * a.reps),
             "# route = knn_index_self_topk under option path 0 (way = knn_index_last_stats [0]); grid / around+grid (k 3): the two calls"
             " with KNN_QUERY_TOPK_GRID; equal = every side's keys are around's keys with self removed",
             "%2s %2s %18s %18s %9s %3s %18s %3s %18s %18s %5s" % ("k", "K", "self ms", "around ms", "spread ms", "ok", "route ms", "way",
                                                                   "grid ms", "around+grid ms", "equal")]

    def pair(r, name):
        return "%8.4f (%7.4f)" % (r[name + "_ms"], r[name + "_min_ms"]) if name + "_ms" in r else "-"

    for r in rows:
        lines.append("%2d %2d %18s %18s %9.4f %3s %18s %3d %18s %18s %5s" % (
            r["k"], r["K"], pair(r, "self"), pair(r, "around"), r["spread_ms"], "yes" if r["ok"] else "NO", pair(r, "route"),
            r["ways"]["route"], pair(r, "grid"), pair(r, "around_grid"), "yes" if r["equal"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if len(rows) == len(SHAPES) and all(r["equal"] and r["ok"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
