#!/usr/bin/env python3
"""knn_index_query_topk_large against one exact knn_index_count_within call of the same shape and, at K = 64, against
knn_index_query_topk on the exact top-K scan (option path = 1): ms per call, timed with stream events around windows of calls.

Cases: k in {3, 16, 128}, n = 2^20, m = 1024, uniform rows (knn_synth_fill_device with seeds 1001 / 1000 as bench.py), K in
{64, 256, 4096}, max_dist2 = +INF, KNN_QUERY_INIT_KEYS.  What the code leads one to expect: a select pass and the fill are each one
scan of the shard with the count scan's arithmetic, so a call is about (passes + 1) count scans plus the sort — the table gives
that ratio, large ms / ((passes + 1) * count ms), with passes = 4, or 8 when knn_index_last_stats says the index word's passes ran.
Per (k, K): warm-ups of each form, then `reps` windows of `calls` calls each, the forms alternating in the same process; median and
minimum ms per call.  At K = 64 the large call's keys must equal the top-K call's.
Every k runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: topk_large_timing.py [--reps R] [--calls C] [--warmup W] [--ks 3 16 128] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

M, LOG2N = 1024, 20
KS = (3, 16, 128)
BIG_KS = (64, 256, 4096)


def step(k, reps, calls, warmup):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    n, m = 1 << LOG2N, M
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    Q = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(Q.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    pkg.set_option("path", 1)   # the exact ways alone: no grid index, no filter layouts
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    inf = float("inf")

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        for _ in range(calls):
            fn()
        b.record(ts)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    try:
        counts = torch.empty(m, dtype=torch.int32, device=dev)
        for K in BIG_KS:
            keys = torch.empty(m * K, dtype=torch.int64, device=dev)
            forms = [("large", lambda: ix.query_topk_large(m, K, Q.data_ptr(), keys.data_ptr(), stream=stream, init_keys=True)),
                     ("count", lambda: ix.count_within(m, Q.data_ptr(), inf, counts.data_ptr(), stream=stream, init=True))]
            keys64 = None
            if K <= 64:
                keys64 = torch.empty(m * K, dtype=torch.int64, device=dev)
                forms.append(("topk", lambda: ix.query_topk(m, K, Q.data_ptr(), keys64.data_ptr(), stream=stream, init_keys=True)))
            for _ in range(warmup):
                for _, f in forms:
                    f()
            torch.cuda.synchronize()
            t = {name: [] for name, _ in forms}
            stats = None
            for _ in range(reps):
                for name, f in forms:
                    t[name].append(window(f))
                    if name == "large":
                        stats = ix.last_stats()
                    elif name == "topk":
                        assert ix.last_stats()[0] == 1, ix.last_stats()
            passes = 8 if stats[2] else 4
            got = keys.cpu().numpy().view(np.uint64).reshape(m, K)
            ok = bool((got[:, 1:] > got[:, :-1]).all()) and bool((counts.cpu().numpy().view(np.uint32) == n).all())
            if keys64 is not None:
                ok = ok and bool((keys == keys64).all().item())
            med = {name: float(np.median(v)) for name, v in t.items()}
            row = dict(k=k, n=n, m=m, K=K, large_ms=round(med["large"], 4), large_min_ms=round(min(t["large"]), 4),
                       count_ms=round(med["count"], 4), count_min_ms=round(min(t["count"]), 4),
                       topk_ms=round(med["topk"], 4) if "topk" in med else None, passes=passes, stats=stats,
                       ratio=round(med["large"] / ((passes + 1) * med["count"]), 3), ok=ok)
            print(json.dumps(row), flush=True)
    finally:
        ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per form")
    ap.add_argument("--calls", type=int, default=5, help="calls per window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", nargs="*", type=int, default=list(KS))
    ap.add_argument("--limit", type=int, default=240, help="seconds a k's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.calls, a.warmup)
    rows, rc = [], 0
    for k in a.ks:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", str(k), "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("k %d ended with status %d: stopping" % (k, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/topk_large_timing.py: n = 2^%d, m = %d, uniform rows, max_dist2 = +INF, one MI355X, one call at a time, ms per call"
             " (median / minimum of %d windows of %d calls, %d warm-ups), events around the window" % (LOG2N, M, a.reps, a.calls, a.warmup),
             "# large = knn_index_query_topk_large, count = one exact knn_index_count_within call of the same shape, topk ="
             " knn_index_query_topk on the exact top-K scan (path 1; K = 64 only), alternating on one index",
             "# passes = select passes that ran (4, or 8 when stats[2] = 1); ratio = large ms / ((passes + 1) * count ms): 1 = a call costs"
             " its scans at the count scan's speed; equal = lists ascending, counts = n, and at K = 64 the keys of large and topk agree",
             "%3s %5s %10s %10s %10s %10s %10s %6s %6s %-14s %5s" % ("k", "K", "large ms", "large min", "count ms", "count min", "topk ms",
                                                                   "passes", "ratio", "stats", "equal")]
    for r in rows:
        lines.append("%3d %5d %10.4f %10.4f %10.4f %10.4f %10s %6d %6.3f %-14s %5s" % (
            r["k"], r["K"], r["large_ms"], r["large_min_ms"], r["count_ms"], r["count_min_ms"],
            "%.4f" % r["topk_ms"] if r["topk_ms"] is not None else "-", r["passes"], r["ratio"], str(r["stats"]),
            "yes" if r["ok"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if rows and all(r["ok"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
