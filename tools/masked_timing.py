#!/usr/bin/env python3
"""knn_index_query_topk_masked against what a caller had before it, ms per call, timed on one MI355X.

Shape: k 16, n 2^20, m 1024 (uniform rows, knn_synth_fill_device with seeds 1001 / 1000 as bench.py), K 8 and 64, no radius.
Masks: admitted fractions 1, 1/2, 1/16, 1/256 of the rows, as random bits ("random") and as one contiguous range of that many
rows starting at an odd row ("range").
Forms, on the same device in the same process:
  masked    knn_index_query_topk_masked on the index of the whole shard (events around windows of `calls` calls)
  unmasked  (a) knn_index_query_topk of the whole shard on the exact scan (option path 1): what over-fetching starts from — it
            answers another question (the K nearest of ALL rows), its time does not depend on the mask; masked and unmasked
            windows alternate
  subset    (b) gather the admitted rows, build an index over them (library defaults), query it, map the numbers back: a host
            clock around the whole sequence ending in a device synchronise (the build synchronises anyway), `builds` times after
            one warm-up; "query" is that index's query alone, events around windows, before it is closed
equal: the masked keys equal (b)'s keys with the numbers mapped back (both are exact) on every query.
Every K runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: masked_timing.py [--reps R] [--calls C] [--warmup W] [--builds B] [--ks 8 64] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys
import time

sys.path.insert(0, ".")

K_DIM, LOG2N, M = 16, 20, 1024
FRACTIONS = (1, 2, 16, 256)   # 1 / f of the rows admitted


def step(K, reps, calls, warmup, builds):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    k, n, m = K_DIM, 1 << LOG2N, M
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    Q = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(Q.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    pkg.set_option("path", 1)
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    rng = np.random.default_rng(20)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        for _ in range(calls):
            fn()
        b.record(ts)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    def subset(rows_d, keys_out):
        """(b): gather, build, query, map back; returns (the index, its keys) — the caller closes."""
        sub = R.view(n, k).index_select(0, rows_d).contiguous()
        sx = pkg.KnnIndex(k, sub.data_ptr(), n_local=sub.shape[0], refs_on_device=True, owners=sub)
        sx.query_topk(m, K, Q.data_ptr(), keys_out.data_ptr(), stream=stream, init_keys=True)
        real = (keys_out >> 32) < 0x7F800000
        mapped = (keys_out & ~0xFFFFFFFF) | rows_d[(keys_out & 0xFFFFFFFF).clamp(max=rows_d.numel() - 1)]
        return sx, torch.where(real, mapped, keys_out)

    try:
        keys_m = torch.empty(m * K, dtype=torch.int64, device=dev)
        keys_u = torch.empty(m * K, dtype=torch.int64, device=dev)
        keys_s = torch.empty(m * K, dtype=torch.int64, device=dev)
        for f in FRACTIONS:
            for shape in ("random", "range"):
                T = n // f
                bits = np.zeros(n, dtype=bool)
                if shape == "random":
                    bits[rng.permutation(n)[:T]] = True
                else:
                    start = (n - T) // 3 | 1 if T < n else 0
                    bits[start:start + T] = True
                words = torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy()).to(dev)
                rows_d = torch.from_numpy(np.flatnonzero(bits)).to(dev)
                forms = [lambda: ix.query_topk_masked(m, K, Q.data_ptr(), words.data_ptr(), keys_m.data_ptr(), stream=stream, init_keys=True),
                         lambda: ix.query_topk(m, K, Q.data_ptr(), keys_u.data_ptr(), stream=stream, init_keys=True)]
                for _ in range(warmup):
                    for fn in forms:
                        fn()
                torch.cuda.synchronize()
                t = [[], []]
                for _ in range(reps):
                    for g in range(2):
                        t[g].append(window(forms[g]))
                way_u = ix.last_stats()[0]
                # (b) under the library's defaults
                pkg.set_option("path", 0)
                total, query, got = [], [], None
                for i in range(builds + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sx, got = subset(rows_d, keys_s)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if i > 0:
                        total.append((t1 - t0) * 1e3)
                    if i == builds:
                        way_s = sx.last_stats()[0]
                        query = [window(lambda: sx.query_topk(m, K, Q.data_ptr(), keys_s.data_ptr(), stream=stream, init_keys=True))
                                 for _ in range(reps)]
                    sx.close()
                pkg.set_option("path", 1)
                forms[0]()
                torch.cuda.synchronize()
                row = dict(K=K, fraction="1/%d" % f, shape=shape, admitted=T,
                           masked_ms=round(float(np.median(t[0])), 4), masked_min_ms=round(min(t[0]), 4),
                           unmasked_ms=round(float(np.median(t[1])), 4), unmasked_min_ms=round(min(t[1]), 4), unmasked_way=way_u,
                           subset_ms=round(float(np.median(total)), 3), subset_min_ms=round(min(total), 3),
                           subset_query_ms=round(float(np.median(query)), 4), subset_way=way_s,
                           equal=bool((keys_m == got).all().item()))
                print(json.dumps(row), flush=True)
    finally:
        ix.close()
        pkg.set_option("path", 0)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per form")
    ap.add_argument("--calls", type=int, default=10, help="calls per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--builds", type=int, default=3, help="timed gather-build-query sequences per mask")
    ap.add_argument("--ks", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--limit", type=int, default=240, help="seconds a K's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.calls, a.warmup, a.builds)
    rows, rc = [], 0
    for K in a.ks:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", str(K), "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup), "--builds", str(a.builds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        if p.returncode != 0:
            print("K %d ended with status %d: stopping" % (K, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/masked_timing.py: k = %d, n = 2^%d, m = %d, uniform rows, no radius, one MI355X, one call at a time" % (K_DIM, LOG2N, M),
             "# masked = knn_index_query_topk_masked, unmasked = knn_index_query_topk of the whole shard on the exact scan (option path 1;"
             " another question: the K nearest of ALL rows): ms per call, median / minimum of %d windows of %d calls, %d warm-ups, events"
             " around the window, the two alternating" % (a.reps, a.calls, a.warmup),
             "# subset = gather the admitted rows + build an index over them (library defaults) + query + map the numbers back: ms per"
             " sequence on a host clock ending in a device synchronise, median / minimum of %d after one warm-up; query = that index's"
             " query alone (way = its knn_index_last_stats [0])" % a.builds,
             "# equal = the masked keys are the subset index's keys with the numbers mapped back, on every query",
             "%2s %8s %-6s %8s %10s %10s %11s %11s %10s %10s %9s %3s %5s" % (
                 "K", "fraction", "mask", "admitted", "masked ms", "masked min", "unmasked ms", "unmasked min", "subset ms", "subset min",
                 "query ms", "way", "equal")]
    for r in rows:
        lines.append("%2d %8s %-6s %8d %10.4f %10.4f %11.4f %11.4f %10.3f %10.3f %9.4f %3d %5s" % (
            r["K"], r["fraction"], r["shape"], r["admitted"], r["masked_ms"], r["masked_min_ms"], r["unmasked_ms"], r["unmasked_min_ms"],
            r["subset_ms"], r["subset_min_ms"], r["subset_query_ms"], r["subset_way"], "yes" if r["equal"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if rows and all(r["equal"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
