#!/usr/bin/env python3
"""knn_index_list_within_masked and knn_index_query_topk_large_masked against the unmasked calls, ms per call, timed on one MI355X.

Shape: k 16, n 2^20, m 1024 (uniform rows, knn_synth_fill_device with seeds 1001 / 1000 as bench.py), option path 1.
Masks: admitted fractions 1, 1/2, 1/16, 1/256 of the rows, as random bits ("random") and as one contiguous range of that many
rows starting at an odd row ("range").
Steps, each in a child process of its own under a time limit, one after the other; the first that fails ends the run:
  list   (a) knn_index_list_within_masked against knn_index_list_within at one radius — chosen by bisection on the unmasked count
         so that it averages about 16 hits per query, printed — on segments made from the call's own (masked / unmasked) counts;
         equal: the masked call's fill is the masked count on every query
  large  (b) knn_index_query_topk_large_masked at K 256 against knn_index_query_topk_large at K 256 (another question: the K
         nearest of ALL rows) and against knn_index_query_topk_masked at K 64; equal: the first 64 keys of the masked large
         list are the masked top-K's keys on every query
The unmasked calls are the baseline: masked and unmasked windows alternate in one process.  ms per call: median, minimum and
maximum of `reps` windows of `calls` calls, events around the window.  cost = (masked ms / admitted rows) / (unmasked ms / rows):
what an admitted row costs against a row of the unmasked scan.
usage: masked_lists_timing.py [--reps R] [--calls C] [--warmup W] [--steps list large] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

K_DIM, LOG2N, M = 16, 20, 1024
FRACTIONS = (1, 2, 16, 256)   # 1 / f of the rows admitted
K_LARGE, K_SMALL = 256, 64
HITS = 16.0                   # unmasked hits per query the list radius aims at


def masks(n):
    import numpy as np

    rng = np.random.default_rng(20)
    for f in FRACTIONS:
        for shape in ("random", "range"):
            T = n // f
            bits = np.zeros(n, dtype=bool)
            if shape == "random":
                bits[rng.permutation(n)[:T]] = True
            else:
                start = (n - T) // 3 | 1 if T < n else 0
                bits[start:start + T] = True
            yield f, shape, T, np.packbits(bits, bitorder="little").view(np.int32).copy()


def step(which, reps, calls, warmup):
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
            for fn in forms:
                fn()
        torch.cuda.synchronize()
        t = [[] for _ in forms]
        for _ in range(reps):
            for g, fn in enumerate(forms):
                t[g].append(window(fn))
        return [(round(float(np.median(x)), 4), round(min(x), 4), round(max(x), 4)) for x in t]

    try:
        if which == "list":
            cnt_u = torch.empty(m, dtype=torch.int32, device=dev)
            cnt_m = torch.empty(m, dtype=torch.int32, device=dev)
            fill = torch.empty(m, dtype=torch.int32, device=dev)
            off_u = torch.empty(m + 1, dtype=torch.int64, device=dev)
            off_m = torch.empty(m + 1, dtype=torch.int64, device=dev)

            def mean_hits(r2):
                ix.count_within(m, Q.data_ptr(), r2, cnt_u.data_ptr(), stream=stream, init=True)
                torch.cuda.synchronize()
                return float(cnt_u.double().mean().item())

            lo, hi = 0.0, float(k)               # no row at 0, every row within k in the unit box
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                if mean_hits(mid) < HITS:
                    lo = mid
                else:
                    hi = mid
            r2 = float(np.float32(hi))
            hits = mean_hits(r2)
            pkg.counts_to_offsets(cnt_u.data_ptr(), m, off_u.data_ptr(), stream=stream)
            torch.cuda.synchronize()
            keys_u = torch.empty(max(int(off_u[m].item()), 1), dtype=torch.int64, device=dev)
            print(json.dumps(dict(step="list", radius2=r2, unmasked_hits_per_query=round(hits, 3))), flush=True)
            for f, shape, T, w in masks(n):
                words = torch.from_numpy(w).to(dev)
                ix.count_within_masked(m, Q.data_ptr(), r2, words.data_ptr(), cnt_m.data_ptr(), stream=stream, init=True)
                pkg.counts_to_offsets(cnt_m.data_ptr(), m, off_m.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                keys_m = torch.empty(max(int(off_m[m].item()), 1), dtype=torch.int64, device=dev)
                forms = [lambda: ix.list_within_masked(m, Q.data_ptr(), r2, words.data_ptr(), off_m.data_ptr(), fill.data_ptr(),
                                                       keys_m.data_ptr(), stream=stream, init=True),
                         lambda: ix.list_within(m, Q.data_ptr(), r2, off_u.data_ptr(), fill.data_ptr(), keys_u.data_ptr(),
                                                stream=stream, init=True)]
                tm, tu = timed(forms)
                forms[0]()
                torch.cuda.synchronize()
                print(json.dumps(dict(step="list", call="list", fraction="1/%d" % f, shape=shape, admitted=T, masked=tm, unmasked=tu,
                                      other=None, hits=round(float(cnt_m.double().mean().item()), 3),
                                      equal=bool((fill == cnt_m).all().item()))), flush=True)
        else:
            keys_m = torch.empty(m * K_LARGE, dtype=torch.int64, device=dev)
            keys_u = torch.empty(m * K_LARGE, dtype=torch.int64, device=dev)
            keys_s = torch.empty(m * K_SMALL, dtype=torch.int64, device=dev)
            for f, shape, T, w in masks(n):
                words = torch.from_numpy(w).to(dev)
                forms = [lambda: ix.query_topk_large_masked(m, K_LARGE, Q.data_ptr(), words.data_ptr(), keys_m.data_ptr(), stream=stream,
                                                            init_keys=True),
                         lambda: ix.query_topk_large(m, K_LARGE, Q.data_ptr(), keys_u.data_ptr(), stream=stream, init_keys=True),
                         lambda: ix.query_topk_masked(m, K_SMALL, Q.data_ptr(), words.data_ptr(), keys_s.data_ptr(), stream=stream,
                                                      init_keys=True)]
                tm, tu, tsm = timed(forms)
                forms[0]()
                forms[2]()
                torch.cuda.synchronize()
                same = (keys_m.view(m, K_LARGE)[:, :K_SMALL] == keys_s.view(m, K_SMALL)).all().item()
                print(json.dumps(dict(step="large", call="large", fraction="1/%d" % f, shape=shape, admitted=T, masked=tm, unmasked=tu,
                                      other=tsm, hits=None, equal=bool(same))), flush=True)
    finally:
        ix.close()
        pkg.set_option("path", 0)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="windows per form")
    ap.add_argument("--calls", type=int, default=10, help="calls per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", nargs="*", default=["list", "large"])
    ap.add_argument("--limit", type=int, default=240, help="seconds a step's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.calls, a.warmup)
    rows, head, rc = [], None, 0
    for which in a.steps:   # one child at a time, each under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", which, "--reps", str(a.reps), "--calls",
               str(a.calls), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                if "radius2" in r:
                    head = r
                else:
                    rows.append(r)
        if p.returncode != 0:
            print("step %s ended with status %d: stopping" % (which, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    n = 1 << LOG2N
    lines = ["# tools/masked_lists_timing.py: k = %d, n = 2^%d, m = %d, uniform rows, option path 1, one MI355X, one call at a time"
             % (K_DIM, LOG2N, M),
             "# ms per call: median / minimum / maximum of %d windows of %d calls, %d warm-ups, events around the window; the masked"
             " and the unmasked call alternate in one process" % (a.reps, a.calls, a.warmup),
             "# list  = knn_index_list_within_masked against knn_index_list_within, each on segments from its own counts"
             + ("; radius^2 = %.9g (bisection on the unmasked count: %.3f hits per query)" % (head["radius2"],
                                                                                            head["unmasked_hits_per_query"]) if head else ""),
             "# large = knn_index_query_topk_large_masked (K %d) against knn_index_query_topk_large (K %d, the K nearest of ALL rows);"
             " other = knn_index_query_topk_masked (K %d)" % (K_LARGE, K_LARGE, K_SMALL),
             "# cost  = (masked ms / admitted rows) / (unmasked ms / rows): an admitted row against a row of the unmasked scan",
             "# equal = list: the masked fill is the masked count; large: the first %d keys are the masked top-K's; on every query" % K_SMALL,
             "%-5s %8s %-6s %8s %9s %9s %9s %9s %9s %9s %9s %6s %8s %5s" % (
                 "call", "fraction", "mask", "admitted", "masked ms", "min", "max", "unmasked", "min", "max", "other ms", "cost",
                 "hits/q", "equal")]
    for r in rows:
        tm, tu = r["masked"], r["unmasked"]
        cost = (tm[0] / r["admitted"]) / (tu[0] / n)
        lines.append("%-5s %8s %-6s %8d %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f %9s %6.2f %8s %5s" % (
            r["call"], r["fraction"], r["shape"], r["admitted"], tm[0], tm[1], tm[2], tu[0], tu[1], tu[2],
            "%.4f" % r["other"][0] if r["other"] else "-", cost, "%.3f" % r["hits"] if r["hits"] is not None else "-",
            "yes" if r["equal"] else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if rows and all(r["equal"] for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
