#!/usr/bin/env python3
"""Top-K on the grid index (KNN_QUERY_TOPK_GRID) against the path the same call takes without the flag (the exact top-K scan),
ms per batch, timed with stream events around the call.

One process, one index per shape: k = 2, 3, 4; n = 2^16, 2^20, 2^24 (k = 3 only at 2^24); K = 1, 8, 64; m = 1024; uniform rows
(knn_synth_fill_device, seeds 1001 / 1000 as bench.py).  Per (shape, K): 3 warm-ups of each form, then 20 timed pairs, the two
forms alternating; the table gives each form's median and minimum.  Once per shape the first 64 queries' keys (K = 64, flag on)
are compared with tests/topk_oracle.py, and for every K the two forms' keys of all m queries with each other.
"path" / "gave up" are knn_index_last_stats()[0] / [2] of the call with the flag.
usage: grid_topk_timing.py [--reps R] [--warmup W] [--shapes k:log2n ...] [--ks K ...] [--out FILE]"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import multicore_hw2_amd as pkg  # noqa: E402
from tests.topk_oracle import topk_keys  # noqa: E402

SHAPES = [(2, 16), (3, 16), (4, 16), (2, 20), (3, 20), (4, 20), (3, 24)]
KS = (1, 8, 64)
M = 1024


def _timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def run(k, log2n, ks, reps, warmup):
    n, m = 1 << log2n, M
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    Q = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(Q.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    rows = []
    try:
        for K in ks:
            keys = [torch.empty(m * K, dtype=torch.int64, device=dev) for _ in range(2)]
            forms = [lambda g=g: ix.query_topk(m, K, Q.data_ptr(), keys[g].data_ptr(), stream=stream, init_keys=True, grid=bool(g))
                     for g in range(2)]
            for _ in range(warmup):
                for f in forms:
                    f()
            torch.cuda.synchronize()
            t = [[], []]
            for _ in range(reps):
                for g in range(2):
                    t[g].append(_timed(forms[g], ts))
            st = ix.last_stats()   # (the last call carried the flag)
            same = bool((keys[0] == keys[1]).all().item())
            row = dict(k=k, n=n, m=m, K=K, exact_ms=round(float(np.median(t[0])), 4), exact_min_ms=round(min(t[0]), 4),
                       grid_ms=round(float(np.median(t[1])), 4), grid_min_ms=round(min(t[1]), 4), path=st[0], gave_up=st[2],
                       keys_equal=same)
            row["speedup"] = round(row["exact_ms"] / row["grid_ms"], 2)
            if K == max(ks):   # the spot check against the oracle: the first 64 queries, chunks that fit the host at n = 2^24
                qh, rh = Q.cpu().numpy()[:64 * k], R.cpu().numpy()
                want = topk_keys(qh, rh, k, K, chunk=max(1, min(64, (1 << 26) // n)))
                got = keys[1].cpu().numpy().view(np.uint64).reshape(m, K)[:64]
                row["oracle_equal"] = bool((got == want).all())
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        ix.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", nargs="*", default=None, metavar="k:log2n")
    ap.add_argument("--ks", type=int, nargs="*", default=None)
    ap.add_argument("--out", default="", help="also write the table there")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes] if a.shapes else SHAPES
    out = []
    for k, log2n in shapes:
        out += run(k, log2n, tuple(a.ks) if a.ks else KS, a.reps, a.warmup)
    lines = ["# tools/grid_topk_timing.py: m = %d, uniform rows, ms per batch (median / minimum of %d, %d warm-ups), events around the call"
             % (M, a.reps, a.warmup),
             "# exact = the call without KNN_QUERY_TOPK_GRID (the exact top-K scan), grid = the same call with it",
             "%2s %9s %3s %10s %10s %10s %10s %8s %5s %8s %6s" % ("k", "n", "K", "exact ms", "exact min", "grid ms", "grid min",
                                                                  "exact/grid", "path", "gave up", "equal")]
    for r in out:
        ok = r["keys_equal"] and r.get("oracle_equal", True)
        lines.append("%2d %9d %3d %10.4f %10.4f %10.4f %10.4f %8.2f %5d %8d %6s" % (
            r["k"], r["n"], r["K"], r["exact_ms"], r["exact_min_ms"], r["grid_ms"], r["grid_min_ms"], r["speedup"], r["path"],
            r["gave_up"], "yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if all(r["keys_equal"] and r.get("oracle_equal", True) for r in out) else 1


if __name__ == "__main__":
    sys.exit(main())
