#!/usr/bin/env python3
"""Clusters on the cell-pruned way (knn_index_self_cluster_within_routed with KNN_QUERY_COUNT_CELLS) against the exact way of the
SAME index and the same build, ms per call.  tools/isa_same.py shows the exact way's kernels unchanged from the parent commit, so
the exact columns are the parent's figures.

Shapes (one MI355X, one call at a time; uniform rows, knn_synth_fill_device with seed 1001 as bench.py; options cells 1,
cells_rows 1, cells_centre 2: the fp16 one-frame layout):
  k16_n18   k 16, n 2^18
  k16_n20   k 16, n 2^20
  k8_n20    k 8,  n 2^20
The radius is made by the library itself: knn_index_self_topk (K = 10) of the first 1024 rows -> the median 10-th neighbour
distance.  min_pts = 5.  Per (shape, way), warm-ups, then `reps` single calls, each between two stream events; median / minimum /
spread ((largest - smallest) / median):
  whole    knn_index_self_cluster_within_routed (labels and core mask), with the cells flag (way 4) or without a flag (way 1)
  degree   knn_index_self_count_within_routed over the whole shard in one call under the same flag: the call's degree step
  link     whole - degree (medians): the link sweep, with the two n-sized passes around it (core, flatten)
`same` = the two ways' labels and core masks are equal; stats = knn_index_last_stats of the call on each way.
Every shape runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: cluster_cells_timing.py [--reps R] [--warmup W] [--shapes k16_n18 ...] [--limit SECONDS] [--out FILE]"""
import argparse
import json
import subprocess
import sys

sys.path.insert(0, ".")

MIN_PTS, K_RADIUS = 5, 10
OPTIONS = {"cells": 1, "cells_rows": 1, "cells_centre": 2}
SHAPES = {"k16_n18": (16, 18), "k16_n20": (16, 20), "k8_n20": (8, 20)}   # k, log2 n
WAYS = (("cells", dict(cells=True)), ("exact", dict()))


def step(shape, reps, warmup):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    k, log2n = SHAPES[shape]
    n = 1 << log2n
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    torch.cuda.synchronize()
    for o, v in OPTIONS.items():
        pkg.set_option(o, v)
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    keys = torch.empty(1024 * K_RADIUS, dtype=torch.int64, device=dev)
    kth = torch.empty(1024, dtype=torch.float32, device=dev)
    ix.self_topk(0, 1024, K_RADIUS, keys.data_ptr(), stream=stream, init_keys=True)
    pkg.keys_column_dist2(keys.data_ptr(), 1024, K_RADIUS, K_RADIUS - 1, kth.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    r2 = float(kth.median().item())

    def one(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        fn()
        b.record(ts)
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def timed(forms):
        for _ in range(warmup):
            for f in forms:
                f()
        torch.cuda.synchronize()
        t = [[] for _ in forms]
        for _ in range(reps):
            for g_, f in enumerate(forms):
                t[g_].append(one(f))
        return [(round(float(np.median(x)), 3), round(min(x), 3), round((max(x) - min(x)) / float(np.median(x)), 3)) for x in t]

    try:
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        core = torch.empty((n + 31) // 32, dtype=torch.int32, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        answers = []
        for way, flag in WAYS:
            (whole, degree) = timed([
                lambda: ix.self_cluster_within_routed(r2, MIN_PTS, labels.data_ptr(), core_dev=core.data_ptr(), stream=stream, **flag),
                lambda: ix.self_count_within_routed(0, n, counts.data_ptr(), cap=r2, stream=stream, init=True, **flag)])
            labels.fill_(-7)
            core.fill_(-1)
            torch.cuda.synchronize()
            ix.self_cluster_within_routed(r2, MIN_PTS, labels.data_ptr(), core_dev=core.data_ptr(), stream=stream, **flag)
            torch.cuda.synchronize()
            st = ix.last_stats()
            lab = labels.cpu().numpy()
            deg = counts.cpu().numpy().view(np.uint32)
            answers.append((lab, core.cpu().numpy()))
            print(json.dumps(dict(shape=shape, way=way, k=k, n=n, radius=r2, hits=round(float(deg.mean()), 2), whole=whole, degree=degree,
                                  link=round(whole[0] - degree[0], 3), stats=st, clusters=int(np.unique(lab[lab >= 0]).size),
                                  core=round(float((deg.astype(np.int64) + 1 >= MIN_PTS).mean()), 3),
                                  noise=round(float((lab < 0).mean()), 3))), flush=True)
        same = bool(np.array_equal(answers[0][0], answers[1][0]) and np.array_equal(answers[0][1], answers[1][1]))
        print(json.dumps(dict(shape=shape, same=same)), flush=True)
    finally:
        ix.close()
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls per form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--limit", type=int, default=300, help="seconds a shape's process may take")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.warmup)
    rows, same, rc = [], {}, 0
    for shape in a.shapes:   # one child at a time, each under its own limit; a failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", shape, "--reps", str(a.reps), "--warmup",
               str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        got = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        rows += [g for g in got if "way" in g]
        same.update({g["shape"]: g["same"] for g in got if "same" in g})
        if p.returncode != 0:
            print("shape %s ended with status %d: stopping" % (shape, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/cluster_cells_timing.py: knn_index_self_cluster_within_routed, min_pts %d, one MI355X, one call at a time, ms per"
             " call: median / minimum / spread ((largest - smallest) / median) of %d single calls between two stream events, %d warm-ups"
             % (MIN_PTS, a.reps, a.warmup),
             "# uniform rows, the fp16 one-frame cell-sorted layout; radius = the median %d-th neighbour distance of the first 1024 rows"
             " (knn_index_self_topk -> knn_keys_column_dist2); hits = the mean degree" % K_RADIUS,
             "# way cells = KNN_QUERY_COUNT_CELLS (way 4), way exact = no flag (way 1: the exact self-scan, the parent commit's kernels)",
             "# whole = the call; degree = knn_index_self_count_within_routed over the whole shard under the same flag (the call's degree"
             " step); link = whole - degree: the link sweep and the two n-sized passes (core, flatten)",
             "# stats = knn_index_last_stats of the call; same = labels and core mask of the two ways are equal",
             "%-8s %-5s %2s %8s %11s %7s | %-28s %-28s %10s | %6s %5s %8s %-22s %4s" % (
                 "shape", "way", "k", "n", "radius", "hits", "whole", "degree", "link", "core", "noise", "clusters", "stats", "same")]
    fmt = lambda t: "%.3f / %.3f / %.3f" % tuple(t)   # noqa: E731
    for r in rows:
        s = same.get(r["shape"])
        lines.append("%-8s %-5s %2d %8d %11.6g %7.2f | %-28s %-28s %10.3f | %6.3f %5.3f %8d %-22s %4s" % (
            r["shape"], r["way"], r["k"], r["n"], r["radius"], r["hits"], fmt(r["whole"]), fmt(r["degree"]), r["link"], r["core"],
            r["noise"], r["clusters"], str(r["stats"]), "-" if s is None else "yes" if s else "NO"))
    by = {(r["shape"], r["way"]): r for r in rows}
    for shape in a.shapes:
        c, e = by.get((shape, "cells")), by.get((shape, "exact"))
        if c and e:
            lines.append("# %s: whole exact / cells = %.2f, degree exact / cells = %.2f, link exact / cells = %.2f%s" % (
                shape, e["whole"][0] / c["whole"][0], e["degree"][0] / c["degree"][0], e["link"] / c["link"] if c["link"] > 0 else float("nan"),
                "" if c["whole"][0] < e["whole"][0] else " — the cell-pruned way is NOT faster here"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if all(same.values()) else 1)


if __name__ == "__main__":
    sys.exit(main())
