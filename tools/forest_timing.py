#!/usr/bin/env python3
"""Minimum spanning forest of the radius graph (knn_index_self_forest_within) against what a caller does at the parent commit — the
CSR adjacency from knn_index_self_list_within_routed_host under the same flag, then Kruskal on the host —, ms per call and bytes.

Shapes (one MI355X, one call at a time; uniform rows: knn_synth_fill_device, seed 1001 as bench.py):
  grid3      k 3,  n 2^20, the grid way, at the radius of profiles/cluster_timing.txt
  exact16    k 16, n 2^16, the exact way, at that radius' rule
  exact16inf k 16, n 2^16, the exact way, max_dist2 = +INF: the spanning tree.  The parent commit has no route to it: a list call
             needs a radius, and the complete graph of 2^16 rows is 2^32 list entries.
The radius is made by the library itself, as tools/cluster_timing.py makes it: knn_index_self_topk (K = 10) of the first 1024 rows ->
the median 10-th neighbour distance.  Per shape, warm-ups, then `reps` single calls, each between two stream events; median /
minimum / spread ((largest - smallest) / median) of the whole call (every round queued).
  route    knn_index_self_list_within_routed_host under the same flag (list) + Kruskal over its CSR on the host, in this tool
           (kruskal: a numpy sort by the edge order and a union-find loop in Python), one run on a host clock; beside it, where
           scipy is installed, scipy's minimum_spanning_tree over the same CSR (scipy), for a caller who has it
  bytes    the CSR's size (8-byte offsets, 4-byte indices, 4-byte distances) beside the call's slot scratch (knn_debug_forest_plan)
           and its outputs (16 bytes per row)
`same` = the call's edge weights, sorted, equal the route's bit for bit (every minimum spanning forest of a graph has the same
multiset of weights; WHICH of several equal edges is taken the tests check against the edge order).  Clocks: the device's current
shader clock as its driver reports it before and after each shape, where readable.  Every shape runs in a child process of its own
under a time limit, one after the other; the first that fails ends the run.
usage: forest_timing.py [--reps R] [--warmup W] [--shapes grid3 ...] [--limit SECONDS] [--no-route] [--out FILE]"""
import argparse
import glob
import json
import subprocess
import sys
import time

sys.path.insert(0, ".")

K_RADIUS = 10
SHAPES = {   # k, log2 n, way, infinite radius
    "grid3": (3, 20, "grid", False),
    "exact16": (16, 16, "exact", False),
    "exact16inf": (16, 16, "exact", True),
}


def sclk():
    """The shader clock the driver reports as current ('*' line of pp_dpm_sclk), or 'not readable'."""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            with open(path) as f:
                cur = [line.split(":")[1].strip().rstrip("*").strip() for line in f if line.rstrip().endswith("*")]
            if cur:
                return cur[0]
        except OSError:
            pass
    return "not readable"


def host_forest(n, offsets, indices, dist2):
    """Kruskal over the CSR, in this tool: the edges i < j sorted by (distance bits, i, j) with numpy, then a union-find loop in
    Python.  (the forest's weights float32 sorted, seconds)."""
    import numpy as np
    t0 = time.perf_counter()
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    b = indices.astype(np.int64)
    keep = a < b
    a, b, w = a[keep], b[keep], dist2[keep]
    order = np.lexsort((b, a, w.view(np.uint32)))
    parent = list(range(n))
    kept = []
    for t, (i, j) in enumerate(zip(a[order].tolist(), b[order].tolist())):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        while parent[j] != j:
            parent[j] = parent[parent[j]]
            j = parent[j]
        if i != j:
            parent[max(i, j)] = min(i, j)
            kept.append(t)
    out = np.sort(w[order][np.asarray(kept, dtype=np.int64)])
    return out, time.perf_counter() - t0


def host_forest_scipy(n, offsets, indices, dist2):
    """The same forest's weights by scipy's minimum_spanning_tree, where scipy is installed: (weights or None, seconds)."""
    import numpy as np
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import minimum_spanning_tree
    except ImportError:
        return None, 0.0
    t0 = time.perf_counter()
    a = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    b = indices.astype(np.int64)
    keep = a < b
    # (a stored zero is no edge to scipy: the weights go in shifted by one, exactly in float64 at these magnitudes)
    t = minimum_spanning_tree(coo_matrix((dist2[keep].astype(np.float64) + 1.0, (a[keep], b[keep])), shape=(n, n))).tocoo()
    return np.sort((t.data - 1.0).astype(np.float32)), time.perf_counter() - t0


def step(shape, reps, warmup, route):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    k, log2n, way, infinite = SHAPES[shape]
    n = 1 << log2n
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    clock0 = sclk()
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    torch.cuda.synchronize()
    ix = pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    try:
        keys = torch.empty(1024 * K_RADIUS, dtype=torch.int64, device=dev)
        kth = torch.empty(1024, dtype=torch.float32, device=dev)
        ix.self_topk(0, 1024, K_RADIUS, keys.data_ptr(), stream=stream, init_keys=True)
        pkg.keys_column_dist2(keys.data_ptr(), 1024, K_RADIUS, K_RADIUS - 1, kth.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        r2 = float("inf") if infinite else float(kth.median().item())
        flag = dict(grid=True) if way == "grid" else dict()
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        ekeys = torch.empty(n, dtype=torch.int64, device=dev)
        ehis = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        call = lambda: ix.self_forest_within(r2, labels.data_ptr(), ekeys.data_ptr(), ehis.data_ptr(), count.data_ptr(), stream=stream, **flag)
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ts)
            call()
            b.record(ts)
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
        st = ix.last_stats()
        cnt = count.cpu().numpy().view(np.uint32).tolist()
        e = cnt[0]
        weights = np.sort((ekeys.cpu().numpy().view(np.uint64)[:e] >> np.uint64(32)).astype(np.uint32).view(np.float32))
        plan = pkg.debug_forest_plan(k=k, n=n, num_cu=256, grid=1 if st[0] == 3 else 0)
        row = dict(shape=shape, way=way, k=k, n=n, radius=r2, edges=e, components=n - e, rounds=cnt[1], of=plan["rounds"],
                   whole=(round(float(np.median(t)), 3), round(min(t), 3), round((max(t) - min(t)) / float(np.median(t)), 3)),
                   stats=st[:3], launches=plan["launches"], scratch_bytes=plan["scratch_bytes"], out_bytes=16 * n + 8)
        if route and not infinite:
            t0 = time.perf_counter()
            off, ind, d2 = ix.self_list_within_routed_host(r2, **flag)
            t_list = time.perf_counter() - t0
            want, t_mst = host_forest(n, off, ind, d2)
            sci, t_sci = host_forest_scipy(n, off, ind, d2)
            eq = lambda x: bool(x.size == weights.size and (x.view(np.uint32) == weights.view(np.uint32)).all())   # noqa: E731
            row.update(route_ms=round(1e3 * (t_list + t_mst), 1), route_list_ms=round(1e3 * t_list, 1), route_mst_ms=round(1e3 * t_mst, 1),
                       route_scipy_ms=round(1e3 * t_sci, 1) if sci is not None else None,
                       csr_bytes=8 * (n + 1) + 8 * int(off[n]), hits=round(float(off[n]) / n, 2),
                       same=eq(want) and (sci is None or eq(sci)))
        print(json.dumps(row), flush=True)
        print(json.dumps(dict(shape=shape, clock_before=clock0, clock_after=sclk())), flush=True)
    finally:
        ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls per shape")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's process may take")
    ap.add_argument("--no-route", action="store_true", help="skip the adjacency route")
    ap.add_argument("--out", default="", help="also write the table there")
    ap.add_argument("--step", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.warmup, not a.no_route)
    rows, clocks, rc = [], [], 0
    for shape in a.shapes:   # one child at a time, each under its own limit; a failure ends the run
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, sys.argv[0], "--step", shape, "--reps", str(a.reps), "--warmup",
               str(a.warmup)] + (["--no-route"] if a.no_route else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        got = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        rows += [g for g in got if "way" in g]
        clocks += [g for g in got if "clock_before" in g]
        if p.returncode != 0:
            print("shape %s ended with status %d: stopping" % (shape, p.returncode), file=sys.stderr)
            rc = p.returncode
            break
    lines = ["# tools/forest_timing.py: knn_index_self_forest_within, uniform rows, one MI355X, one call at a time, ms per call: median /"
             " minimum / spread ((largest - smallest) / median) of %d single calls between two stream events, %d warm-ups" % (a.reps, a.warmup),
             "# radius = the median %d-th neighbour distance of 1024 rows (knn_index_self_topk -> knn_keys_column_dist2), or inf; hits = the"
             " mean degree; rounds = the rounds that added an edge, of ROUNDS(n) queued; launches = kernel launches of the call" % K_RADIUS,
             "# route = what a caller does at the parent commit: knn_index_self_list_within_routed_host under the same flag (list) + Kruskal"
             " over its CSR in this tool (kruskal: numpy sort, Python union-find), one run, host clock, ms; scipy = scipy's"
             " minimum_spanning_tree over the same CSR in kruskal's place; csr: bytes of that CSR; scratch / out: bytes of the call's slot"
             " scratch and of its outputs",
             "# an infinite radius has no route at the parent commit (a list call needs a radius; the complete graph is n^2 entries)",
             "# stats = knn_index_last_stats [0..2] of the call; same = the call's sorted edge weights equal kruskal's (and scipy's) bit for bit",
             "%-10s %-5s %2s %8s %11s %6s | %-28s %8s %10s %6s %8s | %9s %9s %9s %9s | %11s %10s %10s | %-9s %4s" % (
                 "shape", "way", "k", "n", "radius", "hits", "whole", "edges", "components", "rounds", "launches", "route", "list", "kruskal",
                 "scipy", "csr", "scratch", "out", "stats", "same")]
    for r in rows:
        lines.append("%-10s %-5s %2d %8d %11.6g %6s | %-28s %8d %10d %6s %8d | %9s %9s %9s %9s | %11s %10d %10d | %-9s %4s" % (
            r["shape"], r["way"], r["k"], r["n"], r["radius"], r.get("hits", "-"), "%.3f / %.3f / %.3f" % tuple(r["whole"]), r["edges"],
            r["components"], "%d/%d" % (r["rounds"], r["of"]), r["launches"], r.get("route_ms", "none"), r.get("route_list_ms", "-"),
            r.get("route_mst_ms", "-"), r.get("route_scipy_ms") or "-", r.get("csr_bytes", "-"), r["scratch_bytes"], r["out_bytes"],
            str(r["stats"]), "-" if "same" not in r else "yes" if r["same"] else "NO"))
    for c in clocks:
        lines.append("# %s: shader clock before %s, after %s" % (c["shape"], c["clock_before"], c["clock_after"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if all(r.get("same", True) for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
