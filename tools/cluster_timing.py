#!/usr/bin/env python3
"""Clusters of the radius graph (knn_index_self_cluster_within) against the parent commit's route to the same labels — the CSR
adjacency from knn_index_self_list_within_routed_host under the same flag, then a union-find on the host —, ms per call.

Shapes (one MI355X, one call at a time):
  uniform3   k 3, n 2^20, uniform rows (knn_synth_fill_device, seed 1001 as bench.py), on the grid way and on the exact way
  blobs3     k 3, n 2^20, 64 gaussian blobs (sigma 0.04, centres uniform in the unit cube, rows in shuffled order), both ways: dense
             clusters, the heavy union traffic
  uniform16  k 16, n 2^18, uniform rows, the exact way
The radius is made by the library itself: knn_index_self_topk (K = 10) of the first 1024 rows -> the median 10-th neighbour
distance — about 10 rows within the radius of a uniform row; the blobs take uniform3's radius.  min_pts = 5.
Per (shape, way), warm-ups, then `reps` single calls, each between two stream events; median / minimum / spread ((largest -
smallest) / median):
  whole    knn_index_self_cluster_within (labels and core mask)
  degree   knn_index_self_count_within_routed over the whole shard in one call under the same flag: the call's degree step
  link     whole - degree (medians): the link sweep, with the two n-sized passes around it (core, flatten)
  adjacency route   knn_index_self_list_within_routed_host under the same flag + the host union-find over the CSR it returns (core
           rows by their degrees, components of the core-core edges; scipy's connected_components where scipy is installed, else
           numpy label propagation), one run on a host clock: count, offsets, list, sort, the copy to the host, the union-find
  bytes    the CSR's size (8-byte offsets, 4-byte indices, 4-byte distances) beside the call's slot scratch (knn_debug_cluster_plan)
`same` = the call's labels on core rows, renumbered, equal the adjacency route's components (border rows need the distances: the
tests check them).  Clocks: the device's current shader clock as its driver reports it before and after each shape, where readable.
Every shape runs in a child process of its own under a time limit, one after the other; the first that fails ends the run.
usage: cluster_timing.py [--reps R] [--warmup W] [--shapes uniform3 ...] [--limit SECONDS] [--no-route] [--out FILE]"""
import argparse
import glob
import json
import subprocess
import sys
import time

sys.path.insert(0, ".")

MIN_PTS, K_RADIUS = 5, 10
SHAPES = {   # k, log2 n, rows, ways
    "uniform3": (3, 20, "uniform", ("grid", "exact")),
    "blobs3": (3, 20, "blobs", ("grid", "exact")),
    "uniform16": (16, 18, "uniform", ("exact",)),
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


def host_components(n, offsets, indices, min_pts):
    """(labels of core rows numbered by first appearance else -1, seconds, which)."""
    import numpy as np
    t0 = time.perf_counter()
    deg = np.diff(offsets)
    core = deg + 1 >= min_pts
    a = np.repeat(np.arange(n, dtype=np.int64), deg)
    b = indices.astype(np.int64)
    keep = core[a] & core[b] & (b < a)
    a, b = a[keep], b[keep]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _, lab = connected_components(coo_matrix((np.ones(a.size, dtype=np.int8), (a, b)), shape=(n, n)), directed=False)
        which = "scipy"
    except ImportError:
        lab = np.arange(n, dtype=np.int64)
        while True:
            m = np.minimum(lab[a], lab[b])
            new = lab.copy()
            np.minimum.at(new, a, m)
            np.minimum.at(new, b, m)
            while True:
                j = new[new]
                if (j == new).all():
                    break
                new = j
            if (new == lab).all():
                break
            lab = new
        which = "numpy"
    # number the components of core rows by their smallest row
    first = np.full(lab.max() + 1, n, dtype=np.int64)
    rows = np.flatnonzero(core)
    np.minimum.at(first, lab[rows], rows)
    reps = np.sort(first[first < n])
    out = np.full(n, -1, dtype=np.int64)
    out[rows] = np.searchsorted(reps, first[lab[rows]])
    return out, core, time.perf_counter() - t0, which


def step(shape, reps, warmup, route):
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    k, log2n, kind, ways = SHAPES[shape]
    n = 1 << log2n
    dev = torch.device("cuda:0")
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    clock0 = sclk()
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    torch.cuda.synchronize()
    radius_of = R
    if kind == "blobs":
        g = torch.Generator(device="cpu").manual_seed(1002)
        centres = torch.rand((64, k), generator=g)
        which = torch.randint(0, 64, (n,), generator=g)
        B = (centres[which] + 0.04 * torch.randn((n, k), generator=g)).to(torch.float32).contiguous()
        radius_of, R = R, B.reshape(-1).to(dev)
    # the radius: the median K_RADIUS-th neighbour distance of 1024 uniform rows
    ixu = pkg.KnnIndex(k, radius_of.data_ptr(), n_local=n, refs_on_device=True, owners=radius_of)
    keys = torch.empty(1024 * K_RADIUS, dtype=torch.int64, device=dev)
    kth = torch.empty(1024, dtype=torch.float32, device=dev)
    ixu.self_topk(0, 1024, K_RADIUS, keys.data_ptr(), stream=stream, init_keys=True)
    pkg.keys_column_dist2(keys.data_ptr(), 1024, K_RADIUS, K_RADIUS - 1, kth.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    r2 = float(kth.median().item())
    ix = ixu if kind == "uniform" else pkg.KnnIndex(k, R.data_ptr(), n_local=n, refs_on_device=True, owners=R)
    if ix is not ixu:
        ixu.close()

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
        for way in ways:
            flag = dict(grid=True) if way == "grid" else dict()
            (whole, degree) = timed([
                lambda: ix.self_cluster_within(r2, MIN_PTS, labels.data_ptr(), core_dev=core.data_ptr(), stream=stream, **flag),
                lambda: ix.self_count_within_routed(0, n, counts.data_ptr(), cap=r2, stream=stream, init=True, **flag)])
            ix.self_cluster_within(r2, MIN_PTS, labels.data_ptr(), core_dev=core.data_ptr(), stream=stream, **flag)
            torch.cuda.synchronize()
            st = ix.last_stats()
            lab = labels.cpu().numpy()
            deg = counts.cpu().numpy().view(np.uint32)
            is_core = deg.astype(np.int64) + 1 >= MIN_PTS
            plan = pkg.debug_cluster_plan(k=k, n=n, num_cu=256, core_given=1, grid=1 if st[0] == 3 else 0)
            row = dict(shape=shape, way=way, k=k, n=n, radius=r2, hits=round(float(deg.mean()), 2), whole=whole, degree=degree,
                       link=round(whole[0] - degree[0], 3), stats=st[:3], clusters=int(np.unique(lab[lab >= 0]).size),
                       core=round(float(is_core.mean()), 3), noise=round(float((lab < 0).mean()), 3),
                       scratch_bytes=plan["scratch_bytes"] + plan["count_bytes"], csr_bytes=8 * (n + 1) + 8 * int(deg.sum()))
            if route:
                t0 = time.perf_counter()
                off, ind, _ = ix.self_list_within_routed_host(r2, **flag)
                t_list = time.perf_counter() - t0
                comp, hcore, t_uf, which_uf = host_components(n, off, ind, MIN_PTS)
                reps_ = np.unique(lab[hcore])
                mine = np.searchsorted(reps_, lab[hcore])
                row.update(route_ms=round(1e3 * (t_list + t_uf), 1), route_list_ms=round(1e3 * t_list, 1), route_uf_ms=round(1e3 * t_uf, 1),
                           route_uf=which_uf, same=bool((hcore == is_core).all() and (mine == comp[hcore]).all()))
            print(json.dumps(row), flush=True)
        print(json.dumps(dict(shape=shape, clock_before=clock0, clock_after=sclk())), flush=True)
    finally:
        ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls per form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--limit", type=int, default=420, help="seconds a shape's process may take")
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
    lines = ["# tools/cluster_timing.py: knn_index_self_cluster_within, min_pts %d, one MI355X, one call at a time, ms per call: median /"
             " minimum / spread ((largest - smallest) / median) of %d single calls between two stream events, %d warm-ups"
             % (MIN_PTS, a.reps, a.warmup),
             "# radius = the median %d-th neighbour distance of 1024 uniform rows (knn_index_self_topk -> knn_keys_column_dist2); hits = the"
             " mean degree; blobs3: 64 gaussian blobs, sigma 0.04, at uniform3's radius" % K_RADIUS,
             "# whole = the call; degree = knn_index_self_count_within_routed over the whole shard under the same flag (the call's degree"
             " step); link = whole - degree: the link sweep and the two n-sized passes (core, flatten)",
             "# route = the parent commit's way to the labels: knn_index_self_list_within_routed_host under the same flag (list) + a host"
             " union-find over its CSR (uf), one run, host clock, ms; csr / scratch: bytes of that CSR and of the call's slot scratch",
             "# stats = knn_index_last_stats [0..2] of the call; same = the call's core rows and their clusters equal the route's",
             "%-9s %-5s %2s %8s %11s %7s | %-26s %-26s %9s | %10s %10s %9s %-5s | %12s %10s | %6s %5s %8s %-9s %4s" % (
                 "shape", "way", "k", "n", "radius", "hits", "whole", "degree", "link", "route", "list", "uf", "with", "csr", "scratch",
                 "core", "noise", "clusters", "stats", "same")]
    fmt = lambda t: "%.3f / %.3f / %.3f" % tuple(t)   # noqa: E731
    for r in rows:
        lines.append("%-9s %-5s %2d %8d %11.6g %7.2f | %-26s %-26s %9.3f | %10s %10s %9s %-5s | %12d %10d | %6.3f %5.3f %8d %-9s %4s" % (
            r["shape"], r["way"], r["k"], r["n"], r["radius"], r["hits"], fmt(r["whole"]), fmt(r["degree"]), r["link"],
            r.get("route_ms", "-"), r.get("route_list_ms", "-"), r.get("route_uf_ms", "-"), r.get("route_uf", "-"), r["csr_bytes"],
            r["scratch_bytes"], r["core"], r["noise"], r["clusters"], str(r["stats"]), "-" if "same" not in r else "yes" if r["same"] else "NO"))
    for c in clocks:
        lines.append("# %s: shader clock before %s, after %s" % (c["shape"], c["clock_before"], c["clock_after"]))
    for r in rows:
        if r["shape"] == "blobs3" and r["link"] > 2.0 * r["degree"][0]:
            lines.append("# blobs3 %s: the link sweep takes more than twice the degree step; the share of hits that went past the cheap"
                         " skip was not measured (the kernels carry no counters)" % r["way"])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return rc if rc else (0 if all(r.get("same", True) for r in rows) else 1)


if __name__ == "__main__":
    sys.exit(main())
