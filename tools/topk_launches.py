#!/usr/bin/env python3
"""The launches of a top-K call on every way and form, and of the cell-pruned scan's three kinds of pass, for comparing two
builds of the library launch for launch.

Run (no arguments) it issues, on one stream and one workspace slot, the calls below; under
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/topk_launches.py
the trace then holds their kernels in order.  KNN_MI355X_LIB names the build under test (another commit's .so).
  filter  k 16, n 70000, options path 2, cells 2 (the dense filter way)   (m, K) = (8, 2), (40, 64)
  exact   the same index with option path 1                               (m, K) = (8, 2), (40, 64)
  cells   k 16, n 2^17 + 999, fp16 one-frame cell-sorted layout, option topk_cells 1 (two passes)   (m, K) = (1100, 8)
  grid    k 3, n 16384 (the smallest shard that gets a grid index), KNN_QUERY_TOPK_GRID   (m, K) = (70, 2), (70, 64)
Each (index, m, K): a plain call and a call with a finite radius (the median 1-NN distance of the batch), each once writing
its keys and once folding into them.  The cells index then answers one 1-NN call (two batches) and one count call with
KNN_QUERY_COUNT_CELLS at that radius (two passes) of the same m = 1100 queries: with its top-K passes, all three drivers of the
cell-pruned scan.  Each call's way (knn_index_last_stats()[0]) is printed as one JSON line.
  one-way  k 3, n 2000 (no layout): knn_index_query_topk_large and _large_masked (m, K) = (20, 100), _masked (20, 5) and
           knn_index_self_topk on its exact branch (rows 7 .. 26, K 5), each once writing its keys and once folding into them; then
           one call of each of their three host calls and of the list host calls — knn_index_list_within_host, _masked_host,
           knn_index_self_list_within_host and _routed_host (a radius per row) — at a radius of a few hits per row

  topk_launches.py --compare A.csv B.csv
reads two such kernel traces and prints the sequences of (kernel, grid, block) of the library's kernels and whether they are
equal; exit status 1 when they differ."""
import csv
import json
import sys

sys.path.insert(0, ".")


def calls():
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    dev = torch.device("cuda:0")
    options = ("path", "cells", "cells_rows", "cells_centre", "topk_cells")
    indexes = [
        ("filter", 16, 70000, {"path": 2, "cells": 2}, {}, [(8, 2), (40, 64)], {}),
        ("exact", 16, 70000, {"path": 2, "cells": 2}, {"path": 1}, [(8, 2), (40, 64)], {}),
        ("cells", 16, (1 << 17) + 999, {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2}, {"topk_cells": 1}, [(1100, 8)], {}),
        ("grid", 3, 16384, {}, {}, [(70, 2), (70, 64)], {"grid": True}),
    ]
    for name, k, n, build_opts, call_opts, shapes, flags in indexes:
        for o in options:
            pkg.set_option(o, 0)
        for o, v in build_opts.items():
            pkg.set_option(o, v)
        rng = np.random.default_rng(n + k)
        R = rng.random((n, k), dtype=np.float32)
        ix = pkg.KnnIndex(k, R)
        for o, v in call_opts.items():
            pkg.set_option(o, v)
        try:
            for m, K in shapes:
                q = torch.from_numpy(rng.random((m, k), dtype=np.float32).reshape(-1)).to(dev)
                keys = torch.empty(m * K, dtype=torch.int64, device=dev)
                ix.query_topk(m, K, q.data_ptr(), keys.data_ptr(), init_keys=True, **flags)
                torch.cuda.synchronize()
                d2 = (keys.cpu().numpy().view(np.uint64).reshape(m, K)[:, 0] >> np.uint64(32)).astype(np.uint32).view(np.float32)
                r2 = float(np.median(d2))
                for radius in (None, r2):
                    for init in (True, False):
                        if radius is None:
                            ix.query_topk(m, K, q.data_ptr(), keys.data_ptr(), init_keys=init, **flags)
                        else:
                            ix.query_topk_within(m, K, q.data_ptr(), radius, keys.data_ptr(), init_keys=init, **flags)
                        torch.cuda.synchronize()
                        print(json.dumps(dict(index=name, m=m, K=K, radius=radius, init=init, way=ix.last_stats()[0])), flush=True)
                if name == "cells":
                    ix.query_keys(m, q.data_ptr(), keys.data_ptr(), init_keys=True)
                    torch.cuda.synchronize()
                    print(json.dumps(dict(index=name, call="query_keys", m=m, way=ix.last_stats()[0])), flush=True)
                    counts = torch.empty(m, dtype=torch.int32, device=dev)
                    ix.count_within(m, q.data_ptr(), r2, counts.data_ptr(), init=True, cells=True)
                    torch.cuda.synchronize()
                    print(json.dumps(dict(index=name, call="count_within", m=m, radius=r2, way=ix.last_stats()[0])), flush=True)
        finally:
            ix.close()
    for o in options:
        pkg.set_option(o, 0)
    one_way_calls(pkg, np, torch, dev)


def one_way_calls(pkg, np, torch, dev):
    """The one-way top-K entries and the staged host calls (the docstring's last block)."""
    k, n, m, first, r2 = 3, 2000, 20, 7, 0.007
    rng = np.random.default_rng(n + k)
    R = rng.random((n, k), dtype=np.float32)
    Q = R[first:first + m].copy()
    ix = pkg.KnnIndex(k, R)
    try:
        q = torch.from_numpy(Q.reshape(-1)).to(dev)
        words = np.full(pkg.mask_words(n), 0xFFFFFFFF, dtype=np.uint32)
        mask = torch.from_numpy(words.view(np.int32)).to(dev)
        for entry, K in (("query_topk_large", 100), ("query_topk_masked", 5), ("query_topk_large_masked", 100), ("self_topk", 5)):
            keys = torch.empty(m * K, dtype=torch.int64, device=dev)
            for init in (True, False):
                if entry == "query_topk_large":
                    ix.query_topk_large(m, K, q.data_ptr(), keys.data_ptr(), init_keys=init)
                elif entry == "query_topk_masked":
                    ix.query_topk_masked(m, K, q.data_ptr(), mask.data_ptr(), keys.data_ptr(), init_keys=init)
                elif entry == "query_topk_large_masked":
                    ix.query_topk_large_masked(m, K, q.data_ptr(), mask.data_ptr(), keys.data_ptr(), init_keys=init)
                else:
                    ix.self_topk(first, m, K, keys.data_ptr(), init_keys=init)
                torch.cuda.synchronize()
                print(json.dumps(dict(index="one-way", call=entry, m=m, K=K, init=init, way=ix.last_stats()[0])), flush=True)
        radii = (np.float32(r2) * (np.float32(0.5) + np.float32(0.5) * rng.random(n, dtype=np.float32))).astype(np.float32)
        host_calls = (
            ("query_topk_large_host", lambda: ix.query_topk_large_host(Q, 100, max_dist2=r2)),
            ("query_topk_masked_host", lambda: ix.query_topk_masked_host(Q, 5, words, max_dist2=r2)),
            ("query_topk_large_masked_host", lambda: ix.query_topk_large_masked_host(Q, 100, words, max_dist2=r2)),
            ("list_within_host", lambda: ix.list_within_host(Q, r2)),
            ("list_within_masked_host", lambda: ix.list_within_masked_host(Q, r2, words)),
            ("self_list_within_host", lambda: ix.self_list_within_host(r2)),
            ("self_list_within_routed_host", lambda: ix.self_list_within_routed_host(r2, max_dist2=radii)),
        )
        for name, call in host_calls:
            call()
            print(json.dumps(dict(index="one-way", call=name, way=ix.last_stats()[0])), flush=True)
    finally:
        ix.close()


def sequence(path):
    """[(kernel, grid, block)] of the library's kernels of a rocprofv3 kernel trace, in dispatch order."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "knn_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    dims = lambda r, what: "x".join(r["%s_Size_%s" % (what, a)] for a in "XYZ")
    name = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
    return [(name(r), dims(r, "Grid"), dims(r, "Workgroup")) for r in rows]


def compare(a_path, b_path):
    a, b = sequence(a_path), sequence(b_path)
    for tag, path, seq in (("A", a_path, a), ("B", b_path, b)):
        print("%s: %s — %d launches" % (tag, path, len(seq)))
        for i, (name, grid, block) in enumerate(seq):
            print("%s %4d  %-96s grid %-16s block %s" % (tag, i, name, grid, block))
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    if first is None and a:
        print("verdict: EQUAL — %d launches, the same (kernel, grid, block) in the same order" % len(a))
        return 0
    print("verdict: DIFFERENT at launch %s (A %d launches, B %d)" % (first, len(a), len(b)))
    return 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    calls()
