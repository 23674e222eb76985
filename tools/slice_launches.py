#!/usr/bin/env python3
"""The launches of every launcher of the exact slice scans (csrc/knn_slice_launch.h: one chunk walk, one KC switch, one select
round), for comparing two builds of the library launch for launch — tools/topk_launches.py's method and its --compare.

Run (no arguments) it issues, on one stream and one workspace slot, the calls below; under
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/slice_launches.py
the trace then holds their kernels in order.  KNN_MI355X_LIB names the build under test (another commit's .so).
  forms     k = 16, 17, 128, 129 (KC 1, 2, 8, 0), n 1600, m 70, option path 1 (the exact way): the top-K scan plain and within a
            radius; the count and the list scan, scalar and with a radius per query; the large top-K (K 100) writing and folding;
            the masked top-K, count, list and large top-K (writing and folding); the self top-K plain and within, the self count
            and list, scalar and with a radius per row; the cluster call (the link sweep)
  gated     k 3, n 65536 + 70 (a grid index), 70 queries or rows, every routed call with KNN_QUERY_COUNT_GRID: the gated exact
            count and list, scalar and each; the gated self count and list, scalar and each; the gated masked count and list; the
            gated link sweep.  (The gated launches are enqueued whether or not the grid's walk gives up.  Only a grid index, k <= 3,
            puts them behind a call of this size.)
  boundary  the same index, every launcher once with 65536 + 70 queries or rows: two chunks
Each list call is the third step of count -> knn_counts_to_offsets -> list.  One JSON line per call.

  slice_launches.py --compare A.csv B.csv     (tools/topk_launches.py's: the two sequences of (kernel, grid, block), and a verdict)"""
import json
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tools")

CHUNK = 65536


def run_all():
    import numpy as np
    import torch

    import multicore_hw2_amd as pkg

    dev = torch.device("cuda:0")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(dev)
    i32 = lambda count: torch.zeros(max(count, 1), dtype=torch.int32, device=dev)
    i64 = lambda count: torch.zeros(max(count, 1), dtype=torch.int64, device=dev)

    def said(block, call, **what):
        torch.cuda.synchronize()
        print(json.dumps(dict(block=block, call=call, **what)), flush=True)

    def count_list(block, name, size, count, lst, **what):
        """count(counts) -> offsets -> lst(offsets, fill, keys) for `size` queries or rows, as a caller chains them."""
        counts, off, fill = i32(size), i64(size + 1), i32(size)
        count(counts.data_ptr())
        pkg.counts_to_offsets(counts.data_ptr(), size, off.data_ptr())
        torch.cuda.synchronize()
        keys = i64(int(off[size].item()))
        said(block, name + " count", hits=int(off[size].item()), **what)
        lst(off.data_ptr(), fill.data_ptr(), keys.data_ptr())
        said(block, name + " list", **what)

    def family(block, ix, k, n, m, Q, first, rows, r2, K=5, KL=100, cluster=True):
        """Every launcher of the family on the exact way: m queries Q, own rows first .. first + rows."""
        q = f32(Q)
        rng = np.random.default_rng(n + m)
        qr, rr = f32(np.float32(r2) * rng.random(m, dtype=np.float32)), f32(np.float32(r2) * rng.random(rows, dtype=np.float32))
        mask = torch.from_numpy(rng.integers(0, 2 ** 32, pkg.mask_words(n), dtype=np.uint32).view(np.int32)).to(dev)
        keys, large, own = i64(m * K), i64(m * KL), i64(rows * K)
        what = dict(k=k, m=m)
        ix.query_topk(m, K, q.data_ptr(), keys.data_ptr(), init_keys=True)
        said(block, "query_topk", way=ix.last_stats()[0], **what)
        ix.query_topk_within(m, K, q.data_ptr(), r2, keys.data_ptr(), init_keys=True)
        said(block, "query_topk_within", **what)
        count_list(block, "scalar", m, lambda c: ix.count_within(m, q.data_ptr(), r2, c, init=True),
                   lambda o, f, kk: ix.list_within(m, q.data_ptr(), r2, o, f, kk, init=True), **what)
        count_list(block, "each", m, lambda c: ix.count_within_each(m, q.data_ptr(), qr.data_ptr(), c, cap=r2, init=True),
                   lambda o, f, kk: ix.list_within_each(m, q.data_ptr(), qr.data_ptr(), o, f, kk, cap=r2, init=True), **what)
        for init in (True, False):
            ix.query_topk_large(m, KL, q.data_ptr(), large.data_ptr(), init_keys=init)
            said(block, "query_topk_large", init=init, **what)
        ix.query_topk_masked(m, K, q.data_ptr(), mask.data_ptr(), keys.data_ptr(), init_keys=True)
        said(block, "query_topk_masked", **what)
        count_list(block, "masked", m, lambda c: ix.count_within_masked(m, q.data_ptr(), r2, mask.data_ptr(), c, init=True),
                   lambda o, f, kk: ix.list_within_masked(m, q.data_ptr(), r2, mask.data_ptr(), o, f, kk, init=True), **what)
        for init in (True, False):
            ix.query_topk_large_masked(m, KL, q.data_ptr(), mask.data_ptr(), large.data_ptr(), init_keys=init)
            said(block, "query_topk_large_masked", init=init, **what)
        ix.self_topk(first, rows, K, own.data_ptr(), init_keys=True)
        said(block, "self_topk", way=ix.last_stats()[0], k=k, rows=rows)
        ix.self_topk(first, rows, K, own.data_ptr(), max_dist2=r2, init_keys=True)
        said(block, "self_topk within", k=k, rows=rows)
        count_list(block, "self", rows, lambda c: ix.self_count_within(first, rows, r2, c, init=True),
                   lambda o, f, kk: ix.self_list_within(first, rows, r2, o, f, kk, init=True), k=k, rows=rows)
        count_list(block, "self each", rows, lambda c: ix.self_count_within_each(first, rows, rr.data_ptr(), c, cap=r2, init=True),
                   lambda o, f, kk: ix.self_list_within_each(first, rows, rr.data_ptr(), o, f, kk, cap=r2, init=True), k=k, rows=rows)
        if cluster:
            labels = i32(n)
            ix.self_cluster_within(r2, 3, labels.data_ptr())
            said(block, "self_cluster_within", k=k, n=n)

    def gated(block, ix, k, n, m, Q, first, r2):
        """The gated twins, behind the grid way of the routed calls."""
        q = f32(Q)
        rng = np.random.default_rng(n + m + 1)
        radii = f32(np.float32(r2) * rng.random(m, dtype=np.float32))
        mask = torch.from_numpy(rng.integers(0, 2 ** 32, pkg.mask_words(n), dtype=np.uint32).view(np.int32)).to(dev)
        what = dict(k=k, m=m)
        count_list(block, "scalar grid", m, lambda c: ix.count_within(m, q.data_ptr(), r2, c, init=True, grid=True),
                   lambda o, f, kk: ix.list_within(m, q.data_ptr(), r2, o, f, kk, init=True, grid=True), **what)
        said(block, "way", way=ix.last_stats()[0])
        count_list(block, "each grid", m, lambda c: ix.count_within_each(m, q.data_ptr(), radii.data_ptr(), c, cap=r2, init=True, grid=True),
                   lambda o, f, kk: ix.list_within_each(m, q.data_ptr(), radii.data_ptr(), o, f, kk, cap=r2, init=True, grid=True), **what)
        for name, rd in (("self routed grid", None), ("self routed each grid", radii.data_ptr())):
            count_list(block, name, m,
                       lambda c: ix.self_count_within_routed(first, m, c, cap=r2, max_dist2_dev=rd, init=True, grid=True),
                       lambda o, f, kk: ix.self_list_within_routed(first, m, o, f, kk, cap=r2, max_dist2_dev=rd, init=True, grid=True), **what)
        count_list(block, "masked routed grid", m,
                   lambda c: ix.count_within_masked_routed(m, q.data_ptr(), r2, mask.data_ptr(), c, init=True, grid=True),
                   lambda o, f, kk: ix.list_within_masked_routed(m, q.data_ptr(), r2, mask.data_ptr(), o, f, kk, init=True, grid=True), **what)
        labels = i32(n)
        ix.self_cluster_within(r2, 3, labels.data_ptr(), grid=True)
        said(block, "self_cluster_within grid", way=ix.last_stats()[0], k=k, n=n)

    pkg.set_option("path", 1)
    try:
        for k in (16, 17, 128, 129):
            n, m = 1600, 70
            rng = np.random.default_rng(k)
            R = rng.random((n, k), dtype=np.float32)
            ix = pkg.KnnIndex(k, R)
            try:
                d = ((R[7:7 + m, None, :] - R[None, :64, :]) ** 2).sum(axis=2)
                family("forms", ix, k, n, m, R[7:7 + m] + np.float32(0.01), 7, m, float(np.median(d)) / 2)
            finally:
                ix.close()
    finally:
        pkg.set_option("path", 0)
    k, n = 3, CHUNK + 70
    R = np.random.default_rng(k).random((n, k), dtype=np.float32)
    ix = pkg.KnnIndex(k, R)
    try:
        gated("gated", ix, k, n, 70, R[100:170] + np.float32(0.001), 100, 0.0002)
        pkg.set_option("path", 1)
        family("boundary", ix, k, n, n, R + np.float32(0.001), 0, n, 0.0002, KL=70)   # (its cluster call sweeps two chunks of rows)
    finally:
        pkg.set_option("path", 0)
        ix.close()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        import topk_launches
        sys.exit(topk_launches.compare(sys.argv[2], sys.argv[3]))
    run_all()
