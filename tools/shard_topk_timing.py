#!/usr/bin/env python3
"""Top-K on a cell-range shard: the cell-pruned scan bounded through the seed layer (KNN_QUERY_TOPK_PARTIAL, option topk_cells = 1)
against the exact top-K scan the same call takes without the flag, timed with device events.  A measurement, not a gate.

Shape: the C3 set (k 16, n 2^24, fp32 rows from knn_synth_fill_device, seeds 1001 / 1000 as bench.py) split into `--ranks` cell-range
shards on ONE GPU, every rank's part of the seed layer exported and the layer attached everywhere; m 1024 queries.  The timed rank is
`--rank`; both forms run on the same index and slot, in alternating windows of enough calls to last about 50 ms, after a warm-up of
either; the median and the smallest window are reported as ms per call.  Per K it also records, from one flagged call on EVERY rank:
records per query (knn_index_last_stats()[1] / m) and the fallback flag ([2]) of the timed rank, how many ranks fell back, how many
ranks returned at least one list shorter than K, the share of all (rank, query) lists that are shorter — and it checks that the
ranks' flagged lists merge (knn_keys_topk_merge) to exactly what their full lists merge to.
usage: shard_topk_timing.py [--reps R] [--ranks N] [--rank r] [--ks K ...] [--out FILE]"""
import argparse
import json
import math
import sys

sys.path.insert(0, ".")
import torch  # noqa: E402

import multicore_hw2_amd as pkg  # noqa: E402

KS = (1, 8, 32, 64)
KEY_INIT = 0x7F80000000000000


def _window(fn, calls):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(calls):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def _calls_for(fn, target_ms=50.0):
    fn()
    torch.cuda.synchronize()
    one = max(_window(fn, 1), 1e-3)
    return max(1, min(400, math.ceil(target_ms / one)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--ks", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default="profiles/shard_topk_timing.txt")
    a = ap.parse_args()
    k, m, n = 16, 1024, 1 << 24
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    R = torch.empty(n * k, dtype=torch.float32, device=dev)
    Q = torch.empty(m * k, dtype=torch.float32, device=dev)
    pkg.synth_fill_device(R.data_ptr(), n * k, 1001)
    pkg.synth_fill_device(Q.data_ptr(), m * k, 1000)
    torch.cuda.synchronize()
    R = R.view(n, k)
    geom = pkg.KnnGeom(k, n, a.ranks, R[:: n // 4096][:4096].cpu().numpy())
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    geom.assign(R.data_ptr(), n, owner.data_ptr())
    torch.cuda.synchronize()
    idx = []
    for r in range(a.ranks):
        g = torch.nonzero(owner == r).reshape(-1)
        rows, gids = R[g].contiguous(), g.to(torch.int32)
        idx.append(pkg.KnnIndex.sharded(geom, r, rows.data_ptr(), gids.data_ptr(), rows.shape[0], owners=(rows, gids)))
    layer = torch.zeros(geom.layer_bytes, dtype=torch.uint8, device=dev)
    for ix in idx:
        ix.seed_export(layer.data_ptr())
    torch.cuda.synchronize()
    for ix in idx:
        ix.seed_attach(layer.data_ptr(), owner=layer)
    pkg.set_option("topk_cells", 1)
    lines = ["cell-range shards, top-K: rank %d of %d of the C3 set (k %d, m %d, n 2^24; %d rows on the timed rank, %d cells in the grid, "
             "layer depth %d)" % (a.rank, a.ranks, k, m, idx[a.rank].n, geom.ncells, geom.seed_tiles),
             "ms per call, median (smallest) of %d alternating windows of about 50 ms; device events; topk_cells = 1" % a.reps,
             "%4s %18s %5s %8s %3s %18s %5s %7s %9s %11s %11s" % ("K", "pruned ms", "path", "rec/q", "fb", "exact ms", "path", "x", "ranks fb",
                                                                  "ranks short", "lists short")]
    out = []
    try:
        mine = idx[a.rank]
        for K in a.ks:
            keys = torch.empty(m * K, dtype=torch.int64, device=dev)

            def pruned():
                mine.query_topk(m, K, Q.data_ptr(), keys.data_ptr(), stream=stream, init_keys=True, partial=True)

            def exact():
                mine.query_topk(m, K, Q.data_ptr(), keys.data_ptr(), stream=stream, init_keys=True)

            np_, ne = _calls_for(pruned), _calls_for(exact)
            tp, te = [], []
            for _ in range(a.reps):
                tp.append(_window(pruned, np_))
                te.append(_window(exact, ne))
            exact()
            torch.cuda.synchronize()
            st_e = mine.last_stats()
            # every rank once, flagged and not: what came back, and that the merged answers agree
            part = torch.empty((a.ranks, m, K), dtype=torch.int64, device=dev)
            full = torch.empty((a.ranks, m, K), dtype=torch.int64, device=dev)
            stats = []
            for r, ix in enumerate(idx):
                ix.query_topk(m, K, Q.data_ptr(), part[r].data_ptr(), stream=stream, init_keys=True, partial=True)
                torch.cuda.synchronize()
                stats.append(ix.last_stats())
                ix.query_topk(m, K, Q.data_ptr(), full[r].data_ptr(), stream=stream, init_keys=True)
            torch.cuda.synchronize()
            short = (part == KEY_INIT).any(dim=2)                     # [rank][query]: the list holds padding
            mp, mf = part[0].clone(), full[0].clone()
            for r in range(1, a.ranks):
                pkg.keys_topk_merge(part[r].data_ptr(), mp.data_ptr(), m, K, stream=stream)
                pkg.keys_topk_merge(full[r].data_ptr(), mf.data_ptr(), m, K, stream=stream)
            torch.cuda.synchronize()
            assert torch.equal(mp, mf), "the flagged lists do not merge to the global top-K (K %d)" % K
            tp.sort()
            te.sort()
            st = stats[a.rank]
            row = dict(K=K, pruned_ms=round(tp[len(tp) // 2], 4), pruned_min_ms=round(tp[0], 4), pruned_path=st[0],
                       records_per_query=round(st[1] / m, 2), fallback=st[2], exact_ms=round(te[len(te) // 2], 4),
                       exact_min_ms=round(te[0], 4), exact_path=st_e[0], ranks_fallback=sum(1 for s_ in stats if s_[2] != 0),
                       ranks_with_short_lists=int(short.any(dim=1).sum().item()),
                       lists_short_share=round(float(short.float().mean().item()), 4), calls_per_window=[np_, ne])
            out.append(row)
            print(json.dumps(row), flush=True)
            lines.append("%4d %9.4f (%7.4f) %4d %8.2f %3d %9.4f (%7.4f) %4d %7.1f %9d %11d %11.4f" % (
                K, row["pruned_ms"], row["pruned_min_ms"], row["pruned_path"], row["records_per_query"], row["fallback"],
                row["exact_ms"], row["exact_min_ms"], row["exact_path"], row["exact_ms"] / row["pruned_ms"], row["ranks_fallback"],
                row["ranks_with_short_lists"], row["lists_short_share"]))
    finally:
        pkg.set_option("topk_cells", 0)
        for ix in idx:
            ix.close()
        geom.close()
    lines.append("(merged answers of the flagged and the full lists: identical at every K above)")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
