#!/usr/bin/env python3
"""Randomised differential test of the top-K calls (knn_index_query_topk, knn_index_query_topk_within) against the numpy
restatement of v0 (tests/topk_oracle.py): random families of index (the exact scan, the dense MFMA filter, the cell-pruned scan,
the grid index), layouts, shapes, K, data kinds, radii, folds, slots and flags.  usage: fuzz_topk.py [cases] [seed]
(cases per family).  Every call must give bit-exact keys and the indices of those keys, whatever way answers it and whether or
not it fell back.  Exit status 1 on the first mismatch (prints the case so it can be replayed).

Two halves: draw_run() draws the case dicts — plain values, no data, no GPU — and materialise_index() / materialise_batch() turn
them into rows, queries, the oracle's lists, the radius and the held keys, still on the CPU (tests/test_topk_fuzz_logic.py checks
both without loading the library); run_batch() makes the call."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multicore_hw2_amd as pkg                                       # noqa: E402
from fuzz_parity import make_data                                     # noqa: E402
from tests.topk_oracle import keys_dist2, topk_keys         # noqa: E402
from tests.within_helper import clip                                  # noqa: E402

FAMILIES = ("exact", "filter", "cells", "grid")
WAY = {"exact": 1, "filter": 2, "cells": 4, "grid": 3}               # knn_index_last_stats()[0] of the family's intended way
OPTIONS = ("path", "cells", "cells_rows", "cells_centre", "cells_u8_frame", "scan_deal", "topk_cells")
K_EXACT = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128, 129)
N17 = (1 << 17) + 999
FP16 = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 2, "topk_cells": 1}
BINS = {"path": 2, "cells": 1, "cells_rows": 2, "cells_u8_frame": 2, "topk_cells": 1}
CENTRED = {"path": 2, "cells": 1, "cells_rows": 1, "cells_centre": 1, "topk_cells": 1}
LAYOUTS = {"exact": {"path": 1}, "dense": {"path": 2, "cells": 2}, "grid": {}, "fp16": FP16, "bins": BINS, "centred": CENTRED}
SHAPES = {   # family: (rows, dimensions, indexes a run builds — its cases share them, so a case buys calls and not builds)
    "exact": ((1, 5, 63, 1000, 4097, 20000), K_EXACT, 10),
    "filter": ((66000, 70001), (3, 16, 20, 32, 40, 64, 100, 128), 6),
    "cells": ((N17, 150001), (8, 12, 16, 17, 20), 4),
    "grid": ((40000, 100000), (2, 3, 4), 4),
}
MS = (1, 5, 33, 64, 100)
M_TILED, M_TILED_DISTINCT = 1031, 96                                   # cells: two passes, 96 distinct queries tiled
K_EDGES = (1, 2, 3, 31, 32, 33, 63, 64)
# rows: the kinds of tools/fuzz_parity.py.  `tight` and `onepoint` overflow the filter's candidates by construction: with a
# non-finite query (P_BAD_QUERY) and a far query (P_FAR_QUERY) they are the inputs that fall back by design, together under 1/4
ROW_KINDS = ("uniform", "uniform", "uniform", "gauss", "gauss", "mixture", "clusters", "heavy", "lowrank", "grid", "offset")
# (the grid family: a grid index is ruled out — and the filter or the exact scan answers — when a cell would hold more than 4096
# rows or the rows' box is not finite, i.e. for lattices, far offsets, heavy tails, tight clusters and any non-finite row; its mix
# leans towards the kinds that get one)
GRID_ROW_KINDS = ("uniform", "uniform", "uniform", "uniform", "gauss", "gauss", "gauss", "mixture", "mixture", "mixture", "lowrank",
                  "lowrank", "clusters", "heavy")
BY_DESIGN_KINDS = ("tight", "onepoint")
P_BY_DESIGN_KIND, P_BAD_QUERY, P_FAR_QUERY, P_BAD_ROW, P_COINCIDE = 0.08, 0.06, 0.06, 0.15, 0.3
P_GRID_FLAG = 0.9     # (a call without KNN_QUERY_TOPK_GRID takes the exact scan: at one half the grid could not answer half the calls)
RADII = ("quantile", "held", "below", "zero", "under_all")
# the runs tests/test_topk_fuzz_gpu.py makes: family -> (seed, cases)
SUITE_RUNS = {"exact": (20261, 30), "filter": (20272, 16), "cells": (20273, 12), "grid": (20494, 20)}


CELL_LAYOUTS = ("fp16", "bins", "centred", "fp16")


def draw_index(rng, family, i=None):
    """An index of the family; i: its place in a run's pool — the pool walks through the family's row counts and, for `cells`,
    its layouts, so that a run has them all whatever the seed."""
    rows, dims, _ = SHAPES[family]
    n = int(rng.choice(rows)) if i is None else rows[i % len(rows)]
    k = int(rng.choice(dims))
    layout = {"exact": "exact", "filter": "dense", "grid": "grid"}.get(family)
    if family == "cells":   # 8-bit rows and per-cell frames: k <= 16
        layout = str(rng.choice(CELL_LAYOUTS)) if i is None else CELL_LAYOUTS[i % len(CELL_LAYOUTS)]
        if layout != "fp16":
            k = int(rng.choice([d for d in dims if d <= 16]))
    kind = str(rng.choice(BY_DESIGN_KINDS)) if rng.random() < P_BY_DESIGN_KIND else str(rng.choice(GRID_ROW_KINDS if family == "grid" else ROW_KINDS))
    bad_row = str(rng.choice(["nan", "inf", "-inf", "3e38"])) if rng.random() < P_BAD_ROW else None
    return dict(family=family, layout=layout, k=k, n=n, kind=kind, base=int(rng.choice([0, 7, 1 << 20])), bad_row=bad_row,
                data_seed=int(rng.integers(0, 1 << 31)))


def draw_batch(rng, ix):
    family = ix["family"]
    m = int(rng.choice(MS + (M_TILED,) if family == "cells" else MS))
    K = int(rng.choice(K_EDGES)) if rng.random() < 0.6 else int(rng.integers(1, 65))
    b = dict(m=m, K=K, slot=int(rng.integers(0, 2)), data_seed=int(rng.integers(0, 1 << 31)))
    b["queries"] = str(rng.choice(["rows_jittered", "same_kind"]))
    b["jitter"] = float(rng.choice([0.0, 1e-3, 1e-1]))
    b["coincide"] = bool(rng.random() < P_COINCIDE)
    b["bad_query"] = str(rng.choice(["nan", "inf", "1e30"])) if rng.random() < P_BAD_QUERY else None
    b["far_query"] = bool(rng.random() < P_FAR_QUERY)
    b["call"] = str(rng.choice(["plain", "within"]))
    b["radius"] = (str(rng.choice(RADII)), float(rng.random()))
    b["fold"] = bool(rng.random() < 0.4)
    b["grid"] = bool(family == "grid" and rng.random() < P_GRID_FLAG)
    b["frames"] = bool(ix["layout"] == "centred" and rng.random() < 0.75)
    b["scan_deal"] = int(rng.integers(1, 3)) if ix["layout"] == "fp16" else 0
    return b


def one_case(rng, case, family, indexes=None):
    """One case: an index (of `indexes`, or drawn) and two different batches, one after the other on the same index and slot."""
    which = int(rng.integers(0, len(indexes))) if indexes else None
    ix = indexes[which] if indexes else draw_index(rng, family)
    first, second = draw_batch(rng, ix), draw_batch(rng, ix)
    second["slot"] = first["slot"]
    return dict(case=case, family=family, index=which, spec=ix, batches=[first, second])


def draw_run(seed, family, cases):
    """(indexes, cases) of a seeded run of one family."""
    rng = np.random.default_rng([int(seed), FAMILIES.index(family)])
    indexes = [draw_index(rng, family, i) for i in range(SHAPES[family][2])]
    return indexes, [one_case(rng, c, family, indexes) for c in range(cases)]


def by_design(ix, b):
    """The batch falls back by design: its rows' kind, a non-finite query or a far one."""
    return ix["kind"] in BY_DESIGN_KINDS or b["bad_query"] is not None or b["far_query"]


BAD = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "3e38": 3e38, "1e30": 1e30}


def materialise_index(ix, rows_cap=None):
    """The rows of a drawn index (rows_cap: only that many — for checks of the generator that need no full shard)."""
    rng = np.random.default_rng(ix["data_seed"])
    n = ix["n"] if rows_cap is None else min(ix["n"], rows_cap)
    R = make_data(rng, ix["kind"], n, ix["k"])
    if ix["bad_row"]:
        R[rng.integers(0, n), rng.integers(0, ix["k"])] = np.float32(BAD[ix["bad_row"]])
    return np.ascontiguousarray(R, dtype=np.float32)


def radius_of(kind, u, want):
    """The radius of a drawn (kind, u) from the oracle's lists: a quantile of their distances, a value a row holds exactly, the
    next float below it, 0, or a value below every distance."""
    d = keys_dist2(want)
    held = np.unique(d[d < np.float32(np.inf)])
    if kind == "zero" or held.size == 0:
        return 0.0
    if kind == "under_all":
        return float(np.float32(held[0] * np.float32(0.5)))
    if kind == "quantile":
        return float(np.float32(np.quantile(held.astype(np.float64), u)))
    v = held[min(held.size - 1, int(u * held.size))]
    return float(v if kind == "held" else np.nextafter(v, np.float32(0)))


def materialise_batch(ix, R, b, R_cols=None):
    """Queries, the oracle's lists, the radius and the held keys of a drawn batch against rows R (R_cols: the same rows in
    column-major order, which the oracle's per-dimension passes read many times faster)."""
    rng = np.random.default_rng(b["data_seed"])
    k, n = ix["k"], R.shape[0]
    tiled = b["m"] == M_TILED
    m0 = M_TILED_DISTINCT if tiled else b["m"]
    finite = R[(np.abs(R) < np.float32(1e30)).all(axis=1)]   # (not NaN, not INF, not the stray 3e38)
    if finite.shape[0] == 0:
        finite = np.zeros((1, k), dtype=np.float32)
    spread = finite.astype(np.float64).std(axis=0).astype(np.float32)

    def near_rows(count, jitter):
        return (finite[rng.integers(0, finite.shape[0], count)] + rng.normal(0, 1, (count, k)) * jitter * spread).astype(np.float32)
    if b["queries"] == "same_kind" and ix["kind"] in ("uniform", "gauss", "grid", "heavy"):
        Q = make_data(rng, ix["kind"], m0, k)
    else:   # (the other kinds draw hidden centres and offsets: a second draw of the kind would lie somewhere else)
        Q = near_rows(m0, b["jitter"])
    if b["coincide"]:
        c = min(m0, 8)
        Q[:c] = finite[rng.integers(0, finite.shape[0], c)]
    if b["bad_query"]:
        Q[rng.integers(0, m0), rng.integers(0, k)] = np.float32(BAD[b["bad_query"]])
    if b["far_query"]:
        Q[rng.integers(0, m0)] = np.float32(1e6)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    K = b["K"]
    want = topk_keys(Q, R if R_cols is None else R_cols, k, K, base=ix["base"])
    out = dict(Q=Q, m0=m0, rep=np.arange(b["m"]) % m0, want=want, r2=None, held=None)
    exp = want
    if b["call"] == "within":
        out["r2"] = radius_of(b["radius"][0], b["radius"][1], want)
        exp = clip(want, out["r2"])
    if b["fold"]:   # another shard's plain top-K of the same queries, its global numbers beyond this shard's
        out["held_base"] = ix["base"] + ix["n"] + 1000
        out["held"] = topk_keys(Q, near_rows(300, 0.1), k, K, base=out["held_base"])
        exp = np.sort(np.concatenate([out["held"], exp], axis=1), axis=1)[:, :K]
    out["expect"] = exp
    return out


# ---- the GPU half ---------------------------------------------------------------------------------------------------------------

def set_options(ix, b):
    opts = dict(LAYOUTS[ix["layout"]], scan_deal=b["scan_deal"]) if b else LAYOUTS[ix["layout"]]
    for name in OPTIONS:
        pkg.set_option(name, opts.get(name, 0))


def reset_options():
    for name in OPTIONS:
        pkg.set_option(name, 0)


def build_index(ix, R):
    set_options(ix, None)
    return pkg.KnnIndex(ix["k"], R, base_index=ix["base"])


def run_batch(handle, ix, b, mat):
    """The call of a materialised batch: (keys are bit-exact and the indices theirs, last_stats)."""
    import torch
    from tests.within_helper import dev, dev_keys, host_keys, within
    from tests.topk_oracle import keys_index
    set_options(ix, b)
    m, K, rep = b["m"], b["K"], mat["rep"]
    Q = mat["Q"][rep]
    keys = dev_keys(m, K, fill=mat["held"][rep]) if b["fold"] else None
    flags = dict(grid=b["grid"], frames=b["frames"])
    if b["call"] == "within":
        assert mat["r2"] >= 0.0
        got = within(handle, Q, K, mat["r2"], keys=keys, init=not b["fold"], slot=b["slot"], **flags)
    else:
        q_d = torch.from_numpy(Q.reshape(-1)).to(dev())
        keys = dev_keys(m, K) if keys is None else keys
        ind = torch.full((m * K,), -7, dtype=torch.int32, device=dev())
        torch.cuda.synchronize()
        handle.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=not b["fold"], indices_dev=ind.data_ptr(), slot=b["slot"],
                          **flags)
        torch.cuda.synchronize()
        got = host_keys(keys, m, K)
        np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return bool((got == mat["expect"][rep]).all()), handle.last_stats(), got


class Runner:
    """Runs drawn cases, building each index once; tallies the ways and the fallbacks of the calls."""

    def __init__(self):
        self.open = {}
        self.calls = self.intended = 0
        self.ways = {}

    def index(self, case):
        key = case["index"] if case["index"] is not None else ("own", case["case"])
        if key not in self.open:
            R = materialise_index(case["spec"])
            self.open[key] = (build_index(case["spec"], R), R, np.asfortranarray(R))
        return key, self.open[key]

    def run(self, case):
        key, (handle, R, R_cols) = self.index(case)
        ix = case["spec"]
        ok = True
        for b in case["batches"]:
            mat = materialise_batch(ix, R, b, R_cols)
            good, st, got = run_batch(handle, ix, b, mat)
            self.calls += 1
            self.intended += int(st[0] == WAY[ix["family"]] and st[2] == 0)
            self.ways[(st[0], int(st[2] != 0))] = self.ways.get((st[0], int(st[2] != 0)), 0) + 1
            if not good:
                j = int(np.flatnonzero((got != mat["expect"][mat["rep"]]).any(axis=1))[0])
                print("MISMATCH", case, "failing batch", b, "r2", mat["r2"], "stats", st, "query", j, "got", got[j],
                      "want", mat["expect"][mat["rep"]][j], flush=True)
                ok = False
                break
        if case["index"] is None:
            self.close(key)
        return ok

    def close(self, key=None):
        for k in [key] if key is not None else list(self.open):
            self.open.pop(k)[0].close()
        if key is None:
            reset_options()

    def tally(self):
        return "%d of %d calls on the intended way without fallback; (way, fell back): %s" % (
            self.intended, self.calls, dict(sorted(self.ways.items())))


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 12345
    t0 = time.time()
    for family in FAMILIES:
        runner = Runner()
        try:
            for case in draw_run(seed, family, cases)[1]:
                if not runner.run(case):
                    return 1
        finally:
            runner.close()
        print("%s: %d cases bit-exact, %.0f s; %s" % (family, cases, time.time() - t0, runner.tally()), flush=True)
    print("all %d cases per family bit-exact (seed %d)" % (cases, seed))
    return 0


if __name__ == "__main__":
    sys.exit(main())
