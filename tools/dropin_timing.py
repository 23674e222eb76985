#!/usr/bin/env python3
"""PCIe-inclusive timing of the drop-in entry: wall clock around cudaCallback exactly as the
reference's harness times it (main.cu:69-73), host pageable inputs, all visible GPUs."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multicore_hw2_amd as pkg              # noqa: E402
from tests.oracle_lib import Oracle           # noqa: E402

o = Oracle(os.path.join(ROOT, "oracle", "libknn_oracle.so"))
shapes = [(3, 1, 1 << 24), (16, 1, 1 << 24), (3, 1024, 1 << 20), (16, 1024, 1 << 20), (16, 1024, 1 << 24)]
# usage: dropin_timing.py [--reps N] [--samples S] [k,m,n ...] — a sample is N calls back to back (small shapes: enough of
# them that a sample spans a good fraction of a second), reported per call
args, reps, samples = sys.argv[1:], 1, 3
while args and args[0] in ("--reps", "--samples"):
    if args[0] == "--reps":
        reps = int(args[1])
    else:
        samples = int(args[1])
    args = args[2:]
if args:
    shapes = [tuple(int(t) for t in a.split(",")) for a in args]
print(f"library {pkg.lib_path}, {reps} call(s) per sample, {samples} samples", flush=True)
for k, m, n in shapes:
    Q, R = o.synth(m * k, 1000), o.synth(n * k, 1001)
    pkg.cudaCallback(k, 1, 1024, Q[:k], R[:1024 * k])          # warm the runtime
    ts = []
    for _ in range(samples):
        t0 = time.perf_counter()
        for _ in range(reps):
            out = pkg.cudaCallback(k, m, n, Q, R)
        ts.append((time.perf_counter() - t0) / reps)
    sel = np.random.default_rng(0).choice(m, min(m, 8), replace=False)
    ok = (out[sel] == o.v0(k, Q.reshape(m, k)[sel], R)).all()
    gb = 4.0 * k * (n + m) / 1e9
    print(f"cudaCallback(k={k}, m={m}, n={n}): best {min(ts) * 1e3:9.4f} ms median {float(np.median(ts)) * 1e3:9.4f} ms of "
          f"{[round(t * 1e3, 4) for t in ts]} ({gb / min(ts):.1f} GB/s of host input, {m / min(ts):.0f} queries/s), "
          f"bit-exact on sample: {ok}", flush=True)
