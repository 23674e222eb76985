"""The radius graph on the grid and cell-pruned ways (knn_index_self_count_within_routed, knn_index_self_list_within_routed, the
host call and knn_debug_self_routed_plan; include/knn_mi355x.h 2k) without a GPU: the exported names, the argument rules of the two
device calls in the header's order, the three flags they admit, and the plan — knn_debug_count_plan's for `rows` queries with the
self-scan's slices."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EINVAL = -1
INF = float("inf")
NAN = float("nan")
vp = ctypes.c_void_p
NAMES = ("knn_index_self_count_within_routed", "knn_index_self_list_within_routed", "knn_index_self_list_within_routed_host",
         "knn_debug_self_routed_plan")
INIT, PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS = 1, 2, 4, 8, 16, 32
FLAGS_TEXT = "unknown flag (KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS)"
CAP_TEXT = "cap must be >= 0 (or +INF) and not NaN"


def test_the_four_names_are_declared_under_2k_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    at = header.index("2k. The radius graph on the grid and cell-pruned ways")
    assert at > header.index("2j. A radius per query")
    for name in NAMES:
        m = re.search(r"^int %s\s*\(" % name, header, flags=re.M)
        assert m and m.start() > at, name
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    for name in ("self_count_within_routed_c", "self_list_within_routed_c", "self_list_within_routed_host_c", "debug_self_routed_plan"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("self_count_within_routed", "self_list_within_routed", "self_list_within_routed_host"):
        assert callable(getattr(pkg.KnnIndex, name)), name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for proto in (
            "int knn_index_self_count_within_routed(knn_index *idx, int slot, long long row_first, int rows, "
            "const float *max_dist2_dev , float cap, unsigned *counts_dev , void *stream, unsigned flags);",
            "int knn_index_self_list_within_routed(knn_index *idx, int slot, long long row_first, int rows, "
            "const float *max_dist2_dev , float cap, const unsigned long long *offsets_dev , unsigned *fill_dev , "
            "unsigned long long *keys_dev, void *stream, unsigned flags);",
            "int knn_index_self_list_within_routed_host(knn_index *idx, const float *max_dist2_host, float cap, unsigned flags, "
            "long long *offsets_host , int **indices_out, float **dist2_out );",
            "int knn_debug_self_routed_plan(const long long in[16], long long out[8]);"):
        assert proto in flat, proto


def _walk(who, rc, steps):
    """steps: (keyword overrides that break ONE more rule than the step before, the text that must speak).  Every earlier rule's
    breakage is mended in turn, so each text shows alone, in the header's order; the index — null throughout — speaks last."""
    broken = {}
    for over, _ in steps:
        broken.update(over)
    for over, text in steps:
        assert rc(**broken) == (EINVAL, who + text), (who, text)
        for key in over:                      # mend this rule: the next one speaks
            del broken[key]
    assert not broken
    assert rc() == (EINVAL, who + "null index")


def _cap_and_flag_rules(who, rc):
    assert rc(cap=NAN)[1] == who + CAP_TEXT and rc(cap=-1e-30)[1] == who + CAP_TEXT
    for cap in (-0.0, 0.0, 1.0, INF):         # -0 and +INF pass the first rule: the index speaks
        assert rc(cap=cap) == (EINVAL, who + "null index"), cap
    for flags in (PARTIAL, GRID, FRAMES, 64, 1 << 31, INIT | PARTIAL, COUNT_CELLS | FRAMES):
        assert rc(flags=flags)[1] == who + FLAGS_TEXT, flags
    for flags in (0, INIT, COUNT_GRID, COUNT_CELLS, INIT | COUNT_GRID | COUNT_CELLS):
        assert rc(flags=flags) == (EINVAL, who + "null index"), flags
    assert rc(radii=None) == (EINVAL, who + "null index")        # the scalar form: no radii is no error


def test_the_count_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    r, c = vp(0x2000), vp(0x3000)

    def rc(slot=0, row_first=0, rows=7, radii=r, cap=1.0, counts=c, flags=INIT):
        return (pkg.self_count_within_routed_c()(None, slot, row_first, rows, radii, cap, counts, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_self_count_within_routed: "
    _walk(who, rc, [
        (dict(cap=-0.5), CAP_TEXT),
        (dict(flags=GRID), FLAGS_TEXT),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(rows=0), "rows < 1"),
        (dict(row_first=-1), "row_first < 0"),
        (dict(counts=None), "null counts"),
    ])
    _cap_and_flag_rules(who, rc)
    assert rc(rows=0, row_first=-1)[1] == who + "rows < 1"
    assert rc(slot=-1)[1] == who + "slot outside 0 .. 7" and rc(rows=-3)[1] == who + "rows < 1"


def test_the_list_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    r, o, f, k = vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000)

    def rc(slot=0, row_first=0, rows=7, radii=r, cap=1.0, offsets=o, fill=f, keys=k, flags=INIT):
        return (pkg.self_list_within_routed_c()(None, slot, row_first, rows, radii, cap, offsets, fill, keys, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_self_list_within_routed: "
    _walk(who, rc, [
        (dict(cap=NAN), CAP_TEXT),
        (dict(flags=FRAMES), FLAGS_TEXT),
        (dict(slot=-2), "slot outside 0 .. 7"),
        (dict(rows=-1), "rows < 1"),
        (dict(row_first=-7), "row_first < 0"),
        (dict(keys=None), "null offsets, fill or keys"),
    ])
    _cap_and_flag_rules(who, rc)
    assert rc(offsets=None)[1] == who + "null offsets, fill or keys" and rc(fill=None)[1] == who + "null offsets, fill or keys"


def test_the_host_call_rejects_its_bad_arguments_without_a_gpu():
    L = pkg.lib()
    f = pkg.self_list_within_routed_host_c()
    who = "knn_index_self_list_within_routed_host: "
    off = (ctypes.c_longlong * 2)()
    ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
    good = [None, None, 1.0, COUNT_CELLS, ctypes.cast(off, vp), ctypes.byref(ind), ctypes.byref(d2)]
    for pos, value, text in ((2, NAN, CAP_TEXT), (2, -1.0, CAP_TEXT), (3, GRID, FLAGS_TEXT), (3, 64, FLAGS_TEXT),
                             (4, None, "null offsets or indices"), (5, None, "null offsets or indices")):
        args = list(good)
        args[pos] = value
        assert f(*args) == EINVAL and L.knn_last_error().decode() == who + text, (pos, value)
    assert f(*good) == EINVAL and L.knn_last_error().decode() == who + "null index"
    bad = list(good)
    bad[2], bad[3], bad[4] = -1.0, GRID, None       # the cap speaks before the flag, the flag before the pointers
    assert f(*bad) == EINVAL and L.knn_last_error().decode() == who + CAP_TEXT


def _inputs(**over):
    base = dict(k=16, m=1025, n=1 << 20, radius_finite=1, flag_grid=0, flag_cells=0, has_grid=0, has_cells=0, centred=0, rows_u8=0,
                bins=0, sharded=0, path=0, cells=0, num_cu=256, radius_rings=0)
    base.update(over)
    return base


# the layouts an index can have: none; a one-frame fp16 cell layout; per-cell frames (fp16, 8-bit rows); 8-bit rows in bin frames;
# a cell-range shard's layout; a grid index (k <= 4, never sharded)
LAYOUTS = [
    ("none", dict()),
    ("cells_fp16", dict(has_cells=1)),
    ("cells_frames", dict(has_cells=1, centred=1)),
    ("cells_frames_u8", dict(has_cells=1, centred=1, rows_u8=1)),
    ("cells_bins", dict(has_cells=1, rows_u8=1, bins=1)),
    ("shard", dict(has_cells=1, sharded=1)),
    ("grid", dict(k=3, has_grid=1, radius_rings=9)),
    ("grid_far", dict(k=3, has_grid=1, radius_rings=40000)),
    ("grid_and_cells", dict(k=4, has_grid=1, has_cells=1, radius_rings=3)),
]


@pytest.mark.parametrize("name,layout", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_the_plan_is_the_count_calls_plan_with_the_self_scans_slices(name, layout):
    ways = set()
    for rows, finite, (fg, fc), path, cells in itertools.product((4, 5, 1025), (0, 1), ((0, 0), (1, 0), (0, 1), (1, 1)), range(4),
                                                                 range(3)):
        inp = _inputs(m=rows, radius_finite=finite, flag_grid=fg, flag_cells=fc, path=path, cells=cells, **layout)
        if not finite:
            inp["radius_rings"] = 0
        got = pkg.debug_self_routed_plan(**inp)
        want = pkg.debug_count_plan(**inp)
        slices = pkg.debug_self_plan(k=inp["k"], rows=rows, K=0, shard_rows=inp["n"], num_cu=inp["num_cu"], init=1)["slices"]
        for key in pkg.COUNT_PLAN:
            assert got[key] == (slices if key == "slices" else want[key]), (inp, key, got, want)
        ways.add(got["way"])
        # the rules a caller relies on, restated: no flag is way 1; the cell way needs a finite cap, rows >= 5, a one-frame layout
        if not (fg or fc):
            assert got["way"] == 1, inp
        if got["way"] == 4:
            assert fc and finite and rows >= 5 and cells != 2 and path in (0, 2) and got["pass_m"] == min(rows, 1024), inp
            assert got["passes"] == (rows + 1023) // 1024 and got["scratch_bytes"] == 4 * rows
        if got["way"] == 3:
            assert fg and path in (0, 3) and got["scratch_bytes"] == 4 * rows and got["blocks"] == (rows + 3) // 4, inp
    expect = {"none": {1}, "cells_fp16": {1, 4}, "cells_frames": {1}, "cells_frames_u8": {1}, "cells_bins": {1, 4}, "shard": {1, 4},
              "grid": {1, 3}, "grid_far": {1, 3}, "grid_and_cells": {1, 3, 4}}[name]
    assert ways == expect, (name, ways)


def test_the_plan_refuses_rows_outside_the_shard_and_the_count_plans_bad_inputs():
    L = pkg.lib()
    who = "knn_debug_self_routed_plan: bad arguments"
    for over in (dict(m=0), dict(m=9, n=8), dict(n=(1 << 32) + 1, m=5), dict(path=4), dict(cells=3), dict(num_cu=0), dict(k=0),
                 dict(k=5, has_grid=1), dict(k=3, has_grid=1, sharded=1), dict(centred=2)):
        with pytest.raises(pkg.KnnError):
            pkg.debug_self_routed_plan(**_inputs(**over))
        assert L.knn_last_error().decode().startswith(who), over
    assert pkg.debug_self_routed_plan(**_inputs(m=8, n=8))["way"] == 1          # the whole shard is inside the shard


# ---- what the compiler made of the new kernels ---------------------------------------------------------------------------

FLOAT_FMA = re.compile(r"\bv_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_f32|\bv_dot\d")
# a new kernel -> the kernel it is a form of: (file, new name, twin's name)
TWINS = (("knn_grid", "knn_grid_self_count_kernel", "knn_grid_each_count_kernel"),
         ("knn_grid", "knn_grid_self_list_kernel", "knn_grid_each_list_kernel"),
         ("knn_self", "knn_self_count_gated_kernel", "knn_self_count_each_kernel"),
         ("knn_self", "knn_self_list_gated_kernel", "knn_self_list_each_kernel"),
         ("knn_self_routed", "knn_count_self_rerank_kernel", "knn_count_each_rerank_kernel"),
         ("knn_self_routed", "knn_count_self_outlier_kernel", "knn_count_each_outlier_kernel"),
         ("knn_self_routed", "knn_list_self_rerank_kernel", "knn_list_each_rerank_kernel"),
         ("knn_self_routed", "knn_list_self_outlier_kernel", "knn_list_each_outlier_kernel"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_the_new_kernels_use_no_scratch_no_fused_multiply_add_and_stay_beside_their_twins_registers(tmp_path):
    """The list forms' hit path is the long one (knn_self.hip's note on self_scan_one): a self form may take a register or two for
    the own row and the drop, never a wave of occupancy — below 64 VGPRs a SIMD holds its 8 waves whatever the count, above it a
    form must stay within its twin's allocation granule of 8."""
    names = ("knn_grid", "knn_self", "knn_self_routed", "knn_each")
    procs = []
    for name in names:     # (tests/test_each_logic.py's command)
        src = os.path.join(ROOT, "multicore_hw2_amd", "csrc", name + ".hip")
        procs.append(subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
                                       "--cuda-device-only", "-o", str(tmp_path / (name + ".s")), src]))
    meta, text = {}, ""
    for name, p in zip(names, procs):
        assert p.wait() == 0, name
        one = (tmp_path / (name + ".s")).read_text()
        text += one
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", one, flags=re.S):
            meta[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1)),
                                int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)))
    seen = 0
    for _, new, twin in TWINS:
        mine = sorted(n for n in meta if new in n)
        # 8 grid forms (k 1 .. 4, scalar and per-row radius), 9 gated scans (KC 0 .. 8), one of each re-rank and out-of-box kernel
        assert len(mine) == (8 if "grid" in new else 9 if "gated" in new else 1), (new, mine)
        for name in mine:
            shape = re.search(r"kernelILi(\d)E", name)
            theirs = [n for n in meta if twin in n and (not shape or "kernelILi%sE" % shape.group(1) in n)]
            assert len(theirs) == 1, (name, theirs)
            vgpr, scratch = meta[name]
            tv = meta[theirs[0]][0]
            assert scratch == 0, (name, meta[name])
            assert vgpr <= 64 and tv <= 64 or (vgpr + 7) // 8 <= (tv + 7) // 8, (name, vgpr, tv)
            assert vgpr <= tv + 2, (name, vgpr, tv)
            seen += 1
    assert seen == 2 * 8 + 2 * 9 + 4
    scans = "knn_grid_self_count_kernel|knn_grid_self_list_kernel|knn_self_count_gated_kernel|knn_self_list_gated_kernel|" \
            "knn_count_self_outlier_kernel|knn_list_self_outlier_kernel|knn_count_self_rerank_kernel|knn_list_self_rerank_kernel"
    bodies = re.findall(r"^(_Z\w*(?:%s)\w*):(.*?)^\.Lfunc_end" % scans, text, flags=re.S | re.M)
    assert len(bodies) == seen, len(bodies)
    for name, body in bodies:
        bad = FLOAT_FMA.findall(body)
        assert not bad, (name, bad[:3])
        assert re.search(r"v_(pk_)?mul_f32", body), name
