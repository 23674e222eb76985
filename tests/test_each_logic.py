"""A radius per query (knn_index_count_within_each, knn_index_list_within_each, their self forms, knn_keys_column_dist2;
include/knn_mi355x.h 2j) without a GPU: the exported names, the argument rules of the four device calls in the header's order, the
radius of one query (knn_debug_each_radius, the kernels' own lines in csrc/knn_each_radius.h), and what the compiler made of the
new kernels."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EINVAL = -1
INF = float("inf")
NAN = float("nan")
vp = ctypes.c_void_p
NAMES = ("knn_index_count_within_each", "knn_index_list_within_each", "knn_index_self_count_within_each",
         "knn_index_self_list_within_each", "knn_keys_column_dist2", "knn_index_count_within_each_host",
         "knn_index_list_within_each_host", "knn_debug_each_radius")
INIT, PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS = 1, 2, 4, 8, 16, 32


def test_the_eight_names_are_declared_under_2j_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    at = header.index("2j. A radius per query")
    assert at > header.index("2i. Queries about the shard's own rows")
    for name in NAMES:
        m = re.search(r"^int %s\s*\(" % name, header, flags=re.M)
        assert m and m.start() > at, name
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    for name in ("count_within_each_c", "list_within_each_c", "self_count_within_each_c", "self_list_within_each_c",
                 "count_within_each_host_c", "list_within_each_host_c", "keys_column_dist2_c", "keys_column_dist2",
                 "debug_each_radius"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("count_within_each", "list_within_each", "self_count_within_each", "self_list_within_each",
                 "count_within_each_host", "list_within_each_host"):
        assert callable(getattr(pkg.KnnIndex, name)), name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for proto in (
            "int knn_index_count_within_each(knn_index *idx, int slot, int m, const float *queries_dev, const float *max_dist2_dev, "
            "float cap, unsigned *counts_dev, void *stream, unsigned flags);",
            "int knn_index_list_within_each(knn_index *idx, int slot, int m, const float *queries_dev, const float *max_dist2_dev, "
            "float cap, const unsigned long long *offsets_dev , unsigned *fill_dev , unsigned long long *keys_dev, void *stream, "
            "unsigned flags);",
            "int knn_index_self_count_within_each(knn_index *idx, int slot, long long row_first, int rows, "
            "const float *max_dist2_dev , float cap, unsigned *counts_dev , void *stream, unsigned flags);",
            "int knn_index_self_list_within_each(knn_index *idx, int slot, long long row_first, int rows, "
            "const float *max_dist2_dev , float cap, const unsigned long long *offsets_dev , unsigned *fill_dev , "
            "unsigned long long *keys_dev, void *stream, unsigned flags);",
            "int knn_keys_column_dist2(int device, const unsigned long long *keys_dev, int m, int K, int column, float *dist2_dev, "
            "void *stream);",
            "int knn_index_count_within_each_host(knn_index *idx, int m, const float *queries_host, const float *max_dist2_host, "
            "float cap, unsigned *counts_host);",
            "int knn_index_list_within_each_host(knn_index *idx, int m, const float *queries_host, const float *max_dist2_host, "
            "float cap, long long *offsets_host, int **indices_out, float **dist2_out );",
            "int knn_debug_each_radius(float radius, float cap, float out[2]);"):
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


COUNT_FLAGS_TEXT = "unknown flag (KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS)"
SELF_FLAGS_TEXT = "unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)"
CAP_TEXT = "cap must be >= 0 (or +INF) and not NaN"


def _cap_rule(who, rc):
    assert rc(cap=NAN)[1] == who + CAP_TEXT and rc(cap=-1e-30)[1] == who + CAP_TEXT
    for cap in (-0.0, 0.0, 1.0, INF):         # -0 and +INF pass the first rule: the index speaks
        assert rc(cap=cap) == (EINVAL, who + "null index"), cap


def test_the_count_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    q, r, c = vp(0x1000), vp(0x2000), vp(0x3000)

    def rc(slot=0, m=7, queries=q, radii=r, cap=1.0, counts=c, flags=INIT):
        return pkg.count_within_each_c()(None, slot, m, queries, radii, cap, counts, None, flags), L.knn_last_error().decode()

    who = "knn_index_count_within_each: "
    _walk(who, rc, [
        (dict(cap=-1.0), CAP_TEXT),
        (dict(flags=GRID), COUNT_FLAGS_TEXT),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(m=0), "m < 1"),
        (dict(queries=None), "null queries"),
        (dict(radii=None), "null radii"),
        (dict(counts=None), "null counts"),
    ])
    _cap_rule(who, rc)
    assert rc(queries=None, radii=None)[1] == who + "null queries"      # the radii speak after the queries
    for flags in (PARTIAL, GRID, FRAMES, 64, 1 << 31, INIT | PARTIAL):
        assert rc(flags=flags)[1] == who + COUNT_FLAGS_TEXT, flags
    for flags in (0, INIT, COUNT_GRID, COUNT_CELLS, INIT | COUNT_GRID | COUNT_CELLS):
        assert rc(flags=flags) == (EINVAL, who + "null index"), flags
    assert rc(slot=-1)[1] == who + "slot outside 0 .. 7" and rc(m=-3)[1] == who + "m < 1"


def test_the_list_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    q, r, o, f, k = vp(0x1000), vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000)

    def rc(slot=0, m=7, queries=q, radii=r, cap=1.0, offsets=o, fill=f, keys=k, flags=INIT):
        return (pkg.list_within_each_c()(None, slot, m, queries, radii, cap, offsets, fill, keys, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_list_within_each: "
    _walk(who, rc, [
        (dict(cap=NAN), CAP_TEXT),
        (dict(flags=FRAMES), COUNT_FLAGS_TEXT),
        (dict(slot=-1), "slot outside 0 .. 7"),
        (dict(m=-1), "m < 1"),
        (dict(queries=None), "null queries"),
        (dict(radii=None), "null radii"),
        (dict(offsets=None), "null offsets, fill or keys"),
    ])
    _cap_rule(who, rc)
    assert rc(queries=None, radii=None)[1] == who + "null queries"
    assert rc(fill=None)[1] == who + "null offsets, fill or keys" and rc(keys=None)[1] == who + "null offsets, fill or keys"
    for flags in (PARTIAL, GRID, FRAMES, 64, 1 << 31):
        assert rc(flags=flags)[1] == who + COUNT_FLAGS_TEXT, flags
    for flags in (0, INIT, COUNT_GRID, COUNT_CELLS, INIT | COUNT_GRID | COUNT_CELLS):
        assert rc(flags=flags) == (EINVAL, who + "null index"), flags


def test_the_self_count_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    r, c = vp(0x2000), vp(0x3000)

    def rc(slot=0, row_first=0, rows=7, radii=r, cap=1.0, counts=c, flags=INIT):
        return (pkg.self_count_within_each_c()(None, slot, row_first, rows, radii, cap, counts, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_self_count_within_each: "
    _walk(who, rc, [
        (dict(cap=-0.5), CAP_TEXT),
        (dict(flags=COUNT_GRID), SELF_FLAGS_TEXT),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(rows=0), "rows < 1"),
        (dict(row_first=-1), "row_first < 0"),
        (dict(radii=None), "null radii"),
        (dict(counts=None), "null counts"),
    ])
    _cap_rule(who, rc)
    assert rc(rows=0, row_first=-1)[1] == who + "rows < 1"
    for flags in (PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS, 64, 1 << 31, INIT | COUNT_CELLS):   # every flag but the init flag
        assert rc(flags=flags)[1] == who + SELF_FLAGS_TEXT, flags
    assert rc(flags=0) == (EINVAL, who + "null index")


def test_the_self_list_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    r, o, f, k = vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000)

    def rc(slot=0, row_first=0, rows=7, radii=r, cap=1.0, offsets=o, fill=f, keys=k, flags=INIT):
        return (pkg.self_list_within_each_c()(None, slot, row_first, rows, radii, cap, offsets, fill, keys, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_self_list_within_each: "
    _walk(who, rc, [
        (dict(cap=NAN), CAP_TEXT),
        (dict(flags=COUNT_CELLS), SELF_FLAGS_TEXT),
        (dict(slot=-2), "slot outside 0 .. 7"),
        (dict(rows=-1), "rows < 1"),
        (dict(row_first=-7), "row_first < 0"),
        (dict(radii=None), "null radii"),
        (dict(keys=None), "null offsets, fill or keys"),
    ])
    _cap_rule(who, rc)
    assert rc(offsets=None)[1] == who + "null offsets, fill or keys" and rc(fill=None)[1] == who + "null offsets, fill or keys"
    for flags in (PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS, 64, 1 << 31, INIT | COUNT_GRID):
        assert rc(flags=flags)[1] == who + SELF_FLAGS_TEXT, flags
    assert rc(flags=0) == (EINVAL, who + "null index")


def test_the_column_call_and_the_host_calls_reject_their_bad_arguments_without_a_gpu():
    L = pkg.lib()
    p = vp(0x1000)
    f = pkg.keys_column_dist2_c()
    who = "knn_keys_column_dist2: "
    for args, text in (((0, p, 0, 8, 7, p, None), "m < 1"), ((0, p, 5, 0, 0, p, None), "K < 1 or column outside 0 .. K - 1"),
                       ((0, p, 5, 8, 8, p, None), "K < 1 or column outside 0 .. K - 1"),
                       ((0, p, 5, 8, -1, p, None), "K < 1 or column outside 0 .. K - 1"),
                       ((0, None, 5, 8, 7, p, None), "null keys or dist2"), ((0, p, 5, 8, 7, None, None), "null keys or dist2")):
        assert f(*args) == EINVAL and L.knn_last_error().decode() == who + text, args
    ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
    ch, lh = pkg.count_within_each_host_c(), pkg.list_within_each_host_c()
    for cap in (1.0, -1.0, NAN, INF):          # (no index: every one of them fails before anything is touched)
        assert ch(None, 3, p, p, cap, p) == EINVAL
        assert L.knn_last_error().decode().startswith("knn_index_count_within_each_host: bad arguments")
        assert lh(None, 3, p, p, cap, p, ctypes.byref(ind), ctypes.byref(d2)) == EINVAL
        assert L.knn_last_error().decode().startswith("knn_index_list_within_each_host: bad arguments")


F32 = np.float32
SUBNORMAL = float(np.nextafter(F32(0), F32(1)))
RADII = (NAN, -1.0, -0.0, 0.0, SUBNORMAL, 1.0, INF)
CAPS = (0.0, 1.0, INF)


@pytest.mark.parametrize("cap", CAPS)
def test_the_radius_of_one_query_through_the_kernels_own_lines(cap):
    """knn_each_radius.h: candidates iff radius >= 0 (NaN fails); the bound is the radius when radius <= cap, else cap."""
    for radius in RADII:
        has, bound = pkg.debug_each_radius(radius, cap)
        if math.isnan(radius) or radius < 0.0:
            assert not has, (radius, cap)
            continue
        assert has, (radius, cap)
        want = radius if radius <= cap else cap
        assert bound == want and not math.isnan(bound), (radius, cap, bound)
        # every distance E >= 0 is within the radius and the cap exactly when it is within the bound
        for e in (0.0, SUBNORMAL, 0.5, 1.0, float(np.nextafter(F32(1), F32(2))), 3e38):
            assert (e <= radius and e <= cap) == (e <= bound), (radius, cap, e)
    has, bound = pkg.debug_each_radius(-0.0, cap)
    assert has and bound == 0.0                # -0 is a candidate with bound 0
    out = (ctypes.c_float * 2)()
    f = pkg.lib().knn_debug_each_radius
    f.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_float)]
    assert f(1.0, -1.0, out) == EINVAL and f(1.0, NAN, out) == EINVAL and f(1.0, 1.0, None) == EINVAL


# ---- what the compiler made of the new kernels ---------------------------------------------------------------------------

FLOAT_FMA = re.compile(r"\bv_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_f32|\bv_dot\d")
V0_KERNELS = r"knn_exact_count_each_kernel|knn_exact_list_each_kernel|knn_grid_each_count_kernel|knn_grid_each_list_kernel|" \
             r"knn_self_count_each_kernel|knn_self_list_each_kernel"
OTHER_KERNELS = r"knn_count_each_rerank_kernel|knn_count_each_outlier_kernel|knn_list_each_rerank_kernel|" \
                r"knn_list_each_outlier_kernel|knn_keys_column_dist2_kernel|knn_cells_prep_each_kernel"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_the_new_kernels_use_no_scratch_and_their_scans_hold_no_fused_multiply_add(tmp_path):
    names = ("knn_exact", "knn_grid", "knn_cells", "knn_self", "knn_each")
    procs = []
    for name in names:     # (tests/test_within_logic.py::_metadata's command)
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
    new = [n for n in meta if re.search(V0_KERNELS + "|" + OTHER_KERNELS, n)]
    # 9 forms (KC 0 .. 8) of each exact and self scan, 4 (k 1 .. 4) of each grid walk, 4 (PW x KT) of the prep form, 5 single kernels
    assert len(new) == 4 * 9 + 2 * 4 + 4 + 5, sorted(new)
    for name in new:
        assert meta[name][1] == 0, (name, meta[name])
    bodies = re.findall(r"^(_Z\w*(?:%s)\w*):(.*?)^\.Lfunc_end" % V0_KERNELS, text, flags=re.S | re.M)
    assert len(bodies) == 4 * 9 + 2 * 4, len(bodies)
    for name, body in bodies:
        bad = FLOAT_FMA.findall(body)
        assert not bad, (name, bad[:3])
        assert re.search(r"v_mul_f32", body), name
    # the preparation form beside the scalar count form of the same shape: reported, not gated
    for name in sorted(n for n in meta if "knn_cells_prep_each_kernel" in n):
        shape = re.search(r"each_kernelILi(\d)ELi(\d)ELi(\d)E", name).groups()
        twin = [n for n in meta if re.search(r"knn_cells_prep_count_kernelILi%sELi%sELi%sE" % shape, n)]
        assert len(twin) == 1, (name, twin)
        print("prep form PW %s SD %s KT %s: %d VGPRs with a radius per query, %d scalar" % (shape + (meta[name][0], meta[twin[0]][0])))
