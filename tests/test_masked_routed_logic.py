"""Counts and lists within a radius over a subset of the rows on the grid and cell-pruned ways
(knn_index_count_within_masked_routed, knn_index_list_within_masked_routed; include/knn_mi355x.h 2l) without a GPU: the exported
names and prototypes, the argument rules of the two calls in the header's order on a null index, the three flags they admit, and
that the existing masked calls still refuse the routing flags."""
import ctypes
import os
import re

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
INF = float("inf")
NAN = float("nan")
vp = ctypes.c_void_p
NAMES = ("knn_index_count_within_masked_routed", "knn_index_list_within_masked_routed")
INIT, PARTIAL, GRID, FRAMES, COUNT_GRID, COUNT_CELLS = 1, 2, 4, 8, 16, 32
FLAGS_TEXT = "unknown flag (KNN_QUERY_INIT_KEYS, KNN_QUERY_COUNT_GRID, KNN_QUERY_COUNT_CELLS)"
RADIUS_TEXT = "max_dist2 must be >= 0 and not NaN"


def test_the_two_names_are_declared_under_2l_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    at = header.index("2l. Counts and lists within a radius over a subset of the rows, on the grid and cell-pruned ways")
    assert at > header.index("2k. The radius graph on the grid and cell-pruned ways")
    for name in NAMES:
        m = re.search(r"^int %s\s*\(" % name, header, flags=re.M)
        assert m and m.start() > at, name
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    for name in ("count_within_masked_routed_c", "list_within_masked_routed_c"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("count_within_masked_routed", "list_within_masked_routed"):
        assert callable(getattr(pkg.KnnIndex, name)), name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for proto in (
            "int knn_index_count_within_masked_routed(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2, "
            "const unsigned *mask_dev, unsigned *counts_dev, void *stream, unsigned flags);",
            "int knn_index_list_within_masked_routed(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2, "
            "const unsigned *mask_dev, const unsigned long long *offsets_dev , unsigned *fill_dev , unsigned long long *keys_dev, "
            "void *stream, unsigned flags);"):
        assert proto in flat, proto
    # the gaps the section states
    section = re.sub(r"\s+", " ", re.sub(r"\n \* ?", "\n", header[at:header.index("*/", at)]))
    for gap in ("a radius per query under a mask", "masked self calls", "the masked top-K on the pruned ways", "a default policy",
                "using the mask to skip whole cells"):
        assert gap in section, gap


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


def _radius_and_flag_rules(who, rc):
    assert rc(r2=NAN)[1] == who + RADIUS_TEXT and rc(r2=-1e-30)[1] == who + RADIUS_TEXT
    for r2 in (-0.0, 0.0, 1.0, INF):          # -0 and +INF pass the first rule: the index speaks
        assert rc(r2=r2) == (EINVAL, who + "null index"), r2
    for flags in (PARTIAL, GRID, FRAMES, 64, 1 << 31, INIT | PARTIAL, COUNT_CELLS | FRAMES):
        assert rc(flags=flags) == (EINVAL, who + FLAGS_TEXT), flags
    for flags in (0, INIT, COUNT_GRID, COUNT_CELLS, COUNT_GRID | COUNT_CELLS | INIT):
        assert rc(flags=flags) == (EINVAL, who + "null index"), flags


def test_the_count_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    q, w, c = vp(0x1000), vp(0x2000), vp(0x3000)

    def rc(slot=0, m=7, queries=q, r2=1.0, mask=w, counts=c, flags=INIT):
        return (pkg.count_within_masked_routed_c()(None, slot, m, queries, r2, mask, counts, None, flags), L.knn_last_error().decode())

    who = "knn_index_count_within_masked_routed: "
    _walk(who, rc, [
        (dict(r2=-0.5), RADIUS_TEXT),
        (dict(flags=GRID), FLAGS_TEXT),
        (dict(slot=8), "slot outside 0 .. 7"),
        (dict(m=0), "m < 1"),
        (dict(queries=None), "null queries"),
        (dict(mask=None), "null mask"),
        (dict(counts=None), "null counts"),
    ])
    _radius_and_flag_rules(who, rc)
    assert rc(slot=-1)[1] == who + "slot outside 0 .. 7" and rc(m=-3)[1] == who + "m < 1"
    assert rc(queries=None, counts=None)[1] == who + "null queries" and rc(mask=None, counts=None)[1] == who + "null mask"


def test_the_list_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    q, w, o, f, k = vp(0x1000), vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000)

    def rc(slot=0, m=7, queries=q, r2=1.0, mask=w, offsets=o, fill=f, keys=k, flags=INIT):
        return (pkg.list_within_masked_routed_c()(None, slot, m, queries, r2, mask, offsets, fill, keys, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_list_within_masked_routed: "
    _walk(who, rc, [
        (dict(r2=NAN), RADIUS_TEXT),
        (dict(flags=FRAMES), FLAGS_TEXT),
        (dict(slot=-2), "slot outside 0 .. 7"),
        (dict(m=-1), "m < 1"),
        (dict(queries=None), "null queries"),
        (dict(mask=None), "null mask"),
        (dict(keys=None), "null offsets, fill or keys"),
    ])
    _radius_and_flag_rules(who, rc)
    assert rc(offsets=None)[1] == who + "null offsets, fill or keys" and rc(fill=None)[1] == who + "null offsets, fill or keys"
    assert rc(mask=None, fill=None)[1] == who + "null mask"


def test_the_existing_masked_calls_still_refuse_the_routing_flags():
    L = pkg.lib()
    q, w, c, o, f, k = vp(0x1000), vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000), vp(0x6000)
    text = "unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)"
    count = L.knn_index_count_within_masked
    count.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_float, vp, vp, vp, ctypes.c_uint]
    for flags in (COUNT_CELLS, COUNT_GRID, COUNT_CELLS | INIT):
        assert count(None, 0, 7, q, 1.0, w, c, None, flags) == EINVAL
        assert L.knn_last_error().decode() == "knn_index_count_within_masked: " + text, flags
        assert pkg.list_within_masked_c()(None, 0, 7, q, 1.0, w, o, f, k, None, flags) == EINVAL
        assert L.knn_last_error().decode() == "knn_index_list_within_masked: " + text, flags
    assert count(None, 0, 7, q, 1.0, w, c, None, INIT) == EINVAL
    assert L.knn_last_error().decode() == "knn_index_count_within_masked: null index"
