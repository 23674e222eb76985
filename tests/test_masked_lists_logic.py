"""Lists within a radius and top-K beyond 64 over a subset of the rows (knn_index_list_within_masked,
knn_index_query_topk_large_masked; include/knn_mi355x.h 2h) without a GPU: the exported names, the argument rules of both device
calls in the header's order, the call's plan (knn_debug_masked_lists_plan) against a restatement here and against the masked count's
and the unmasked large call's own hooks, the reduction the device path rests on — a masked select is a select over the admitted
rows (knn_debug_radix_kth) — and the ISA of the three new kernel templates."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
INT_MAX = 2**31 - 1
CHUNK = 65536
vp = ctypes.c_void_p
NAMES = ("knn_index_list_within_masked", "knn_index_list_within_masked_host", "knn_index_query_topk_large_masked",
         "knn_index_query_topk_large_masked_host", "knn_debug_masked_lists_plan")


def test_the_five_names_are_declared_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"^int %s\s*\(" % name, header, flags=re.M), name
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    assert "2h. Lists within a radius and top-K beyond 64 over a subset of the rows" in header
    assert header.index("2g. Queries over a subset of the rows") < header.index("2h. Lists within a radius")
    for name in ("list_within_masked_c", "query_topk_large_masked_c", "list_within_masked_host_c", "query_topk_large_masked_host_c",
                 "debug_masked_lists_plan"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("list_within_masked", "list_within_masked_host", "query_topk_large_masked", "query_topk_large_masked_host"):
        assert callable(getattr(pkg.KnnIndex, name)), name
    # the prototypes, argument for argument
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    for proto in (
            "int knn_index_list_within_masked(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2, "
            "const unsigned *mask_dev, const unsigned long long *offsets_dev , unsigned *fill_dev , unsigned long long *keys_dev, "
            "void *stream, unsigned flags);",
            "int knn_index_list_within_masked_host(knn_index *idx, int m, const float *queries_host, float max_dist2, "
            "const unsigned *mask_host, long long *offsets_host , int **indices_out, float **dist2_out );",
            "int knn_index_query_topk_large_masked(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2, "
            "const unsigned *mask_dev, unsigned long long *keys_dev , int *indices_dev , void *stream, unsigned flags);",
            "int knn_index_query_topk_large_masked_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2, "
            "const unsigned *mask_host, int *indices_host, float *dist2_host , int *counts_host );",
            "int knn_debug_masked_lists_plan(const long long in[6], long long out[8]);"):
        assert proto in flat, proto


BAD_FLAGS = (2, 4, 8, 16, 32, 64, 1 << 31, 1 | 2)


def check_rules(rc, who, rules):
    """tests/test_masked_logic.py's scheme: every rule alone has its own text, and with every later rule broken too the earlier one
    speaks.  The index is looked at last, so the rules show with a null index: nothing behind them is reached."""
    assert rc() == (EINVAL, who + "null index") and rc(flags=0) == (EINVAL, who + "null index")
    for r2 in (0.0, -0.0, float("inf")):
        assert rc(r2=r2)[1] == who + "null index"
    for text, cases in rules:
        for kw in cases:
            assert rc(**kw) == (EINVAL, who + text), kw
    assert len({t for t, _ in rules}) == len(rules)
    for i, (text, cases) in enumerate(rules):
        kw = dict(cases[0])
        for _, later in rules[i + 1:]:
            for key, val in later[0].items():
                kw.setdefault(key, val)   # (an argument the earlier rules already broke stays as they broke it)
        assert rc(**kw) == (EINVAL, who + text), (text, kw)
    for i in range(len(rules)):      # a call that breaks rules i and j reports i
        for j in range(i + 1, len(rules)):
            kw = dict(rules[j][1][0])
            kw.update(rules[i][1][0])
            if all(kw[key] == val for key, val in rules[j][1][0].items()):
                assert rc(**kw) == (EINVAL, who + rules[i][0]), (i, j, kw)


def test_the_list_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    q, w, o, f, k = vp(0x1000), vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000)

    def rc(slot=0, m=7, queries=q, r2=1.0, mask=w, offsets=o, fill=f, keys=k, flags=1):
        return (pkg.list_within_masked_c()(None, slot, m, queries, r2, mask, offsets, fill, keys, None, flags),
                L.knn_last_error().decode())

    rules = [
        ("max_dist2 must be >= 0 and not NaN", [dict(r2=-1.0), dict(r2=float("nan")), dict(r2=-float("inf"))]),
        ("unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)", [dict(flags=fl) for fl in BAD_FLAGS]),
        ("slot outside 0 .. 7", [dict(slot=8), dict(slot=-1)]),
        ("m < 1", [dict(m=0), dict(m=-3)]),
        ("null queries", [dict(queries=None)]),
        ("null mask", [dict(mask=None)]),
        ("null offsets, fill or keys", [dict(offsets=None), dict(fill=None), dict(keys=None)]),
    ]
    check_rules(rc, "knn_index_list_within_masked: ", rules)
    assert len(rules) == 7


def test_the_large_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    L = pkg.lib()
    q, w, k = vp(0x1000), vp(0x2000), vp(0x3000)

    def rc(slot=0, m=7, K=100, queries=q, r2=1.0, mask=w, keys=k, flags=1):
        return (pkg.query_topk_large_masked_c()(None, slot, m, K, queries, r2, mask, keys, None, None, flags),
                L.knn_last_error().decode())

    who = "knn_index_query_topk_large_masked: "
    rules = [
        ("max_dist2 must be >= 0 and not NaN", [dict(r2=-1.0), dict(r2=float("nan")), dict(r2=-float("inf"))]),
        ("unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)", [dict(flags=fl) for fl in BAD_FLAGS]),
        ("slot outside 0 .. 7", [dict(slot=8), dict(slot=-1)]),
        ("m < 1", [dict(m=0), dict(m=-3)]),
        ("K outside 1 .. 4096", [dict(K=0), dict(K=4097), dict(K=-1)]),
        ("m * K above INT_MAX", [dict(m=INT_MAX // 4096 + 1, K=4096)]),
        ("null queries", [dict(queries=None)]),
        ("null mask", [dict(mask=None)]),
        ("null keys", [dict(keys=None)]),
    ]
    check_rules(rc, who, rules)
    assert len(rules) == 9
    for K in (1, 64, 65, 4096):
        assert rc(K=K)[1] == who + "null index"
    assert rc(m=INT_MAX // 4096, K=4096)[1] == who + "null index"


def test_the_host_calls_argument_errors_need_no_gpu():
    L = pkg.lib()
    Q = np.zeros((4, 3), dtype=np.float32)
    ind = np.zeros((4, 100), dtype=np.int32)
    words = np.zeros(4, dtype=np.uint32)

    def host(m=4, K=100, queries=Q.ctypes.data, r2=1.0, mask=words.ctypes.data, out=ind.ctypes.data):
        return (pkg.query_topk_large_masked_host_c()(None, m, K, vp(queries) if queries else None, r2, vp(mask) if mask else None,
                                                     vp(out) if out else None, None, None), L.knn_last_error().decode())

    who = "knn_index_query_topk_large_masked_host: "
    assert host() == (EINVAL, who + "null index")
    for bad in (-1.0, float("nan")):
        assert host(r2=bad) == (EINVAL, who + "max_dist2 must be >= 0 and not NaN")
    assert host(m=0) == (EINVAL, who + "m < 1")
    assert host(K=0) == (EINVAL, who + "K outside 1 .. 4096") and host(K=4097) == (EINVAL, who + "K outside 1 .. 4096")
    assert host(m=INT_MAX // 4096 + 1, K=4096) == (EINVAL, who + "m * K above INT_MAX")
    for kw in (dict(queries=None), dict(mask=None), dict(out=None)):
        assert host(**kw) == (EINVAL, who + "null queries, mask or indices")

    offs = np.zeros(5, dtype=np.int64)
    pi, pd = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()

    def lists(m=4, queries=Q.ctypes.data, r2=1.0, mask=words.ctypes.data, offsets=offs.ctypes.data):
        return (pkg.list_within_masked_host_c()(None, m, vp(queries) if queries else None, r2, vp(mask) if mask else None,
                                                vp(offsets) if offsets else None, ctypes.byref(pi), ctypes.byref(pd)),
                L.knn_last_error().decode())

    for kw in (dict(), dict(m=0), dict(queries=None), dict(mask=None), dict(offsets=None), dict(r2=-1.0), dict(r2=float("nan"))):
        rc, text = lists(**kw)
        assert rc == EINVAL and text.startswith("knn_index_list_within_masked_host: bad arguments"), kw


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def divup(a, b):
    return -(-a // b)


def count_slices(mc, n, cu):
    """Slices of the exact count scan for one chunk of mc queries (knn_exact.hip): about 32 waves per CU, at least 1024 rows each,
    at most 65535; then evened out."""
    s = max(min(cu * 32 // divup(mc, 64), divup(n, 1024), 65535), 1)
    return divup(n, divup(n, s))


def select_slices(mc, n, cu):
    """Slices of one select pass (knn_select.hip): four 8-wave blocks per CU, at least 128 rows per wave, at most 65535; evened."""
    s = max(min(cu * 4 // divup(mc, 64), divup(n, 128 * 8), 65535), 1)
    return divup(n, divup(n, s))


def align256(v):
    return (v + 255) // 256 * 256


def select_scratch(mc, K, init):
    mcp = divup(mc, 64) * 64
    prefix = align256(256 * mcp * 4)
    need = align256(prefix + mcp * 8)
    cursor = align256(need + mcp * 4)
    gate = align256(cursor + mcp * 4)
    state = align256(gate + 9 * 4)
    return state + (0 if init else mc * K * 8)


def restated_plan(k, m, K, rows, cu, init):
    mc, chunks = min(m, CHUNK), divup(m, CHUNK)
    if rows == 0:
        return dict(granules=0, slices=0, slice_waves=0, chunks=chunks, lds_bytes=0, mask_bytes=0, select_bytes=0,
                    launches=1 if K > 0 and init else 0)
    G = divup(rows, 1024)
    mask_bytes = (G + 1) * 8 + (G * 4 + 7) // 8 * 8
    if K == 0:
        return dict(granules=G, slices=count_slices(mc, rows, cu), slice_waves=1, chunks=chunks, lds_bytes=0, mask_bytes=mask_bytes,
                    select_bytes=0, launches=2 + chunks)
    # per chunk: the state's memset, a scan and a pick per distance pass, the fill, the sort, a fold's merge
    per_chunk = 1 + 2 * 4 + 1 + 1 + (0 if init else 1)
    return dict(granules=G, slices=select_slices(mc, rows, cu), slice_waves=8, chunks=chunks, lds_bytes=256 * 64 * 4,
                mask_bytes=mask_bytes, select_bytes=select_scratch(mc, K, init), launches=2 + chunks * per_chunk)


def test_the_plan_against_its_restatement_the_masked_count_and_the_large_call():
    cu = 256
    for k in (1, 16, 17, 128, 129):
        for m in (1, 64, 65, 65536, 65537):
            for K in (0, 1, 64, 65, 100, 4096):
                for rows in (0, 1, 1023, 1024, 1025, 3149, 1 << 20):
                    for init in (0, 1):
                        if m * K > INT_MAX:
                            continue
                        got = pkg.debug_masked_lists_plan(k=k, m=m, K=K, rows=rows, num_cu=cu, init=init)
                        assert got == restated_plan(k, m, K, rows, cu, init), (k, m, K, rows, init)
                        if K == 0:   # a list call cuts the shard as the masked count does
                            cnt = pkg.debug_masked_plan(k=k, m=m, K=0, rows=rows, num_cu=cu, init=init)
                            assert (got["granules"], got["slices"], got["chunks"], got["mask_bytes"]) == \
                                   (cnt["granules"], cnt["slices"], cnt["chunks"], cnt["mask_bytes"]), (k, m, rows)
                            assert got["select_bytes"] == 0 and got["lds_bytes"] == 0
                            assert got["launches"] == cnt["launches"]
                        elif rows > 0:   # the select's state and a fold's lists are the unmasked large call's
                            big = pkg.debug_topk_large_plan(k=k, m=m, K=K, rows=rows, num_cu=cu, init=init)
                            assert got["select_bytes"] == big["scratch_bytes"] and got["slices"] == big["slices"]
                            assert got["lds_bytes"] == big["lds_bytes"] and got["chunks"] == big["chunks"]
                            assert got["launches"] == 2 + big["launches_clean"]
                            # every wave of every block has its own slice number below 2^20: the cut's products stay in 64 bits
                            assert got["slices"] * got["slice_waves"] < 1 << 20
    # an empty shard launches nothing but an init large call's fill
    for K, init, launches in ((100, 1, 1), (100, 0, 0), (0, 1, 0), (0, 0, 0)):
        p = pkg.debug_masked_lists_plan(k=3, m=70, K=K, rows=0, num_cu=cu, init=init)
        assert p["launches"] == launches and p["granules"] == p["slices"] == p["mask_bytes"] == p["select_bytes"] == 0
    L = pkg.lib()
    for kw in (dict(k=0), dict(m=0), dict(K=-1), dict(K=4097), dict(m=INT_MAX // 4096 + 1, K=4096), dict(rows=-1),
               dict(rows=(1 << 32) + 1), dict(num_cu=0), dict(init=2)):
        args = dict(k=3, m=70, K=100, rows=5000, num_cu=cu, init=1)
        args.update(kw)
        with pytest.raises(pkg.KnnError):
            pkg.debug_masked_lists_plan(**args)
        assert L.knn_last_error().decode().startswith("knn_debug_masked_lists_plan")


# ---- the select under a mask ----------------------------------------------------------------------------------------------------
def test_a_masked_select_is_a_select_over_the_admitted_rows():
    """The device path counts only admitted candidates into the histograms and hands them to the unmasked pick: so the threshold
    must be the one the pick finds over the admitted keys alone — exactly K admitted keys are <= T, whatever the excluded rows
    hold, also when the cut falls inside a class of equal distances (then the index word's passes run)."""
    rng = np.random.default_rng(4242)
    n = 5000
    dist = rng.integers(0, 40, size=n).astype(np.float32) * np.float32(0.25)    # ~125 rows per distance class
    keys = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    for density in (1.0, 0.5, 1 / 16):
        admit = rng.random(n) < density
        adm = keys[admit]
        order = np.sort(adm)
        for K in (1, 8, 64, 100, 256, 4096):
            T, passes = pkg.debug_radix_kth(adm, K)
            want = min(K, adm.size)
            assert int((adm <= np.uint64(T)).sum()) == want, (density, K)
            if K <= adm.size:
                # the cut inside a class <=> the K-th and the (K + 1)-th admitted key share a distance, or the class ends elsewhere
                assert order[K - 1] <= np.uint64(T) and (K == adm.size or order[K] > np.uint64(T))
                cls = order[(order >> np.uint64(32)) == (order[K - 1] >> np.uint64(32))]
                inside = cls[-1] != order[K - 1]
                assert (passes > 4) == bool(inside), (density, K, passes)
            # excluded rows nearer than every admitted one change nothing: they are never counted
            assert pkg.debug_radix_kth(adm, K)[0] == T
            # ... while a select that ignored the mask would admit excluded rows
            if density < 1.0 and K <= adm.size:
                T_all, _ = pkg.debug_radix_kth(keys, K)
                assert T_all <= T
    # a class of K + 5 copies of which the mask admits part: the cut is inside the class among the ADMITTED keys only
    K = 100
    block = (np.uint64(np.float32(1.0).view(np.uint32)) << np.uint64(32)) | np.arange(1000, 1000 + K + 5, dtype=np.uint64)
    near = (np.uint64(np.float32(0.5).view(np.uint32)) << np.uint64(32)) | np.arange(10, dtype=np.uint64)
    T, passes = pkg.debug_radix_kth(np.concatenate([near, block]), K)            # 10 nearer + 105 copies: cut inside the class
    assert passes > 4 and T == int(block[K - 10 - 1])
    T, passes = pkg.debug_radix_kth(np.concatenate([near, block[:K - 10 - 3]]), K)   # fewer copies than places: no cut inside
    assert passes <= 4 and int((np.concatenate([near, block[:K - 10 - 3]]) <= np.uint64(T)).sum()) == K - 3


# ---- the kernels' ISA -----------------------------------------------------------------------------------------------------------
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLOAT_FMA = re.compile(r"\bv_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_f32|\bv_dot\d")   # tests/test_host_logic.py's pattern
NEW_KERNELS = r"knn_masked_(?:list|hist|fill)_kernel"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_the_new_kernels_hold_no_fused_multiply_add_and_use_no_scratch(tmp_path):
    """Bit-exactness against v0 needs one rounding per operation; a kernel that keeps its query in registers must not spill; and no
    new kernel carries a name the masked top-K / count pin (tests/test_masked_logic.py) would match."""
    src = os.path.join(ROOT, "multicore_hw2_amd", "csrc", "knn_masked_lists.hip")
    asm = tmp_path / "knn_masked_lists.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                           "-o", str(asm), src])
    text = asm.read_text()
    bodies = re.findall(r"^(_Z\w*%s\w*):(.*?)^\.Lfunc_end" % NEW_KERNELS, text, flags=re.S | re.M)
    assert len(bodies) >= 27, len(bodies)
    for name, body in bodies:
        bad = FLOAT_FMA.findall(body)
        assert not bad, (name, bad[:3])
        assert re.search(r"v_mul_f32", body), name
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        name, meta = m.group(1), m.group(2)
        assert not re.search(r"knn_masked_(topk|count)_kernelILi[1-8]E", name), name
        form = re.search(NEW_KERNELS + r"ILi(\d)E", name)
        if not form or form.group(1) == "0":
            continue
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        assert scratch == 0, (name, scratch)
        seen += 1
    assert seen == 24, seen
