"""Queries over a subset of the rows (knn_index_query_topk_masked, knn_index_count_within_masked; include/knn_mi355x.h 2g) without a
GPU: the exported names, the argument rules of the entry points in the header's order, the call's plan (knn_debug_masked_plan)
against a restatement here and against the unmasked scans' own hooks, the cut by admitted rows (knn_debug_mask_split and
knn_debug_mask_split_rows, the kernels' own lines in csrc/knn_mask_split.h) against brute-force restatements, and the ISA of the
masked scan kernels."""
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
NAMES = ("knn_index_query_topk_masked", "knn_index_count_within_masked", "knn_mask_set_rows", "knn_index_query_topk_masked_host",
         "knn_debug_masked_plan", "knn_debug_mask_split", "knn_debug_mask_split_rows")


def test_the_new_names_are_declared_exported_and_mirrored():
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"^int %s\s*\(" % name, header, flags=re.M), name
        assert name in pkg.EXPORTED_SYMBOLS
        assert hasattr(pkg.lib(), name)
    assert "2g. Queries over a subset of the rows" in header
    for name in ("mask_words", "mask_set_rows", "debug_masked_plan", "debug_mask_split", "debug_mask_split_rows"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("query_topk_masked", "count_within_masked", "query_topk_masked_host"):
        assert callable(getattr(pkg.KnnIndex, name)), name
    assert [pkg.mask_words(n) for n in (0, 1, 31, 32, 33, 1024, 1025)] == [0, 1, 1, 1, 2, 32, 33]
    # the prototypes, argument for argument
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    for proto in (
            "int knn_index_query_topk_masked(knn_index *idx, int slot, int m, int K, const float *queries_dev, float max_dist2, "
            "const unsigned *mask_dev, unsigned long long *keys_dev , int *indices_dev , void *stream, unsigned flags);",
            "int knn_index_count_within_masked(knn_index *idx, int slot, int m, const float *queries_dev, float max_dist2, "
            "const unsigned *mask_dev, unsigned *counts_dev, void *stream, unsigned flags);",
            "int knn_mask_set_rows(int device, long long n_local, const unsigned *rows_dev, long long count, int value, "
            "unsigned *mask_dev, void *stream);",
            "int knn_index_query_topk_masked_host(knn_index *idx, int m, int K, const float *queries_host, float max_dist2, "
            "const unsigned *mask_host, int *indices_host, float *dist2_host, int *counts_host);",
            "int knn_debug_masked_plan(const long long in[6], long long out[8]);",
            "int knn_debug_mask_split(const unsigned *granule_counts, long long granules, int slices, long long *first_granule );",
            "int knn_debug_mask_split_rows(const unsigned *mask_host, long long n_local, int slices, long long *first_row );"):
        assert proto in flat, proto


BAD_FLAGS = (2, 4, 8, 16, 32, 64, 1 << 31, 1 | 2)


def test_the_top_k_call_argument_errors_speak_in_the_headers_order_without_a_gpu():
    """Every rule has its own text and the index is looked at last, so the rules show with a null index: nothing behind them is
    reached (the pointers here are never read)."""
    L = pkg.lib()
    q, w, k = vp(0x1000), vp(0x2000), vp(0x3000)

    def rc(slot=0, m=7, K=8, queries=q, r2=1.0, mask=w, keys=k, flags=1):
        return pkg.query_topk_masked_c()(None, slot, m, K, queries, r2, mask, keys, None, None, flags), L.knn_last_error().decode()

    who = "knn_index_query_topk_masked: "
    assert rc() == (EINVAL, who + "null index") and rc(flags=0) == (EINVAL, who + "null index")
    for r2 in (0.0, -0.0, float("inf")):
        assert rc(r2=r2)[1] == who + "null index"
    for K in (1, 64):
        assert rc(K=K)[1] == who + "null index"
    # each rule alone
    rules = [
        ("max_dist2 must be >= 0 and not NaN", [dict(r2=-1.0), dict(r2=float("nan")), dict(r2=-float("inf"))]),
        ("unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)", [dict(flags=f) for f in BAD_FLAGS]),
        ("slot outside 0 .. 7", [dict(slot=8), dict(slot=-1)]),
        ("m < 1", [dict(m=0), dict(m=-3)]),
        ("K outside 1 .. 64", [dict(K=0), dict(K=65), dict(K=-1), dict(K=4096)]),
        ("m * K above INT_MAX", [dict(m=INT_MAX // 64 + 1, K=64)]),
        ("null queries, mask or keys", [dict(queries=None), dict(mask=None), dict(keys=None)]),
    ]
    for text, cases in rules:
        for kw in cases:
            assert rc(**kw) == (EINVAL, who + text), kw
    assert rc(m=INT_MAX // 64, K=64)[1] == who + "null index"
    assert len({t for t, _ in rules}) == 7
    # the order: with every later rule broken too, the earlier one speaks
    for i, (text, cases) in enumerate(rules):
        kw = dict(cases[0])
        for _, later in rules[i + 1:]:
            for key, val in later[0].items():
                kw.setdefault(key, val)   # (an argument the earlier rules already broke stays as they broke it)
        assert rc(**kw) == (EINVAL, who + text), (text, kw)


def test_the_count_call_the_host_call_and_set_rows_argument_errors_need_no_gpu():
    L = pkg.lib()
    q, w, c = vp(0x1000), vp(0x2000), vp(0x3000)

    def rc(slot=0, m=7, queries=q, r2=1.0, mask=w, counts=c, flags=1):
        return pkg.count_within_masked_c()(None, slot, m, queries, r2, mask, counts, None, flags), L.knn_last_error().decode()

    who = "knn_index_count_within_masked: "
    assert rc() == (EINVAL, who + "null index") and rc(flags=0) == (EINVAL, who + "null index")
    rules = [
        ("max_dist2 must be >= 0 and not NaN", [dict(r2=-1.0), dict(r2=float("nan"))]),
        ("unknown flag (KNN_QUERY_INIT_KEYS alone is admitted)", [dict(flags=f) for f in BAD_FLAGS]),
        ("slot outside 0 .. 7", [dict(slot=8), dict(slot=-1)]),
        ("m < 1", [dict(m=0)]),
        ("null queries, mask or counts", [dict(queries=None), dict(mask=None), dict(counts=None)]),
    ]
    for text, cases in rules:
        for kw in cases:
            assert rc(**kw) == (EINVAL, who + text), kw
    for i, (text, cases) in enumerate(rules):
        kw = dict(cases[0])
        for _, later in rules[i + 1:]:
            kw.update({key: val for key, val in later[0].items() if key not in kw})
        assert rc(**kw) == (EINVAL, who + text), (text, kw)

    Q = np.zeros((4, 3), dtype=np.float32)
    ind = np.zeros((4, 8), dtype=np.int32)
    words = np.zeros(4, dtype=np.uint32)

    def host(m=4, K=8, queries=Q.ctypes.data, r2=1.0, mask=words.ctypes.data, out=ind.ctypes.data):
        return (pkg.query_topk_masked_host_c()(None, m, K, vp(queries) if queries else None, r2, vp(mask) if mask else None,
                                               vp(out) if out else None, None, None), L.knn_last_error().decode())

    who = "knn_index_query_topk_masked_host: "
    assert host() == (EINVAL, who + "null index")
    for bad in (-1.0, float("nan")):
        assert host(r2=bad) == (EINVAL, who + "max_dist2 must be >= 0 and not NaN")
    assert host(m=0) == (EINVAL, who + "m < 1")
    assert host(K=0) == (EINVAL, who + "K outside 1 .. 64") and host(K=65) == (EINVAL, who + "K outside 1 .. 64")
    assert host(m=INT_MAX // 64 + 1, K=64) == (EINVAL, who + "m * K above INT_MAX")
    for kw in (dict(queries=None), dict(mask=None), dict(out=None)):
        assert host(**kw) == (EINVAL, who + "null queries, mask or indices")

    def set_rows(n=100, rows=q, count=5, value=1, mask=w):
        return pkg.mask_set_rows_c()(0, n, rows, count, value, mask, None), L.knn_last_error().decode()

    who = "knn_mask_set_rows: "
    assert set_rows(n=-1) == (EINVAL, who + "n_local < 0")
    assert set_rows(count=-1) == (EINVAL, who + "count < 0")
    for value in (2, -1):
        assert set_rows(value=value) == (EINVAL, who + "value is 0 (clear) or 1 (set)")
    assert set_rows(rows=None) == (EINVAL, who + "null rows or mask") and set_rows(mask=None) == (EINVAL, who + "null rows or mask")


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def divup(a, b):
    return -(-a // b)


def scan_slices(mc, K, n, cu):
    """Slices of the unmasked exact scans for one chunk of mc queries (knn_exact.hip): about 32 waves per CU (8 for K > 16), at
    least 1024 rows each, the top-K's lists within 128 MiB, at most 65535; then evened out.  K = 0: the count scan."""
    s = cu * (32 if K <= 16 else 8) // divup(mc, 64)
    s = min(s, divup(n, 1024), 65535)
    if K > 0:
        s = min(s, (128 << 20) // (mc * K * 8))
    s = max(s, 1)
    return divup(n, divup(n, s))


def restated_plan(k, m, K, rows, cu, init):
    mc, chunks = min(m, CHUNK), divup(m, CHUNK)
    G = divup(rows, 1024)
    part = 0
    if K > 0:
        ml = m - (chunks - 1) * CHUNK
        part = max(scan_slices(mc, K, rows, cu) * mc * K * 8, scan_slices(ml, K, rows, cu) * ml * K * 8)
    return dict(granules=G, slices=scan_slices(mc, K, rows, cu), chunks=chunks, lds_bytes=K * 64 * 8,
                mask_bytes=(G + 1) * 8 + (G * 4 + 7) // 8 * 8, part_bytes=part, launches=2 + chunks * (2 if K > 0 else 1), chunk_m=mc)


def test_the_plan_against_its_restatement_and_the_unmasked_scans_own_hooks():
    cu = 256
    for k in (1, 16, 17, 128, 129):
        for m in (1, 64, 65, 65536, 65537):
            for K in (0, 1, 16, 17, 64):
                for rows in (1, 1023, 1024, 1025, 1 << 20):
                    for init in (0, 1):
                        got = pkg.debug_masked_plan(k=k, m=m, K=K, rows=rows, num_cu=cu, init=init)
                        assert got == restated_plan(k, m, K, rows, cu, init), (k, m, K, rows, init)
                    mc = min(m, CHUNK)
                    if K > 0:   # what the exact top-K scan's list scratch implies: slices x chunk queries x K keys
                        sc = pkg.debug_topk_scratch(way=pkg.WAY_EXACT, m=m, K=K, n=rows, num_cu=cu, init=1, within=1, pass_m=0,
                                                    grid_scratch_bytes=0)
                        assert sc["part_bytes"] == got["slices"] * mc * K * 8, (k, m, K, rows)
                        assert got["part_bytes"] >= sc["part_bytes"]
                        if m <= CHUNK:
                            assert got["part_bytes"] == sc["part_bytes"]
                    else:
                        cp = pkg.debug_count_plan(k=k, m=m, n=rows, radius_finite=1, flag_grid=0, flag_cells=0, has_grid=0, has_cells=0,
                                                  centred=0, rows_u8=0, bins=0, sharded=0, path=0, cells=0, num_cu=cu, radius_rings=0)
                        assert cp["way"] == 1 and cp["slices"] == got["slices"], (k, m, rows)
                    assert got["slices"] <= got["granules"] and got["lds_bytes"] <= 64 * 1024
    # an empty shard launches nothing but an init top-K's fill
    for K, init, launches in ((8, 1, 1), (8, 0, 0), (0, 1, 0), (0, 0, 0)):
        p = pkg.debug_masked_plan(k=3, m=70, K=K, rows=0, num_cu=cu, init=init)
        assert p["launches"] == launches and p["granules"] == p["slices"] == p["mask_bytes"] == p["part_bytes"] == 0
    L = pkg.lib()
    for kw in (dict(k=0), dict(m=0), dict(K=-1), dict(K=65), dict(m=INT_MAX // 64 + 1, K=64), dict(rows=-1), dict(rows=(1 << 32) + 1),
               dict(num_cu=0), dict(init=2)):
        args = dict(k=3, m=70, K=8, rows=5000, num_cu=cu, init=1)
        args.update(kw)
        with pytest.raises(pkg.KnnError):
            pkg.debug_masked_plan(**args)
        assert L.knn_last_error().decode().startswith("knn_debug_masked_plan")


# ---- the cut by admitted rows ---------------------------------------------------------------------------------------------------
def brute_first(counts, S):
    """g_b = min{ g : P[g] * S >= b * T } by a linear walk in Python integers."""
    P = [0]
    for c in counts:
        P.append(P[-1] + int(c))
    T = P[-1]
    return [next(g for g in range(len(P)) if P[g] * S >= b * T) for b in range(S + 1)], P


def check_split(counts, S):
    counts = np.asarray(counts, dtype=np.uint32)
    first = pkg.debug_mask_split(counts, S)
    want, P = brute_first(counts, S)
    T, G = P[-1], len(counts)
    assert first.tolist() == want, (counts.tolist()[:8], S)
    # g_0 = 0, non-decreasing, inside the granules
    assert first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] <= G
    # every admitted row in exactly one slice: the slices are consecutive and no admitted row lies behind the last
    assert P[int(first[-1])] == T
    held = [P[int(first[b + 1])] - P[int(first[b])] for b in range(S)]
    assert sum(held) == T
    # no slice holds more than T / S plus one granule's admitted rows
    biggest = int(counts.max()) if G else 0
    assert all(h * S < T + (biggest + 1) * S for h in held), (max(held), T, S)
    assert all(h <= T // S + 1 + biggest for h in held)
    if T == 0:
        assert (first == 0).all()
    return first, held


def test_the_split_on_hand_made_granule_counts():
    rng = np.random.default_rng(99)
    for S in (1, 2, 3, 7, 64, 1000):
        check_split(np.full(40, 1024), S)                                  # uniform
        check_split(np.full(40, 17), S)
        one = np.zeros(40, dtype=np.uint32)
        one[13] = 1024
        check_split(one, S)                                                # all in one granule
        last = np.zeros(40, dtype=np.uint32)
        last[-1] = 700
        check_split(last, S)                                               # all in the last
        gaps = np.array([0, 0, 0, 5, 1024, 0, 0, 0, 0, 300, 1, 0, 1024, 1024, 0, 0], dtype=np.uint32)
        check_split(gaps, S)                                               # empty granules in front, between and behind
        check_split(np.zeros(40, dtype=np.uint32), S)                      # T = 0
        check_split(rng.integers(0, 1025, size=333), S)
        check_split([5], S)
        check_split([], S)
    # a contiguous range is spread: 64 full granules inside 4096, 64 slices, one granule each
    rng_mask = np.zeros(4096, dtype=np.uint32)
    rng_mask[1000:1064] = 1024
    first, held = check_split(rng_mask, 64)
    assert held == [1024] * 64 and first[0] == 0 and first[1] == 1001 and first[-1] == 1064
    # T < S: most slices are empty
    first, held = check_split([0, 3, 0, 2, 0], 64)
    assert sum(1 for h in held if h) <= 2 and sum(held) == 5
    first, held = check_split([100], 26)
    assert sorted(held) == [0] * 25 + [100]
    # S = 1: everything in one slice
    first, held = check_split(gaps, 1)
    assert held == [int(gaps.sum())]
    # S = 65535 with few granules
    check_split([1024, 0, 1024], 65535)
    check_split([1], 65535)
    # P * S beyond 2^32 (and beyond 2^40): a million rows per granule, 65535 slices
    check_split(np.full(50, 1 << 20), 65535)
    check_split(rng.integers(0, 1 << 32, size=200, dtype=np.uint64), 4097)
    check_split(np.full(3000, 0xFFFFFFFF), 65535)
    # bad arguments
    L = pkg.lib()
    for counts, S in (([1, 2], 0), ([1, 2], 65536), ([1, 2], -1), (np.full(70000, 0xFFFFFFFF), 3)):
        with pytest.raises(pkg.KnnError):
            pkg.debug_mask_split(counts, S)
        assert L.knn_last_error().decode().startswith("knn_debug_mask_split")


def words_of(n, sel):
    bits = np.zeros(pkg.mask_words(n) * 32, dtype=bool)
    bits[:n][sel] = True
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def check_row_split(n, words, S):
    """The whole cut, row for row, against a linear walk: r_b = min{ r : A(r) * S >= b * T }, A(r) the admitted rows before r."""
    words = np.asarray(words, dtype=np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(np.int64)      # bits at and beyond n do not count
    A = np.concatenate([[0], np.cumsum(bits)])
    T = int(A[-1])
    want = [int(np.argmax(A * S >= b * T)) for b in range(S + 1)]
    first = pkg.debug_mask_split_rows(words, n, S)
    assert first.tolist() == want, (n, S, first.tolist()[:6], want[:6])
    # r_0 = 0, non-decreasing, inside the rows; every admitted row in exactly one slice; equal shares to within one row
    assert first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] <= n and A[first[-1]] == T
    held = A[first[1:]] - A[first[:-1]]
    assert held.sum() == T and held.min() >= T // S and held.max() <= -(-T // S)
    if T == 0:
        assert (first == 0).all()
    # the cut lies in the granule the first step names
    G = -(-n // 1024)
    per_granule = np.add.reduceat(np.concatenate([bits, np.zeros(G * 1024 - n, np.int64)]), np.arange(0, G * 1024, 1024)) if G else []
    gran = pkg.debug_mask_split(per_granule, S)
    assert ((first <= gran * 1024) & ((gran == 0) | (first > (gran - 1) * 1024))).all()
    return first, held


def test_the_row_level_split_spreads_a_contiguous_range_and_drops_the_tail_bits():
    rng = np.random.default_rng(77)
    N = 3 * 1024 + 77
    for S in (1, 2, 4, 26, 64, 512, 65535):
        for sel in ([], [0], [N - 1], np.arange(1100, 1200), np.arange(2000, 2100), rng.random(N) < 0.5, rng.random(N) < 1 / 64,
                    np.arange(N), np.repeat(np.arange(pkg.mask_words(N)) % 2 == 0, 32)[:N]):
            check_row_split(N, words_of(N, sel), S)
        for n in (1, 31, 32, 33, 1023, 1024, 1025):
            check_row_split(n, words_of(n, np.arange(n)), S)
            check_row_split(n, words_of(n, rng.random(n) < 0.3), S)
        check_row_split(0, np.zeros(0, dtype=np.uint32), S)
    # bits at and beyond n in the last word change nothing
    w = words_of(N, rng.random(N) < 0.5)
    dirty = w.copy()
    dirty[-1] |= np.uint32(~((1 << (N % 32)) - 1) & 0xFFFFFFFF)
    assert pkg.debug_mask_split_rows(dirty, N, 64).tolist() == pkg.debug_mask_split_rows(w, N, 64).tolist()
    # one range of 2^16 (2^12) rows inside 2^20, 512 slices: 128 (8) rows each, where granules alone would leave 64 (4) busy slices
    n = 1 << 20
    first, held = check_row_split(n, words_of(n, np.arange(349525, 349525 + 65536)), 512)
    assert (held == 128).all() and first[1] == 349525 + 128 and first[-1] == 349525 + 65536
    first, held = check_row_split(n, words_of(n, np.arange(5001, 5001 + 4096)), 512)
    assert (held == 8).all()
    L = pkg.lib()
    f = L.knn_debug_mask_split_rows
    f.argtypes = [vp, ctypes.c_longlong, ctypes.c_int, vp]
    out = np.zeros(70000, dtype=np.int64)
    for n, S in ((100, 0), (100, 65536), (-1, 4), ((1 << 32) + 1, 4)):
        assert f(w.ctypes.data, n, S, out.ctypes.data) == EINVAL and L.knn_last_error().decode().startswith("knn_debug_mask_split_rows")
    with pytest.raises(ValueError):
        pkg.debug_mask_split_rows(w[:-1], N, 4)


# ---- the kernels' ISA -----------------------------------------------------------------------------------------------------------
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLOAT_FMA = re.compile(r"\bv_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_f32|\bv_dot\d")   # tests/test_host_logic.py's pattern


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_the_masked_scan_kernels_hold_no_fused_multiply_add_and_use_no_scratch(tmp_path):
    """Bit-exactness against v0 needs one rounding per operation; a kernel that keeps its query in registers must not spill."""
    src = os.path.join(ROOT, "multicore_hw2_amd", "csrc", "knn_masked.hip")
    asm = tmp_path / "knn_masked.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                           "-o", str(asm), src])
    text = asm.read_text()
    bodies = re.findall(r"^(_Z\w*(?:knn_masked_topk_kernel|knn_masked_count_kernel)\w*):(.*?)^\.Lfunc_end", text, flags=re.S | re.M)
    assert len(bodies) >= 18, len(bodies)
    for name, body in bodies:
        bad = FLOAT_FMA.findall(body)
        assert not bad, (name, bad[:3])
        assert re.search(r"v_(pk_)?mul_f32", body), name
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        name, meta = m.group(1), m.group(2)
        form = re.search(r"knn_masked_(?:topk|count)_kernelILi(\d)E", name)
        if not form or form.group(1) == "0":
            continue
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1))
        assert scratch == 0, (name, scratch)
        seen += 1
    assert seen == 16, seen
