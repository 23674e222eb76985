"""Top-K on the uniform-grid index (KNN_QUERY_TOPK_GRID, include/knn_mi355x.h section 2c): the host arithmetic through
knn_debug_grid_topk_plan against a restatement, the route with the flag off, and the compiled kernel's metadata.  No GPU."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

import multicore_hw2_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TOPK_CHUNK = 65536   # queries per launch pair of the exact top-K (KNN_TOPK_CHUNK)


def _rmax(k, K):
    """Rings before a query gives up: the 1-NN kernel's, or twice (+ 2) the first ring whose block holds 4 K rows at the
    grid's 3 rows per cell, whichever is more."""
    one_nn = {1: 64, 2: 16, 3: 6, 4: 4}[k]
    need = 0
    while 3 * (2 * need + 1) ** k < 4 * K:
        need += 1
    return max(one_nn, 2 * need + 2)


def _plan(k, K, m, has_grid, path, flag):
    if not (has_grid and flag and path in (0, 3)):
        return dict.fromkeys(pkg.GRID_TOPK_PLAN, 0)
    return dict(use=1, rmax=_rmax(k, K), blocks=-(-m // 4), waves=4, scratch_bytes=m * K * 8,
                launches=1 + 2 * -(-m // TOPK_CHUNK) + 1)


def test_plan_matches_its_restatement():
    for k, K, path, has_grid, flag, m in itertools.product((1, 2, 3, 4), (1, 8, 64), (0, 1, 2, 3), (0, 1), (0, 1),
                                                           (1, 5, 70, 1024, 65537)):
        got = pkg.debug_grid_topk_plan(k=k, K=K, m=m, has_grid=has_grid, path=path, flag=flag)
        assert got == _plan(k, K, m, has_grid, path, flag), (k, K, m, has_grid, path, flag, got)
        if got["use"]:
            assert got["rmax"] >= 1 and got["scratch_bytes"] == m * K * 8 and got["blocks"] * got["waves"] >= m
            assert (2 * got["rmax"] + 1) ** k < 2 ** 31   # a ring's positions are counted in an int
    # K = 64 on one axis: 64 rows at 3 per cell are 22 cells, 11 rings
    assert pkg.debug_grid_topk_plan(k=1, K=64, m=1, has_grid=1, path=0, flag=1)["rmax"] >= 11


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=5), dict(K=0), dict(K=65), dict(m=0), dict(m=-3), dict(m=2 ** 31, K=1),
                                 dict(m=2 ** 26, K=64), dict(path=4), dict(path=-1), dict(has_grid=2), dict(flag=2)])
def test_plan_rejects_bad_inputs(bad):
    inputs = dict(k=3, K=8, m=100, has_grid=1, path=0, flag=1)
    inputs.update(bad)
    with pytest.raises(pkg.KnnError, match="knn_debug_grid_topk_plan"):
        pkg.debug_grid_topk_plan(**inputs)
    assert pkg.lib().knn_debug_grid_topk_plan(None, None) != 0


def test_route_without_the_flag_keeps_top_k_off_the_grid():
    """knn_debug_query_route has no input for the flag and means "flag off": a top-K call on a grid index is the exact top-K's,
    a 1-NN call the grid's."""
    base = dict(k=3, K=8, m=70, n=1 << 20, topk_cells=0, has_cells=0, centred=0, rows_u8=0, bins=0, sharded=0, n_outliers=0,
                ncells=0, nitems=0, cap=0, several_slots=0, scan_blocks=0, scan_deal=0, num_cu=256, rec_cap=1 << 22, cells=0,
                path=0, filter_usable=0, has_grid=1, filter_wanted=0, init_keys=1)
    for path in (0, 3):
        for K in (1, 8, 64):
            assert pkg.debug_query_route(**dict(base, path=path, K=K))["way"] == pkg.WAY_EXACT
        assert pkg.debug_query_route(**dict(base, path=path, K=0))["way"] == pkg.WAY_GRID
    assert pkg.QUERY_TOPK_GRID == 4
    with open(os.path.join(ROOT, "include", "knn_mi355x.h")) as f:
        assert re.search(r"^#define KNN_QUERY_TOPK_GRID 4u$", f.read(), flags=re.M)


def test_entry_points_take_the_flag_only_where_it_means_something():
    """No index, no GPU: knn_index_query_topk's argument check names its own reason, not the flag."""
    L = pkg.lib()
    assert L.knn_index_query_topk(None, 0, 1, 1, None, None, None, None, pkg.QUERY_TOPK_GRID) != 0
    assert L.knn_index_query_topk(None, 0, 1, 1, None, None, None, None, 8) != 0
    assert L.knn_index_query(None, 0, 1, None, None, None, None, pkg.QUERY_TOPK_GRID) != 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not present")
def test_grid_kernels_keep_the_list_in_registers_and_v0_arithmetic(tmp_path):
    """The top-K kernel's sorted list is one packed key per lane: the code object's metadata must show no spill and no
    scratch, for the top-K kernels and (unchanged) the 1-NN ones; distances are v0's: a multiply and an add, never fused."""
    src = os.path.join(ROOT, "multicore_hw2_amd", "csrc", "knn_grid.hip")
    asm = tmp_path / "knn_grid.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                           "-o", str(asm), src])
    text = asm.read_text()
    seen = {"topk": 0, "query": 0}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        name, body = m.group(1), m.group(2)
        kind = re.search(r"knn_grid_(topk|query)_kernel", name)
        if not kind:
            continue
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)) <= 128, name   # four blocks of four waves per SIMD pair
        seen[kind.group(1)] += 1
    assert seen == {"topk": 4, "query": 4}, seen
    meta = re.findall(r"\.name:\s+(\S*knn_grid_(?:topk|query)_kernel\S*)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text)
    spills = dict(meta)
    assert len(spills) == 8 and all(int(v) == 0 for v in spills.values()), spills
    fma = re.compile(r"\bv_(fma|fmac|fmamk|fmaak|mad|mac|madmk|madak|pk_fma)_f32|\bv_dot\d")
    bodies = re.findall(r"^(_Z\w*knn_grid_(?:topk|query)_kernel\w*):(.*?)^\.Lfunc_end", text, flags=re.S | re.M)
    assert len(bodies) == 8
    for name, body in bodies:
        assert not fma.findall(body), name
        assert re.search(r"v_(pk_)?mul_f32", body), name
        assert "s_barrier" not in body, name   # waves leave on their own: no block-level barrier
