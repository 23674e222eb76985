"""multicore_hw2_amd — host-side mirror of the reference's operator boundary for ONE hot path:
brute-force nearest-neighbour search behind ``cudaCallback(k, m, n, searchPoints,
referencePoints, results)`` (reference sources/src/core.h:71, sources/src/core.cu:1282-1297).

The product is ``libknn_mi355x.so`` (hand-written HIP for gfx950 + a C-ABI, see
``include/knn_mi355x.h``).  This package only binds it with ctypes so that tests and
``bench.py`` drive exactly the entry points a C/C++ caller would.  There is no CPU fallback:
importing works anywhere, but every compute entry raises if the library is missing or no GPU
is visible.  PyTorch is plumbing only: callers that hold torch tensors pass ``tensor.data_ptr()`` /
``torch.cuda.current_stream().cuda_stream``; ``lib()`` imports torch (when installed) just before the
dlopen so the process ends up with one HIP runtime whatever the import order was.
"""
import ctypes
import os
import sys

import numpy as np

__all__ = ["lib", "lib_path", "cudaCallback", "KnnIndex", "KnnGeom", "KnnError", "KEY_INIT", "set_option",
           "get_option", "trim", "device_count", "EXPORTED_SYMBOLS", "shard_bounds", "keys_topk_merge", "counts_to_offsets",
           "keys_sort_segments", "keys_topk_merge_large", "debug_topk_large_plan", "debug_radix_kth", "TOPK_LARGE_MAX",
           "mask_words", "mask_set_rows", "debug_masked_plan", "debug_mask_split", "debug_mask_split_rows",
           "list_within_masked_c", "query_topk_large_masked_c", "list_within_masked_host_c", "query_topk_large_masked_host_c",
           "debug_masked_lists_plan",
           "self_topk_c", "self_count_within_c", "self_list_within_c", "self_topk_host_c", "self_list_within_host_c",
           "debug_self_plan", "debug_self_ranges", "debug_slice_chunks", "SLICE_CHUNK",
           "count_within_each_c", "list_within_each_c", "self_count_within_each_c", "self_list_within_each_c",
           "count_within_each_host_c", "list_within_each_host_c", "keys_column_dist2_c", "keys_column_dist2", "debug_each_radius",
           "self_count_within_routed_c", "self_list_within_routed_c", "self_list_within_routed_host_c", "debug_self_routed_plan",
           "count_within_masked_routed_c", "list_within_masked_routed_c",
           "self_cluster_within_c", "self_cluster_within_host_c", "debug_cluster_plan", "debug_cluster_unite", "CLUSTER_NOISE",
           "self_cluster_within_routed_c", "self_cluster_within_routed_host_c", "debug_cluster_routed_plan", "debug_cluster_pair",
           "self_forest_within_c", "self_forest_within_host_c", "debug_forest_plan", "debug_forest_round", "forest_rounds",
           "debug_match_tests"]

KEY_INIT = 0x7F80000000000000

# every symbol include/knn_mi355x.h declares
EXPORTED_SYMBOLS = [
    "cudaCallback", "knn_device_count", "knn_last_error", "knn_version", "knn_index_create",
    "knn_index_destroy", "knn_keys_init", "knn_index_query_keys", "knn_keys_to_indices",
    "knn_index_query_host", "knn_set_option", "knn_get_option", "knn_index_last_stats",
    "knn_synth_fill_device", "knn_index_timing", "knn_index_timing_read",
    "knn_debug_filter_scores", "knn_index_query_keys_slot", "knn_trim", "knn_keys_allreduce_min",
    "knn_index_query_keys_ex", "knn_index_debug_counters", "knn_debug_scan_plan", "knn_debug_scan_plan_ex", "knn_debug_cells_query_plan", "knn_debug_cells_topk_plan", "knn_debug_seed_kth", "knn_debug_topk_gate", "knn_debug_filter_query_plan", "knn_debug_query_route", "knn_debug_index_build_plan", "knn_debug_ingest_head_rows", "knn_debug_shard_policy", "knn_debug_plan_shard", "knn_debug_call_plan", "knn_debug_u8_row", "knn_debug_u8_bin_row", "knn_debug_u8_bin_threshold", "knn_index_query",
    "knn_geom_create", "knn_geom_destroy", "knn_geom_info", "knn_geom_assign", "knn_index_create_sharded",
    "knn_index_seed_export", "knn_index_seed_attach", "knn_geom_first_cell",
    "knn_index_query_topk", "knn_keys_topk_merge", "knn_index_query_topk_host", "knn_debug_grid_topk_plan",
    "knn_index_query_topk_within", "knn_index_query_topk_within_host", "knn_debug_grid_within_plan", "knn_debug_within_bound",
    "knn_debug_frame_dup", "knn_debug_topk_scratch",
    "knn_index_count_within", "knn_index_count_within_host", "knn_debug_count_plan",
    "knn_counts_to_offsets", "knn_index_list_within", "knn_keys_sort_segments", "knn_index_list_within_host",
    "knn_index_query_topk_large", "knn_keys_topk_merge_large", "knn_index_query_topk_large_host", "knn_debug_topk_large_plan",
    "knn_debug_radix_kth",
    "knn_index_query_topk_masked", "knn_index_count_within_masked", "knn_mask_set_rows", "knn_index_query_topk_masked_host",
    "knn_debug_masked_plan", "knn_debug_mask_split", "knn_debug_mask_split_rows",
    "knn_index_list_within_masked", "knn_index_list_within_masked_host", "knn_index_query_topk_large_masked",
    "knn_index_query_topk_large_masked_host", "knn_debug_masked_lists_plan",
    "knn_index_self_topk", "knn_index_self_count_within", "knn_index_self_list_within", "knn_index_self_topk_host",
    "knn_index_self_list_within_host", "knn_debug_self_plan", "knn_debug_self_ranges", "knn_debug_slice_chunks",
    "knn_index_count_within_each", "knn_index_list_within_each", "knn_index_self_count_within_each",
    "knn_index_self_list_within_each", "knn_keys_column_dist2", "knn_index_count_within_each_host",
    "knn_index_list_within_each_host", "knn_debug_each_radius",
    "knn_index_self_count_within_routed", "knn_index_self_list_within_routed", "knn_index_self_list_within_routed_host",
    "knn_debug_self_routed_plan",
    "knn_index_count_within_masked_routed", "knn_index_list_within_masked_routed",
    "knn_index_self_cluster_within", "knn_index_self_cluster_within_host", "knn_debug_cluster_plan", "knn_debug_cluster_unite",
    "knn_index_self_cluster_within_routed", "knn_index_self_cluster_within_routed_host", "knn_debug_cluster_routed_plan",
    "knn_debug_cluster_pair",
    "knn_index_self_forest_within", "knn_index_self_forest_within_host", "knn_debug_forest_plan", "knn_debug_forest_round",
    "knn_debug_cells_fetch", "knn_debug_match_tests",
]
TOPK_LARGE_MAX = 4096   # KNN_TOPK_LARGE_MAX
QUERY_INIT_KEYS = 1   # KNN_QUERY_INIT_KEYS
QUERY_TOPK_PARTIAL = 2   # KNN_QUERY_TOPK_PARTIAL
QUERY_TOPK_GRID = 4   # KNN_QUERY_TOPK_GRID
QUERY_TOPK_FRAMES = 8   # KNN_QUERY_TOPK_FRAMES
QUERY_COUNT_GRID = 16   # KNN_QUERY_COUNT_GRID
QUERY_COUNT_CELLS = 32   # KNN_QUERY_COUNT_CELLS
CLUSTER_NOISE = -1   # KNN_CLUSTER_NOISE

_HERE = os.path.dirname(os.path.abspath(__file__))
# KNN_MI355X_LIB: A/B hook — load another build of the same C-ABI (e.g. a previous commit's .so)
lib_path = os.environ.get("KNN_MI355X_LIB") or os.path.join(_HERE, "libknn_mi355x.so")
_lib = None


class KnnError(RuntimeError):
    pass


def lib():
    """Load libknn_mi355x.so (built in-tree by __graft_entry__.build()); fail loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(lib_path):
        raise KnnError(f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    # A process must hold ONE HIP runtime.  PyTorch-ROCm ships its own libamdhip64 (same SONAME as
    # the system one this library is linked against): whichever is mapped first serves both, but if
    # the system one came first torch later finds "No HIP GPUs".  So when torch is installed it is
    # imported before the dlopen — tests, bench.py and smoke() share device memory with it anyway.
    if "torch" not in sys.modules and os.environ.get("KNN_MI355X_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(lib_path)
    c_int, c_ll, c_vp, c_ull = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_ulonglong
    L.cudaCallback.argtypes = [c_int, c_int, c_int, c_vp, c_vp, ctypes.POINTER(ctypes.POINTER(c_int))]
    L.cudaCallback.restype = None
    L.knn_device_count.restype = c_int
    L.knn_last_error.restype = ctypes.c_char_p
    L.knn_version.restype = ctypes.c_char_p
    L.knn_index_create.argtypes = [ctypes.POINTER(c_vp), c_int, c_int, c_ll, c_vp, c_int, c_ll, c_vp]
    L.knn_index_destroy.argtypes = [c_vp]
    L.knn_index_destroy.restype = None
    L.knn_keys_init.argtypes = [c_int, c_vp, c_int, c_vp]
    L.knn_index_query_keys.argtypes = [c_vp, c_int, c_vp, c_vp, c_vp]
    L.knn_index_query_keys_slot.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_vp]
    L.knn_index_query_keys_ex.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_vp, ctypes.c_uint]
    L.knn_index_query.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint]
    L.knn_keys_to_indices.argtypes = [c_int, c_vp, c_int, c_vp, c_vp]
    L.knn_index_query_host.argtypes = [c_vp, c_int, c_vp, c_vp]
    L.knn_set_option.argtypes = [ctypes.c_char_p, c_ll]
    L.knn_get_option.argtypes = [ctypes.c_char_p]
    L.knn_get_option.restype = c_ll
    L.knn_index_last_stats.argtypes = [c_vp, ctypes.POINTER(c_ll)]
    L.knn_synth_fill_device.argtypes = [c_int, c_vp, c_ll, c_ull, c_ll, c_vp]
    L.knn_index_timing.argtypes = [c_vp, c_int]
    L.knn_debug_filter_scores.argtypes = [c_vp, c_int, c_vp, c_vp, c_vp, ctypes.POINTER(ctypes.c_double)]
    L.knn_index_timing_read.argtypes = [c_vp, ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_double)]
    L.knn_geom_create.argtypes = [ctypes.POINTER(c_vp), c_int, c_ll, c_int, c_vp, c_ll, c_int]
    L.knn_geom_destroy.argtypes = [c_vp]
    L.knn_geom_destroy.restype = None
    L.knn_geom_info.argtypes = [c_vp, ctypes.POINTER(c_ll)]
    L.knn_geom_assign.argtypes = [c_vp, c_int, c_vp, c_ll, c_vp, c_vp]
    L.knn_index_create_sharded.argtypes = [ctypes.POINTER(c_vp), c_int, c_vp, c_int, c_ll, c_vp, c_vp, c_vp]
    L.knn_index_seed_export.argtypes = [c_vp, c_vp, c_vp]
    L.knn_index_seed_attach.argtypes = [c_vp, c_vp]
    L.knn_index_query_topk.argtypes = [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, ctypes.c_uint]
    L.knn_keys_topk_merge.argtypes = [c_int, c_int, c_int, c_vp, c_vp, c_vp]
    L.knn_index_query_topk_host.argtypes = [c_vp, c_int, c_int, c_vp, c_vp, c_vp]
    L.knn_index_query_topk_within.argtypes = [c_vp, c_int, c_int, c_int, c_vp, ctypes.c_float, c_vp, c_vp, c_vp, ctypes.c_uint]
    L.knn_index_query_topk_within_host.argtypes = [c_vp, c_int, c_int, c_vp, ctypes.c_float, c_vp, c_vp, c_vp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise KnnError(f"knn_mi355x error {rc}: {lib().knn_last_error().decode(errors='replace')}")


def device_count():
    return lib().knn_device_count()


def set_option(name, value):
    _check(lib().knn_set_option(name.encode(), int(value)))


def get_option(name):
    return lib().knn_get_option(name.encode())


def trim():
    """Release the pooled device staging buffers of the host-input entry points; bytes released."""
    f = lib().knn_trim
    f.restype = ctypes.c_longlong
    return int(f())


def debug_shard_policy(k, m, n, ndev):
    """knn_debug_shard_policy: GPUs a cudaCallback(k, m, n) uses on a node with ndev devices (host arithmetic)."""
    f = lib().knn_debug_shard_policy
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int]
    rc = f(int(k), int(m), int(n), int(ndev))
    if rc < 0:
        _check(rc)
    return rc


def debug_scan_plan(num_cu, blocks_per_cu, nitems, m, self_lists=False):
    """knn_debug_scan_plan[_ex]: sizes of one scan launch of the cell-pruned path (host arithmetic; works without a GPU)."""
    out = (ctypes.c_longlong * 8)()
    f = lib().knn_debug_scan_plan_ex
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    _check(f(int(num_cu), int(blocks_per_cu), int(nitems), int(m), 1 if self_lists else 0, out))
    return dict(zip(("blocks", "nlists", "slice", "ovf_base", "ovf_cap", "lds_bytes", "rec_cap", "max_lists"), list(out)))


CELLS_QUERY_INPUTS = ("k", "kt", "centred", "rows_u8", "ncells", "nitems", "cap", "several_slots", "scan_blocks", "scan_deal",
                      "cells_lists", "m", "num_cu", "rec_cap")
CELLS_QUERY_PLAN = ("prep_pw", "prep_kt", "prep_ctr", "self_lists", "match_waves", "stage", "match_lds",
                    "scan_dyn", "scan_k", "scan_self", "scan_kt", "scan_ctr", "scan_nif", "scan_u8",
                    "blocks", "waves", "nlists", "slice", "ovf_base", "ovf_cap", "lds_bytes", "list_cap",
                    "tail_k", "tail_kt", "tail_blocks", "exact_launch", "scan_lds_limit", "match_lds_limit")


def debug_cells_query_plan(**inputs):
    """knn_debug_cells_query_plan: every choice and size one batch of the cell-pruned query launches with, for the inputs
    named in CELLS_QUERY_INPUTS (host arithmetic; works without a GPU)."""
    vin = (ctypes.c_longlong * len(CELLS_QUERY_INPUTS))(*[int(inputs[n]) for n in CELLS_QUERY_INPUTS])
    out = (ctypes.c_longlong * len(CELLS_QUERY_PLAN))()
    f = lib().knn_debug_cells_query_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(CELLS_QUERY_PLAN, list(out)))


CELLS_TOPK_INPUTS = ("k", "K", "m", "n", "topk_cells", "has_cells", "centred", "rows_u8", "bins", "sharded", "n_outliers", "ncells",
                     "nitems", "cap", "several_slots", "scan_blocks", "scan_deal", "num_cu", "rec_cap", "cells")
CELLS_TOPK_PLAN = ("use", "prep_pw", "prep_kt", "prep_ctr", "match_waves", "stage", "scan_dyn", "scan_kt", "scan_nif",
                   "scan_u8", "scan_self", "scan_ctr", "blocks", "waves", "nlists", "slice", "ovf_base", "ovf_cap", "lds_bytes",
                   "list_cap", "ccap", "passes", "scan_lds_limit", "match_lds_limit", "pass_m")


def debug_cells_topk_plan(**inputs):
    """knn_debug_cells_topk_plan: whether a top-K call takes the cell-pruned scan, and every choice and size of one of its
    passes, for the inputs named in CELLS_TOPK_INPUTS (host arithmetic; works without a GPU)."""
    vin = (ctypes.c_longlong * len(CELLS_TOPK_INPUTS))(*[int(inputs[n]) for n in CELLS_TOPK_INPUTS])
    out = (ctypes.c_longlong * len(CELLS_TOPK_PLAN))()
    f = lib().knn_debug_cells_topk_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(CELLS_TOPK_PLAN, list(out)))


def debug_seed_kth(seed, wide, K, pw=4):
    """knn_debug_seed_kth: the K-th smallest finite seed score as the top-K preparation kernel selects it (+inf: fewer than K
    finite even with the wide sample).  Host arithmetic; works without a GPU."""
    a = np.ascontiguousarray(seed, dtype=np.float32).reshape(-1)
    b = np.ascontiguousarray(wide, dtype=np.float32).reshape(-1)
    out = ctypes.c_float()
    f = lib().knn_debug_seed_kth
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                  ctypes.POINTER(ctypes.c_float)]
    _check(f(a.ctypes.data if a.size else None, a.size, b.ctypes.data if b.size else None, b.size, int(K), int(pw), out))
    return float(out.value)


def debug_topk_gate(k, sigma, amax, bmax, nmax, u, mq):
    """knn_debug_topk_gate: (score threshold, Dup, the top-K re-rank's distance gate) for a seed score u.  Host arithmetic."""
    out = (ctypes.c_double * 3)()
    f = lib().knn_debug_topk_gate
    f.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_double] * 5 + [ctypes.POINTER(ctypes.c_double)]
    _check(f(int(k), float(sigma), float(amax), float(bmax), float(nmax), float(u), float(mq), out))
    return tuple(out)


def debug_within_bound(k, sigma, amax, bmax, nmax, u, mq, max_dist2):
    """knn_debug_within_bound: debug_topk_gate's three values for a call of query_topk_within with radius max_dist2 (squared):
    Dup capped at sigma^2 (max_dist2 (1 + g2) + tau); u = +INF leaves the cap alone.  Host arithmetic."""
    out = (ctypes.c_double * 3)()
    f = lib().knn_debug_within_bound
    f.argtypes = [ctypes.c_int, ctypes.c_float] + [ctypes.c_double] * 5 + [ctypes.c_float, ctypes.POINTER(ctypes.c_double)]
    _check(f(int(k), float(sigma), float(amax), float(bmax), float(nmax), float(u), float(mq), float(max_dist2), out))
    return tuple(out)


CELL_FRAME_WORDS = 20   # KNN_CELL_FRAME_WORDS: a cell's centre [16], scale, ratio, bmax, nmax


def debug_frame_dup(k, frame, query_row, u):
    """knn_debug_frame_dup: (Dup, far) — the frame-free bound, in the shard's scaled units, that the per-cell-frame top-K form of
    the preparation kernel makes of seed score u of a cell with this frame for this query row, and whether the query does not fit
    the frame (the far branch).  Host arithmetic, the kernel's own lines (knn_frame_dup.h); works without a GPU."""
    fr = np.ascontiguousarray(frame, dtype=np.float32).reshape(-1)
    q = np.ascontiguousarray(query_row, dtype=np.float32).reshape(-1)
    if fr.size != CELL_FRAME_WORDS or q.size < int(k):
        raise KnnError("debug_frame_dup: frame of %d floats and a query row of k floats" % CELL_FRAME_WORDS)
    out = (ctypes.c_float * 2)()
    f = lib().knn_debug_frame_dup
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.POINTER(ctypes.c_float)]
    _check(f(int(k), fr.ctypes.data, q.ctypes.data, float(u), out))
    return float(out[0]), bool(out[1])


FILTER_QUERY_INPUTS = ("kt", "ntiles", "m", "num_cu", "rec_cap", "topk", "filter_qt", "filter_rounds", "filter_chain",
                       "run_thresholds", "sample_stride")
FILTER_QUERY_PLAN = ("ok", "form", "kt", "npieces", "nlists", "slice", "stride", "sample_blocks", "umin_floats", "topk", "thr_nb",
                     "thr_running", "scan_running", "in_chain", "chained", "has_rows")
FILTER_PIECE = ("qt", "begin", "count", "gx", "gy", "list_base")


def debug_filter_query_plan(**inputs):
    """knn_debug_filter_query_plan: every choice and size one batch of the dense filter query launches with, for the inputs
    named in FILTER_QUERY_INPUTS (host arithmetic; works without a GPU).  form: 0 register pieces, 1 LDS-tiled, 2 chunked-K;
    "pieces": the npieces launches; "rerank": the re-rank's (n, list_base[4], qrow_base[4])."""
    vin = (ctypes.c_longlong * len(FILTER_QUERY_INPUTS))(*[int(inputs[n]) for n in FILTER_QUERY_INPUTS])
    out = (ctypes.c_longlong * 49)()
    f = lib().knn_debug_filter_query_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    v = list(out)
    p = dict(zip(FILTER_QUERY_PLAN, v))
    p["pieces"] = [dict(zip(FILTER_PIECE, v[16 + 6 * i:22 + 6 * i])) for i in range(p["npieces"])]
    p["rerank"] = (v[40], tuple(v[41:45]), tuple(v[45:49]))
    return p


QUERY_ROUTE_INPUTS = CELLS_TOPK_INPUTS + ("path", "filter_usable", "has_grid", "filter_wanted", "init_keys")
QUERY_ROUTE = ("way", "fill_keys_first", "ccap", "topk_use", "passes", "pass_m")
WAY_EXACT, WAY_FILTER, WAY_GRID, WAY_CELLS = 1, 2, 3, 4   # last_stats()[0]


def debug_query_route(**inputs):
    """knn_debug_query_route: which path answers a call (last_stats()[0]) for the inputs named in QUERY_ROUTE_INPUTS — K = 0: a
    1-NN call; sharded: 0, 1, or 2 (a cell-range shard whose call carries KNN_QUERY_TOPK_PARTIAL); centred: 0, 1, or 2 (per-cell
    frames and the call carries KNN_QUERY_TOPK_FRAMES).  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(QUERY_ROUTE_INPUTS))(*[int(inputs[n]) for n in QUERY_ROUTE_INPUTS])
    out = (ctypes.c_longlong * len(QUERY_ROUTE))()
    f = lib().knn_debug_query_route
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(QUERY_ROUTE, list(out)))


GRID_TOPK_INPUTS = ("k", "K", "m", "has_grid", "path", "flag")
GRID_TOPK_PLAN = ("use", "rmax", "blocks", "waves", "scratch_bytes", "launches")


def debug_grid_topk_plan(**inputs):
    """knn_debug_grid_topk_plan: whether the grid index answers a top-K call that carries KNN_QUERY_TOPK_GRID and what the
    call launches with, for the inputs named in GRID_TOPK_INPUTS.  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(GRID_TOPK_INPUTS))(*[int(inputs[n]) for n in GRID_TOPK_INPUTS])
    out = (ctypes.c_longlong * len(GRID_TOPK_PLAN))()
    f = lib().knn_debug_grid_topk_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(GRID_TOPK_PLAN, list(out)))


GRID_WITHIN_INPUTS = GRID_TOPK_INPUTS + ("radius_rings",)


def debug_grid_within_plan(**inputs):
    """knn_debug_grid_within_plan: debug_grid_topk_plan for a call of query_topk_within whose radius spans radius_rings rings of
    the grid (GRID_WITHIN_INPUTS).  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(GRID_WITHIN_INPUTS))(*[int(inputs[n]) for n in GRID_WITHIN_INPUTS])
    out = (ctypes.c_longlong * len(GRID_TOPK_PLAN))()
    f = lib().knn_debug_grid_within_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(GRID_TOPK_PLAN, list(out)))


COUNT_PLAN_INPUTS = ("k", "m", "n", "radius_finite", "flag_grid", "flag_cells", "has_grid", "has_cells", "centred", "rows_u8", "bins",
                     "sharded", "path", "cells", "num_cu", "radius_rings")
COUNT_PLAN = ("way", "passes", "pass_m", "rmax", "blocks", "waves", "slices", "scratch_bytes")


def debug_count_plan(**inputs):
    """knn_debug_count_plan: which way answers a count_within call (last_stats()[0]) and what it launches with, for the inputs
    named in COUNT_PLAN_INPUTS.  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(COUNT_PLAN_INPUTS))(*[int(inputs[n]) for n in COUNT_PLAN_INPUTS])
    out = (ctypes.c_longlong * len(COUNT_PLAN))()
    f = lib().knn_debug_count_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(COUNT_PLAN, list(out)))


TOPK_SCRATCH_INPUTS = ("way", "m", "K", "n", "num_cu", "init", "within", "pass_m", "grid_scratch_bytes")
TOPK_SCRATCH_PLAN = ("part_bytes", "cand_bytes", "lists_bytes")


def debug_topk_scratch(**inputs):
    """knn_debug_topk_scratch: the bytes a workspace slot's three top-K buffers must hold for a call, for the inputs named in
    TOPK_SCRATCH_INPUTS (way: WAY_EXACT .. WAY_CELLS).  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(TOPK_SCRATCH_INPUTS))(*[int(inputs[n]) for n in TOPK_SCRATCH_INPUTS])
    out = (ctypes.c_longlong * len(TOPK_SCRATCH_PLAN))()
    f = lib().knn_debug_topk_scratch
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(TOPK_SCRATCH_PLAN, list(out)))


INDEX_BUILD_INPUTS = ("k", "n_local", "refs_on_device", "build_filter", "build_grid", "path", "cells", "ingest", "cells_build")
INDEX_BUILD_PLAN = ("filter_wanted", "want_cells", "build_filter", "grid_planned", "want_layouts", "ingest")


def debug_index_build_plan(**inputs):
    """knn_debug_index_build_plan: what an index is built with, for the inputs named in INDEX_BUILD_INPUTS (ingest out: 0 copy
    then build, 1 layouts under the copy, 2 cell sort under the copy).  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(INDEX_BUILD_INPUTS))(*[int(inputs[n]) for n in INDEX_BUILD_INPUTS])
    out = (ctypes.c_longlong * len(INDEX_BUILD_PLAN))()
    f = lib().knn_debug_index_build_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(INDEX_BUILD_PLAN, list(out)))


def debug_ingest_head_rows(k, n, granule):
    """knn_debug_ingest_head_rows: rows of the first of the (at most two) copies an index created from host rows ships its
    shard in (granule 1024: plain layouts under the copy, 4096: cell sort under the copy); the second copy is the rest.  Host
    arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * 3)(int(k), int(n), int(granule))
    out = (ctypes.c_longlong * 1)()
    f = lib().knn_debug_ingest_head_rows
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return int(out[0])


def debug_plan_shard(k, m, rows):
    """knn_debug_plan_shard: how one shard of a one-shot call would be served (host arithmetic; works without a GPU)."""
    out = (ctypes.c_longlong * 4)()
    f = lib().knn_debug_plan_shard
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    _check(f(int(k), int(m), int(rows), out))
    return dict(zip(("filter", "streamed", "grid", "chunks"), list(out)))


CALL_PLAN_FIELDS = ("shards", "per", "threads", "rccl", "refusal", "empty", "last_rows", "probed")


def debug_call_plan(k, m, n, ndev, rccl_usable=True):
    """knn_debug_call_plan: what a cudaCallback(k, m, n) decides under the current options on a node with ndev devices where
    RCCL can (not) be used; first_way / last_way: how shard 0 and the last non-empty shard are served (host arithmetic; works
    without a GPU)."""
    vin = (ctypes.c_longlong * 5)(int(k), int(m), int(n), int(ndev), 1 if rccl_usable else 0)
    out = (ctypes.c_longlong * 16)()
    f = lib().knn_debug_call_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    plan = dict(zip(CALL_PLAN_FIELDS, list(out)[:8]))
    ways = ("filter", "streamed", "grid", "chunks")            # as debug_plan_shard names them
    plan["first_way"], plan["last_way"] = dict(zip(ways, list(out)[8:12])), dict(zip(ways, list(out)[12:16]))
    return plan


def shard_bounds(n, shards):
    """Contiguous index ranges of the reference set, one per shard: the partition of reference
    core.cu:875-883 (ceil(n/G) per shard, the last takes the rest; possibly empty)."""
    shards = max(1, min(int(shards), int(n)))
    per = -(-n // shards)
    return [(min(g * per, n), min(g * per + per, n)) for g in range(shards)]


def _as_f32(a, count, name):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if a.size != count:
        raise ValueError(f"{name}: expected {count} floats, got {a.size}")
    return a


def cudaCallback(k, m, n, searchPoints, referencePoints):
    """The drop-in entry with the reference's argument meaning (core.h:71): host fp32 arrays
    ``searchPoints[m*k]``, ``referencePoints[n*k]`` row-major; returns the ``int[m]`` the C
    function hands back through ``int **results`` (the malloc'd buffer is freed here, as the
    reference's caller does at main.cu:98,175).  Runtime errors exit the process like the
    reference's CHECK macro (core.h:77-87)."""
    L = lib()
    q = _as_f32(searchPoints, k * m, "searchPoints")
    r = _as_f32(referencePoints, k * n, "referencePoints")
    res = ctypes.POINTER(ctypes.c_int)()
    L.cudaCallback(k, m, n, q.ctypes.data_as(ctypes.c_void_p), r.ctypes.data_as(ctypes.c_void_p),
                   ctypes.byref(res))
    out = np.ctypeslib.as_array(res, shape=(m,)).astype(np.int32, copy=True)
    ctypes.CDLL(None).free(res)
    return out


def count_within_c():
    """knn_index_count_within with its argument types (set here, not in lib(): a library loaded through KNN_MI355X_LIB for an
    A/B run may predate the symbol and must still load)."""
    f = lib().knn_index_count_within
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_uint]
    return f


def list_within_c():
    """knn_index_list_within with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_list_within
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def query_topk_large_c():
    """knn_index_query_topk_large with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_query_topk_large
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def keys_topk_merge_large_c():
    f = lib().knn_keys_topk_merge_large
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return f


def query_topk_large_host_c():
    f = lib().knn_index_query_topk_large_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p]
    return f


def keys_topk_merge_large(a_dev, b_dev, m, K, device=0, stream=0):
    """Async (knn_keys_topk_merge_large): b[j] <- the K smallest of a[j] and b[j], device arrays of m sorted lists of K <= 4096
    keys, in place."""
    _check(keys_topk_merge_large_c()(int(device), int(m), int(K), ctypes.c_void_p(int(a_dev)), ctypes.c_void_p(int(b_dev)),
                                     ctypes.c_void_p(stream)))


TOPK_LARGE_INPUTS = ("k", "m", "K", "rows", "num_cu", "init")
TOPK_LARGE_PLAN = ("chunks", "slices", "dist_passes", "index_passes", "lds_bytes", "scratch_bytes", "launches_clean", "launches_ties")


def debug_topk_large_plan(**inputs):
    """knn_debug_topk_large_plan: what a query_topk_large call launches with and the slot scratch it needs, for the inputs named
    in TOPK_LARGE_INPUTS.  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(TOPK_LARGE_INPUTS))(*[int(inputs[n]) for n in TOPK_LARGE_INPUTS])
    out = (ctypes.c_longlong * len(TOPK_LARGE_PLAN))()
    f = lib().knn_debug_topk_large_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(TOPK_LARGE_PLAN, list(out)))


def debug_radix_kth(keys, K):
    """knn_debug_radix_kth: (T, passes_run) of the radix select over the given uint64 keys, through the pick kernel's own lines
    (knn_radix_pick.h) — exactly min(K, n) of distinct keys are <= T; passes_run above 4: the index word's passes ran.  Host
    arithmetic; works without a GPU."""
    a = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    kth, passes = ctypes.c_ulonglong(), ctypes.c_int()
    f = lib().knn_debug_radix_kth
    f.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_int)]
    _check(f(a.ctypes.data if a.size else None, a.size, int(K), ctypes.byref(kth), ctypes.byref(passes)))
    return int(kth.value), int(passes.value)


def query_topk_masked_c():
    """knn_index_query_topk_masked with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_query_topk_masked
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def count_within_masked_c():
    """knn_index_count_within_masked with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_count_within_masked
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_uint]
    return f


def query_topk_masked_host_c():
    f = lib().knn_index_query_topk_masked_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p]
    return f


def mask_set_rows_c():
    f = lib().knn_mask_set_rows
    f.argtypes = [ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return f


def mask_words(n):
    """The uint32 words of a row mask over n local rows: bit i % 32 of word i // 32 admits row i."""
    return (int(n) + 31) // 32


def mask_set_rows(n_local, rows_dev, count, value, mask_dev, device=0, stream=0):
    """Async (knn_mask_set_rows): the mask bits of the local rows rows_dev[count] (uint32) <- value (1 set, 0 clear); rows outside
    0 .. n_local - 1 are ignored.  Allow-lists: zero the mask, then set; tombstones: fill it with ones, then clear."""
    _check(mask_set_rows_c()(int(device), int(n_local), ctypes.c_void_p(int(rows_dev)) if rows_dev else None, int(count),
                             int(value), ctypes.c_void_p(int(mask_dev)), ctypes.c_void_p(stream)))


MASKED_PLAN_INPUTS = ("k", "m", "K", "rows", "num_cu", "init")
MASKED_PLAN = ("granules", "slices", "chunks", "lds_bytes", "mask_bytes", "part_bytes", "launches", "chunk_m")


def debug_masked_plan(**inputs):
    """knn_debug_masked_plan: what a query_topk_masked (K >= 1) or count_within_masked (K = 0) call launches with and the slot
    scratch it needs, for the inputs named in MASKED_PLAN_INPUTS.  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(MASKED_PLAN_INPUTS))(*[int(inputs[n]) for n in MASKED_PLAN_INPUTS])
    out = (ctypes.c_longlong * len(MASKED_PLAN))()
    f = lib().knn_debug_masked_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(MASKED_PLAN, list(out)))


def debug_mask_split(granule_counts, slices):
    """knn_debug_mask_split: first_granule[0 .. slices] (int64) — the granules [first[b],
    first[b + 1]) at the cut's first step — for the given admitted rows per granule, through the kernels' own lines
    (knn_mask_split.h).  Host arithmetic; works without a GPU."""
    a = np.ascontiguousarray(granule_counts, dtype=np.uint32).reshape(-1)
    out = np.empty(int(slices) + 1 if int(slices) >= 0 else 1, dtype=np.int64)
    f = lib().knn_debug_mask_split
    f.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    _check(f(a.ctypes.data if a.size else None, a.size, int(slices), out.ctypes.data))
    return out


def debug_mask_split_rows(mask, n_local, slices):
    """knn_debug_mask_split_rows: first_row[0 .. slices] (int64) — slice b of the masked scans is the rows [first[b],
    first[b + 1]) — for the uint32 words of a mask over n_local rows, through the kernels' own lines (knn_mask_split.h).  Host
    arithmetic; works without a GPU."""
    a = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
    if a.size != mask_words(n_local):
        raise ValueError("mask: expected %d words, got %d" % (mask_words(n_local), a.size))
    out = np.empty(int(slices) + 1 if int(slices) >= 0 else 1, dtype=np.int64)
    f = lib().knn_debug_mask_split_rows
    f.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    _check(f(a.ctypes.data if a.size else None, int(n_local), int(slices), out.ctypes.data))
    return out


def list_within_masked_c():
    """knn_index_list_within_masked with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_list_within_masked
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def query_topk_large_masked_c():
    """knn_index_query_topk_large_masked with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_query_topk_large_masked
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def list_within_masked_host_c():
    f = lib().knn_index_list_within_masked_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.POINTER(ctypes.c_int)), ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    return f


def query_topk_large_masked_host_c():
    f = lib().knn_index_query_topk_large_masked_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p]
    return f


MASKED_LISTS_PLAN = ("granules", "slices", "slice_waves", "chunks", "lds_bytes", "mask_bytes", "select_bytes", "launches")


def debug_masked_lists_plan(**inputs):
    """knn_debug_masked_lists_plan: what a list_within_masked (K = 0) or query_topk_large_masked (K >= 1) call launches with and
    the slot scratch it needs, for the inputs named in MASKED_PLAN_INPUTS.  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(MASKED_PLAN_INPUTS))(*[int(inputs[n]) for n in MASKED_PLAN_INPUTS])
    out = (ctypes.c_longlong * len(MASKED_LISTS_PLAN))()
    f = lib().knn_debug_masked_lists_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(MASKED_LISTS_PLAN, list(out)))


def self_topk_c():
    """knn_index_self_topk with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_topk
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def self_count_within_c():
    """knn_index_self_count_within with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_count_within
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_uint]
    return f


def self_list_within_c():
    """knn_index_self_list_within with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_list_within
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def self_topk_host_c():
    f = lib().knn_index_self_topk_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return f


def self_list_within_host_c():
    f = lib().knn_index_self_list_within_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.POINTER(ctypes.POINTER(ctypes.c_int)),
                  ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    return f


SELF_PLAN_INPUTS = ("k", "rows", "K", "shard_rows", "num_cu", "init")
SELF_PLAN = ("chunks", "slices", "groups", "lds_bytes", "part_bytes", "launches", "chunk_rows", "through_bytes")
SELF_RANGES = ("b0", "b1", "w0", "w1", "a0", "a1")


def debug_self_plan(**inputs):
    """knn_debug_self_plan: what a self_topk (K >= 1), self_count_within (K = 0) or self_list_within (K = -1) call launches with
    and the slot scratch it needs, for the inputs named in SELF_PLAN_INPUTS.  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(SELF_PLAN_INPUTS))(*[int(inputs[n]) for n in SELF_PLAN_INPUTS])
    out = (ctypes.c_longlong * len(SELF_PLAN))()
    f = lib().knn_debug_self_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(SELF_PLAN, list(out)))


def debug_self_ranges(i0, i1, w0, w1):
    """knn_debug_self_ranges: how a block of the self-scans cuts its slice [i0, i1) around its window of own rows [w0, w1), through
    the kernels' own lines (knn_self_window.h): the six bounds named in SELF_RANGES.  Host arithmetic; works without a GPU."""
    out = (ctypes.c_longlong * 6)()
    f = lib().knn_debug_self_ranges
    f.argtypes = [ctypes.c_longlong] * 4 + [ctypes.POINTER(ctypes.c_longlong)]
    _check(f(int(i0), int(i1), int(w0), int(w1), out))
    return dict(zip(SELF_RANGES, list(out)))


SLICE_CHUNK = ("c0", "mc", "slices", "per", "grid_x", "grid_y")
SLICE_RULES = {"count": 0, "topk": 1, "select": 2}


def debug_slice_chunks(m, n, num_cu, K=0, rule="count"):
    """knn_debug_slice_chunks: the chunks of <= 65536 queries the exact slice scans walk m queries in, and each chunk's cut of n rows
    under a slice rule ("count", "topk" with K, "select"): a list of dicts with the names in SLICE_CHUNK.  Host arithmetic; works
    without a GPU."""
    cap = (int(m) + 65535) // 65536 if m > 0 else 1
    out = ((ctypes.c_longlong * 6) * cap)()
    chunks = ctypes.c_int(0)
    vin = (ctypes.c_longlong * 5)(int(m), int(n), int(num_cu), int(K), SLICE_RULES[rule])
    f = lib().knn_debug_slice_chunks
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    _check(f(vin, cap, ctypes.cast(out, ctypes.c_void_p), ctypes.byref(chunks)))
    return [dict(zip(SLICE_CHUNK, list(out[i]))) for i in range(chunks.value)]


def count_within_each_c():
    """knn_index_count_within_each with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_count_within_each
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_uint]
    return f


def list_within_each_c():
    """knn_index_list_within_each with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_list_within_each
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def self_count_within_each_c():
    """knn_index_self_count_within_each with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_count_within_each
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_uint]
    return f


def self_list_within_each_c():
    """knn_index_self_list_within_each with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_list_within_each
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def self_count_within_routed_c():
    """knn_index_self_count_within_routed with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_count_within_routed
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_uint]
    return f


def self_list_within_routed_c():
    """knn_index_self_list_within_routed with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_list_within_routed
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def count_within_masked_routed_c():
    """knn_index_count_within_masked_routed with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_count_within_masked_routed
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_uint]
    return f


def list_within_masked_routed_c():
    """knn_index_list_within_masked_routed with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_list_within_masked_routed
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    return f


def self_cluster_within_c():
    """knn_index_self_cluster_within with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_cluster_within
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_uint]
    return f


def self_cluster_within_host_c():
    f = lib().knn_index_self_cluster_within_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.c_longlong)]
    return f


CLUSTER_PLAN_INPUTS = ("k", "n", "num_cu", "core_given", "grid")
CLUSTER_PLAN = ("chunks", "slices", "launches_exact", "launches_grid", "scratch_bytes", "count_bytes", "way", "launches")


def debug_cluster_plan(**inputs):
    """knn_debug_cluster_plan: what a self_cluster_within call on a shard of n rows launches and the slot scratch it needs, for the
    inputs named in CLUSTER_PLAN_INPUTS (core_given: the caller passes core_dev; grid: the grid way answers, k <= 4).  Host
    arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(CLUSTER_PLAN_INPUTS))(*[int(inputs[n]) for n in CLUSTER_PLAN_INPUTS])
    out = (ctypes.c_longlong * len(CLUSTER_PLAN))()
    f = lib().knn_debug_cluster_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(CLUSTER_PLAN, list(out)))


def debug_cluster_unite(parent, pairs):
    """knn_debug_cluster_unite: the kernels' own union-find lines (knn_cluster_uf.h) with the host's atomics — unite(a, b) for every
    row of pairs [npairs][2], in order, on parent (int32 [n], changed IN PLACE; parent[x] <= x on entry).  Works without a GPU."""
    if not (isinstance(parent, np.ndarray) and parent.dtype == np.int32 and parent.flags.c_contiguous and parent.ndim == 1):
        raise ValueError("parent must be a contiguous one-dimensional int32 array (it is changed in place)")
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    f = lib().knn_debug_cluster_unite
    f.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong]
    _check(f(parent.ctypes.data_as(ctypes.c_void_p), parent.size, pr.ctypes.data_as(ctypes.c_void_p), pr.shape[0]))
    return parent


def self_cluster_within_routed_c():
    """knn_index_self_cluster_within_routed with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_cluster_within_routed
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_uint]
    return f


def self_cluster_within_routed_host_c():
    f = lib().knn_index_self_cluster_within_routed_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.c_longlong)]
    return f


CLUSTER_ROUTED_PLAN = ("way", "passes", "pass_m", "launches", "launches_outliers", "scratch_bytes", "count_bytes", "chunks")
PAIR_ACTIONS = ("nothing", "unite", "border")


def debug_cluster_routed_plan(core_given=1, **inputs):
    """knn_debug_cluster_routed_plan: which way answers a self_cluster_within_routed call and what the whole call launches, for the
    inputs named in COUNT_PLAN_INPUTS (m: the shard's rows, equal to n) and core_given (the caller passes core_dev); the outputs
    are named in CLUSTER_ROUTED_PLAN.  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * (len(COUNT_PLAN_INPUTS) + 1))(*([int(inputs[n]) for n in COUNT_PLAN_INPUTS] + [int(core_given)]))
    out = (ctypes.c_longlong * len(CLUSTER_ROUTED_PLAN))()
    f = lib().knn_debug_cluster_routed_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(CLUSTER_ROUTED_PLAN, list(out)))


def debug_cluster_pair(own_core, row_core, row, own):
    """knn_debug_cluster_pair: what the cell-pruned way's link kernels do with the hit (own, row) — one of PAIR_ACTIONS —, by their
    own lines (knn_cluster_pair.h) compiled for the host.  Works without a GPU."""
    action = ctypes.c_int(-1)
    f = lib().knn_debug_cluster_pair
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)]
    _check(f(int(own_core), int(row_core), int(row), int(own), ctypes.byref(action)))
    return PAIR_ACTIONS[action.value]


def self_forest_within_c():
    """knn_index_self_forest_within with its argument types (set here, not in lib(), as count_within_c)."""
    f = lib().knn_index_self_forest_within
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_uint]
    return f


def self_forest_within_host_c():
    f = lib().knn_index_self_forest_within_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.c_longlong)]
    return f


FOREST_PLAN_INPUTS = ("k", "n", "num_cu", "grid")
FOREST_PLAN = ("rounds", "chunks", "slices", "launches_exact", "launches_grid", "scratch_bytes", "way", "launches")


def forest_rounds(n):
    """ROUNDS(n) = max(1, ceil(log2 n)): the Borůvka rounds a self_forest_within call on n rows queues."""
    return max(1, (int(n) - 1).bit_length())


def debug_forest_plan(**inputs):
    """knn_debug_forest_plan: what a self_forest_within call on a shard of n rows launches and the slot scratch it needs, for the
    inputs named in FOREST_PLAN_INPUTS (grid: the grid way answers, k <= 4).  Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(FOREST_PLAN_INPUTS))(*[int(inputs[n]) for n in FOREST_PLAN_INPUTS])
    out = (ctypes.c_longlong * len(FOREST_PLAN))()
    f = lib().knn_debug_forest_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(FOREST_PLAN, list(out)))


def debug_forest_round(parent, cand, edge_keys, edge_hi, count, threads=1):
    """knn_debug_forest_round: one Borůvka round's flatten, pick and hook by the kernels' own lines (knn_forest_pick.h,
    knn_cluster_uf.h) with the host's atomics.  parent: int32 [n], changed IN PLACE (parent[x] <= x on entry); cand: uint64 [n],
    row i's key (distance bits << 32 | row) of the nearest row of another component, KEY_INIT for none; edge_keys uint64 [n],
    edge_hi uint32 [n] and count uint32 [2] receive the edges at count[0] on (count[1]: rounds that added one).  threads: host
    threads that share every step's rows.  Returns the edges this round added.  Works without a GPU."""
    for name, a, dt in (("parent", parent, np.int32), ("cand", cand, np.uint64), ("edge_keys", edge_keys, np.uint64),
                        ("edge_hi", edge_hi, np.uint32), ("count", count, np.uint32)):
        if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous and a.ndim == 1):
            raise ValueError("%s must be a contiguous one-dimensional %s array" % (name, np.dtype(dt).name))
    n = parent.size
    if cand.size != n or edge_keys.size < n or edge_hi.size < n or count.size != 2:
        raise ValueError("cand [n], edge_keys and edge_hi [>= n], count [2]")
    added = ctypes.c_int(int(threads))
    f = lib().knn_debug_forest_round
    f.argtypes = [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.c_int)]
    _check(f(n, parent.ctypes.data_as(ctypes.c_void_p), cand.ctypes.data_as(ctypes.c_void_p),
             edge_keys.ctypes.data_as(ctypes.c_void_p), edge_hi.ctypes.data_as(ctypes.c_void_p),
             count.ctypes.data_as(ctypes.c_void_p), ctypes.byref(added)))
    return added.value


def self_list_within_routed_host_c():
    f = lib().knn_index_self_list_within_routed_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.POINTER(ctypes.c_int)), ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    return f


def debug_self_routed_plan(**inputs):
    """knn_debug_self_routed_plan: which way answers a self_count_within_routed / self_list_within_routed call and what it launches
    with, for the inputs named in COUNT_PLAN_INPUTS (m: the call's rows); the outputs are COUNT_PLAN's, slices the exact self-scan's.
    Host arithmetic; works without a GPU."""
    vin = (ctypes.c_longlong * len(COUNT_PLAN_INPUTS))(*[int(inputs[n]) for n in COUNT_PLAN_INPUTS])
    out = (ctypes.c_longlong * len(COUNT_PLAN))()
    f = lib().knn_debug_self_routed_plan
    f.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    _check(f(vin, out))
    return dict(zip(COUNT_PLAN, list(out)))


def count_within_each_host_c():
    f = lib().knn_index_count_within_each_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    return f


def list_within_each_host_c():
    f = lib().knn_index_list_within_each_host
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                  ctypes.POINTER(ctypes.POINTER(ctypes.c_int)), ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
    return f


def keys_column_dist2_c():
    f = lib().knn_keys_column_dist2
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return f


def keys_column_dist2(keys_dev, m, K, column, dist2_dev, device=0, stream=0):
    """Async (knn_keys_column_dist2): dist2_dev[j] (float32) <- the distance half of keys_dev[j * K + column], +INF for a padding
    key: a column of a top-K call's lists as the radii of a *_within_each call, without leaving the device."""
    _check(keys_column_dist2_c()(int(device), ctypes.c_void_p(int(keys_dev)), int(m), int(K), int(column),
                                 ctypes.c_void_p(int(dist2_dev)), ctypes.c_void_p(stream)))


def debug_each_radius(radius, cap):
    """knn_debug_each_radius: (whether a query of this radius has candidates, its bound under cap) through the kernels' own lines
    (knn_each_radius.h).  Host arithmetic; works without a GPU."""
    out = (ctypes.c_float * 2)()
    f = lib().knn_debug_each_radius
    f.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_float)]
    _check(f(float(radius), float(cap), out))
    return bool(out[0]), float(out[1])


def debug_match_tests(lo, hi, dup):
    """knn_debug_match_tests: the match kernel's two tests through the kernel's own lines, on n cases of 64 low entries lo[n][64],
    one high entry hi[n] and one Dup dup[n] -> (queued[n] bool: the block of those 64 cells queues the query on its smallest low
    entry; listed[n]: how many of the 64 cells keep it on their list).  Host arithmetic; works without a GPU."""
    import numpy as np
    lo = np.ascontiguousarray(lo, dtype=np.float32)
    hi = np.ascontiguousarray(hi, dtype=np.float32)
    dup = np.ascontiguousarray(dup, dtype=np.float32)
    n = hi.shape[0]
    if lo.shape != (n, 64) or dup.shape != (n,):
        raise ValueError("debug_match_tests: lo must be [n][64], hi and dup [n]")
    queued, listed = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    f = lib().knn_debug_match_tests
    f.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 5
    _check(f(n, lo.ctypes.data, hi.ctypes.data, dup.ctypes.data, queued.ctypes.data, listed.ctypes.data))
    return queued.astype(bool), listed


def counts_to_offsets_c():
    f = lib().knn_counts_to_offsets
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return f


def keys_sort_segments_c():
    f = lib().knn_keys_sort_segments
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return f


def counts_to_offsets(counts_dev, m, offsets_dev, device=0, stream=0):
    """Async (knn_counts_to_offsets): offsets_dev[m + 1] (uint64) <- the exclusive 64-bit prefix sums of counts_dev[m] (uint32)."""
    _check(counts_to_offsets_c()(int(device), ctypes.c_void_p(int(counts_dev)), int(m), ctypes.c_void_p(int(offsets_dev)),
                                 ctypes.c_void_p(stream)))


def keys_sort_segments(m, offsets_dev, fill_dev, keys_dev, device=0, stream=0):
    """Async (knn_keys_sort_segments): the first min(fill_dev[j], room of segment j) keys of every segment ascending."""
    _check(keys_sort_segments_c()(int(device), int(m), ctypes.c_void_p(int(offsets_dev)), ctypes.c_void_p(int(fill_dev)),
                                  ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream)))


class KnnGeom:
    """Global grid of a cell-range sharded set (knn_geom_* in include/knn_mi355x.h): built from a sample of the GLOBAL set,
    identical on every rank that passes the same sample.  Host arithmetic only: works without a GPU (assign needs one)."""

    def __init__(self, k, n_global, nranks, sample, seed_tiles=0):
        self._h = ctypes.c_void_p()
        s = np.ascontiguousarray(sample, dtype=np.float32).reshape(-1)
        self.k, self.nranks = int(k), int(nranks)
        _check(lib().knn_geom_create(ctypes.byref(self._h), self.k, int(n_global), self.nranks,
                                     s.ctypes.data_as(ctypes.c_void_p), s.size // self.k, int(seed_tiles)))
        out = (ctypes.c_longlong * 8)()
        _check(lib().knn_geom_info(self._h, out))
        (self.bits, self.ncells, self.cells_per_rank, self.seed_tiles, self.part_bytes, self.layer_bytes, self.sa, _) = list(out)

    def first_cell(self, rank):
        f = lib().knn_geom_first_cell
        f.argtypes = [ctypes.c_void_p, ctypes.c_int]
        f.restype = ctypes.c_longlong
        return int(f(self._h, int(rank)))

    def assign(self, rows_dev, n, owner_dev, device=0, stream=0):
        """owner_dev[i] (int32, device) = rank whose cell range holds row i of rows_dev."""
        _check(lib().knn_geom_assign(self._h, int(device), ctypes.c_void_p(int(rows_dev)), int(n),
                                     ctypes.c_void_p(int(owner_dev)), ctypes.c_void_p(stream)))

    def close(self):
        if self._h:
            lib().knn_geom_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KnnIndex:
    """Device-resident shard of the reference set (knn_index_* in include/knn_mi355x.h)."""

    @classmethod
    def sharded(cls, geom, rank, refs_dev, gids_dev, n_local, device=0, stream=0, owners=None):
        """A cell-range shard (knn_index_create_sharded): this rank's rows of the global grid `geom` (device pointers;
        gids strictly ascending).  Give it the seed layer (seed_export on every rank, gather, seed_attach) before querying.
        LIFETIME: the index BORROWS refs_dev and gids_dev (and the layer given to seed_attach) until close() — its prep, scan
        and finalise kernels read them on every query.  Pass the objects that own that memory (torch tensors, ...) as
        `owners` and the wrapper keeps them alive; with raw pointers the caller must."""
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        self.k, self.device, self.base, self.n, self._keep = geom.k, int(device), 0, int(n_local), owners
        self._layer = None
        _check(lib().knn_index_create_sharded(ctypes.byref(self._h), self.device, geom._h, int(rank), self.n,
                                              ctypes.c_void_p(int(refs_dev)), ctypes.c_void_p(int(gids_dev)),
                                              ctypes.c_void_p(stream)))
        return self

    def seed_export(self, layer_dev, stream=0):
        _check(lib().knn_index_seed_export(self._h, ctypes.c_void_p(int(layer_dev)), ctypes.c_void_p(stream)))

    def seed_attach(self, layer_dev, owner=None):
        """The replicated seed layer (device pointer, borrowed until close(): `owner` keeps its memory alive)."""
        _check(lib().knn_index_seed_attach(self._h, ctypes.c_void_p(int(layer_dev))))
        self._layer = owner

    def __init__(self, k, refs, n_local=None, device=0, base_index=0, refs_on_device=False, stream=0, owners=None):
        """refs_on_device: `refs` is a device pointer the index BORROWS until close() (`owners`: what keeps it alive);
        else host rows, copied."""
        self._h = ctypes.c_void_p()
        self._layer = None
        self.k, self.device, self.base = int(k), int(device), int(base_index)
        if refs_on_device:
            if n_local is None:
                raise ValueError("n_local is required with a device pointer")
            ptr = ctypes.c_void_p(int(refs))
            self._keep = None
        else:
            arr = np.ascontiguousarray(refs, dtype=np.float32).reshape(-1)
            if n_local is None:
                n_local = arr.size // self.k
            if arr.size != n_local * self.k:
                raise ValueError("refs size does not match n_local * k")
            ptr = arr.ctypes.data_as(ctypes.c_void_p)
            self._keep = arr
        self.n = int(n_local)
        _check(lib().knn_index_create(ctypes.byref(self._h), self.device, self.k, self.n, ptr,
                                      1 if refs_on_device else 0, self.base, ctypes.c_void_p(stream)))
        self._keep = owners if refs_on_device else None   # (host rows were copied: nothing to hold)

    def query_keys(self, m, queries_dev, keys_dev, stream=0, slot=0, init_keys=False, indices_dev=None):
        """Async: fold this shard's nearest (distance, global index) keys into keys_dev[m].
        slot 0..7 picks one of the index's eight independent query workspaces.  init_keys: the call starts the
        keys at (+INF, 0) itself (KNN_QUERY_INIT_KEYS) instead of folding into what keys_dev holds.
        indices_dev: also write the int32 indices there (knn_index_query: no separate knn_keys_to_indices launch)."""
        if indices_dev is not None:
            _check(lib().knn_index_query(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)),
                                         ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(int(indices_dev)),
                                         ctypes.c_void_p(stream), QUERY_INIT_KEYS if init_keys else 0))
        elif init_keys:
            _check(lib().knn_index_query_keys_ex(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)),
                                                 ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream), QUERY_INIT_KEYS))
        else:
            _check(lib().knn_index_query_keys_slot(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)),
                                                   ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream)))

    def query(self, queries):
        """Synchronous host-in/host-out query of this shard alone."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        out = np.empty(m, dtype=np.int32)
        _check(lib().knn_index_query_host(self._h, m, q.ctypes.data_as(ctypes.c_void_p),
                                          out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def query_topk(self, m, K, queries_dev, keys_dev, stream=0, slot=0, init_keys=False, indices_dev=None, partial=False,
                   grid=False, frames=False):
        """Async (knn_index_query_topk): keys_dev[m][K] <- the K smallest (distance, global index) keys of (this shard's rows
        and, unless init_keys, the K sorted keys per query keys_dev already holds), sorted.  indices_dev: also the int32
        indices [m][K].  partial (KNN_QUERY_TOPK_PARTIAL): the caller merges every shard's lists, so this shard need only
        report the rows that can belong to the global top-K — what lets a cell-range shard take the cell-pruned scan
        (option topk_cells = 1); see include/knn_mi355x.h, 2c, for the contract.  grid (KNN_QUERY_TOPK_GRID): an index that
        has a grid index answers the call with it (last_stats()[0] == 3); on any other index the flag changes nothing.
        frames (KNN_QUERY_TOPK_FRAMES): a cell-sorted layout in per-cell frames answers the call with the cell-pruned top-K
        (last_stats()[0] == 4) under option topk_cells = 1; on any other index or option the flag changes nothing."""
        _check(lib().knn_index_query_topk(self._h, int(slot), int(m), int(K), ctypes.c_void_p(int(queries_dev)),
                                          ctypes.c_void_p(int(keys_dev)),
                                          ctypes.c_void_p(int(indices_dev)) if indices_dev is not None else None,
                                          ctypes.c_void_p(stream),
                                          (QUERY_INIT_KEYS if init_keys else 0) | (QUERY_TOPK_PARTIAL if partial else 0) |
                                          (QUERY_TOPK_GRID if grid else 0) | (QUERY_TOPK_FRAMES if frames else 0)))

    def query_topk_within(self, m, K, queries_dev, max_dist2, keys_dev, stream=0, slot=0, init_keys=False, indices_dev=None,
                          partial=False, grid=False, frames=False):
        """Async (knn_index_query_topk_within): query_topk with a distance cap — only rows whose v0 squared distance is
        <= max_dist2 (fp32, equality inside) are candidates; shorter lists are padded with KEY_INIT.  +INF gives query_topk's
        keys; a negative or NaN radius raises.  Keys keys_dev already holds (a fold) are the caller's and are not clipped."""
        _check(lib().knn_index_query_topk_within(self._h, int(slot), int(m), int(K), ctypes.c_void_p(int(queries_dev)),
                                                 float(max_dist2), ctypes.c_void_p(int(keys_dev)),
                                                 ctypes.c_void_p(int(indices_dev)) if indices_dev is not None else None,
                                                 ctypes.c_void_p(stream),
                                                 (QUERY_INIT_KEYS if init_keys else 0) | (QUERY_TOPK_PARTIAL if partial else 0) |
                                                 (QUERY_TOPK_GRID if grid else 0) | (QUERY_TOPK_FRAMES if frames else 0)))

    def query_topk_within_host(self, queries, K, max_dist2):
        """Synchronous radius-bounded top-K of this shard alone: (indices int32 [m][K], dist2 float32 [m][K] with +INF in
        padding, counts int32 [m]: the entries of each list that are not padding)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        idx = np.empty((m, int(K)), dtype=np.int32)
        d2 = np.empty((m, int(K)), dtype=np.float32)
        counts = np.empty(m, dtype=np.int32)
        _check(lib().knn_index_query_topk_within_host(self._h, m, int(K), q.ctypes.data_as(ctypes.c_void_p), float(max_dist2),
                                                      idx.ctypes.data_as(ctypes.c_void_p), d2.ctypes.data_as(ctypes.c_void_p),
                                                      counts.ctypes.data_as(ctypes.c_void_p)))
        return idx, d2, counts

    def count_within(self, m, queries_dev, max_dist2, counts_dev, stream=0, slot=0, init=False, grid=False, cells=False):
        """Async (knn_index_count_within): counts_dev[m] (uint32) += the rows of this shard whose v0 squared distance is finite
        and <= max_dist2 (fp32, equality inside); init (KNN_QUERY_INIT_KEYS): = instead of +=.  grid (KNN_QUERY_COUNT_GRID) /
        cells (KNN_QUERY_COUNT_CELLS): an index that has a grid index / a one-frame cell-sorted layout answers with it
        (last_stats()[0] == 3 / 4); on any other index the flag changes nothing.  A negative or NaN radius raises."""
        _check(count_within_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                           ctypes.c_void_p(int(counts_dev)), ctypes.c_void_p(stream),
                           (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) | (QUERY_COUNT_CELLS if cells else 0)))

    def count_within_host(self, queries, max_dist2):
        """Synchronous count of this shard alone: uint32 [m]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        counts = np.empty(m, dtype=np.uint32)
        f = lib().knn_index_count_within_host
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
        _check(f(self._h, m, q.ctypes.data_as(ctypes.c_void_p), float(max_dist2), counts.ctypes.data_as(ctypes.c_void_p)))
        return counts

    def list_within(self, m, queries_dev, max_dist2, offsets_dev, fill_dev, keys_dev, stream=0, slot=0, init=False, grid=False,
                    cells=False):
        """Async (knn_index_list_within): every row of this shard whose v0 squared distance to query j is finite and <= max_dist2
        reserves place p = fill_dev[j]++ (uint32) and, when p is below the room of segment [offsets_dev[j], offsets_dev[j + 1])
        (uint64), stores its packed key at keys_dev[offsets_dev[j] + p]; init (KNN_QUERY_INIT_KEYS): fill_dev is zeroed first,
        else the call appends.  fill_dev[j] above the room: the segment overflowed (nothing was stored outside it).  grid /
        cells: as count_within.  The order within a segment is unspecified (keys_sort_segments)."""
        _check(list_within_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                               ctypes.c_void_p(int(offsets_dev)), ctypes.c_void_p(int(fill_dev)), ctypes.c_void_p(int(keys_dev)),
                               ctypes.c_void_p(stream),
                               (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) | (QUERY_COUNT_CELLS if cells else 0)))

    def list_within_host(self, queries, max_dist2):
        """Synchronous lists of this shard alone (knn_index_list_within_host): (offsets int64 [m + 1], indices int32 [total],
        dist2 float32 [total]); query j's rows, nearest first, are entries offsets[j] .. offsets[j + 1] - 1."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        offsets = np.empty(m + 1, dtype=np.int64)
        ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
        f = lib().knn_index_list_within_host
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                      ctypes.POINTER(ctypes.POINTER(ctypes.c_int)), ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]
        _check(f(self._h, m, q.ctypes.data_as(ctypes.c_void_p), float(max_dist2), offsets.ctypes.data_as(ctypes.c_void_p),
                 ctypes.byref(ind), ctypes.byref(d2)))
        total = int(offsets[m])
        free = ctypes.CDLL(None).free
        free.argtypes = [ctypes.c_void_p]
        try:
            indices = np.ctypeslib.as_array(ind, shape=(max(total, 1),))[:total].astype(np.int32, copy=True)
            dist2 = np.ctypeslib.as_array(d2, shape=(max(total, 1),))[:total].astype(np.float32, copy=True)
        finally:
            free(ind)
            free(d2)
        return offsets, indices, dist2

    def count_within_each(self, m, queries_dev, max_dist2_dev, counts_dev, cap=float("inf"), stream=0, slot=0, init=False,
                          grid=False, cells=False):
        """Async (knn_index_count_within_each): count_within with a radius per query — max_dist2_dev[m] (float32, on the device):
        a row counts for query j when its v0 squared distance is finite, <= max_dist2_dev[j] and <= cap.  A NaN or negative radius
        counts nothing.  cap (>= 0 or +INF): the caller's bound for the radii; the way is the scalar call's at max_dist2 = cap
        (cells needs a finite cap).  init, grid, cells: as count_within."""
        _check(count_within_each_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), ctypes.c_void_p(int(max_dist2_dev)),
                                     float(cap), ctypes.c_void_p(int(counts_dev)), ctypes.c_void_p(stream),
                                     (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) |
                                     (QUERY_COUNT_CELLS if cells else 0)))

    def list_within_each(self, m, queries_dev, max_dist2_dev, offsets_dev, fill_dev, keys_dev, cap=float("inf"), stream=0, slot=0,
                         init=False, grid=False, cells=False):
        """Async (knn_index_list_within_each): list_within with a radius per query, under count_within_each's rule.  The third
        step of count_within_each -> counts_to_offsets -> this -> keys_sort_segments."""
        _check(list_within_each_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), ctypes.c_void_p(int(max_dist2_dev)),
                                    float(cap), ctypes.c_void_p(int(offsets_dev)), ctypes.c_void_p(int(fill_dev)),
                                    ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream),
                                    (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) |
                                    (QUERY_COUNT_CELLS if cells else 0)))

    def count_within_each_host(self, queries, max_dist2, cap=float("inf")):
        """Synchronous count of this shard alone with a radius per query (max_dist2: float32 [m] on the host): uint32 [m]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        r = np.ascontiguousarray(max_dist2, dtype=np.float32).reshape(-1)
        if r.size != m:
            raise ValueError("max_dist2 must hold one radius per query")
        counts = np.empty(m, dtype=np.uint32)
        _check(count_within_each_host_c()(self._h, m, q.ctypes.data_as(ctypes.c_void_p), r.ctypes.data_as(ctypes.c_void_p), float(cap),
                                          counts.ctypes.data_as(ctypes.c_void_p)))
        return counts

    def list_within_each_host(self, queries, max_dist2, cap=float("inf")):
        """Synchronous lists of this shard alone with a radius per query (knn_index_list_within_each_host): what list_within_host
        returns — (offsets int64 [m + 1], indices int32 [total], dist2 float32 [total]), nearest first within a query."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        r = np.ascontiguousarray(max_dist2, dtype=np.float32).reshape(-1)
        if r.size != m:
            raise ValueError("max_dist2 must hold one radius per query")
        offsets = np.empty(m + 1, dtype=np.int64)
        ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
        _check(list_within_each_host_c()(self._h, m, q.ctypes.data_as(ctypes.c_void_p), r.ctypes.data_as(ctypes.c_void_p), float(cap),
                                         offsets.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ind), ctypes.byref(d2)))
        total = int(offsets[m])
        free = ctypes.CDLL(None).free
        free.argtypes = [ctypes.c_void_p]
        try:
            indices = np.ctypeslib.as_array(ind, shape=(max(total, 1),))[:total].astype(np.int32, copy=True)
            dist2 = np.ctypeslib.as_array(d2, shape=(max(total, 1),))[:total].astype(np.float32, copy=True)
        finally:
            free(ind)
            free(d2)
        return offsets, indices, dist2

    def query_topk_large(self, m, K, queries_dev, keys_dev, max_dist2=float("inf"), stream=0, slot=0, init_keys=False,
                         indices_dev=None, flags=0):
        """Async (knn_index_query_topk_large): query_topk_within for 1 <= K <= 4096 — keys_dev[m][K] <- the K smallest keys of
        (this shard's rows with a finite v0 squared distance <= max_dist2 and, unless init_keys, the K sorted keys per query
        keys_dev already holds, which are not clipped), sorted, padded with KEY_INIT.  One way on every index (last_stats()[0]
        == 1; [2] == 1: some query's cut fell inside a class of equal distances).  flags: further flag bits as they are (every
        one of them raises)."""
        _check(query_topk_large_c()(self._h, int(slot), int(m), int(K), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                                    ctypes.c_void_p(int(keys_dev)),
                                    ctypes.c_void_p(int(indices_dev)) if indices_dev is not None else None,
                                    ctypes.c_void_p(stream), (QUERY_INIT_KEYS if init_keys else 0) | int(flags)))

    def query_topk_large_host(self, queries, K, max_dist2=float("inf")):
        """Synchronous large top-K of this shard alone: (indices int32 [m][K], dist2 float32 [m][K] with +INF in padding, counts
        int32 [m]: the entries of each list that are not padding)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        idx = np.empty((m, int(K)), dtype=np.int32)
        d2 = np.empty((m, int(K)), dtype=np.float32)
        counts = np.empty(m, dtype=np.int32)
        _check(query_topk_large_host_c()(self._h, m, int(K), q.ctypes.data_as(ctypes.c_void_p), float(max_dist2),
                                         idx.ctypes.data_as(ctypes.c_void_p), d2.ctypes.data_as(ctypes.c_void_p),
                                         counts.ctypes.data_as(ctypes.c_void_p)))
        return idx, d2, counts

    def query_topk_masked(self, m, K, queries_dev, mask_dev, keys_dev, max_dist2=float("inf"), stream=0, slot=0, init_keys=False,
                          indices_dev=None, flags=0):
        """Async (knn_index_query_topk_masked): query_topk_within over the rows the mask admits — keys_dev[m][K] <- the K smallest
        keys of (this shard's rows whose bit is set in mask_dev (uint32 [mask_words(n)], bit i % 32 of word i // 32 = local row i)
        and whose v0 squared distance is finite and <= max_dist2 and, unless init_keys, the K sorted keys per query keys_dev already
        holds, which are not clipped), sorted, padded with KEY_INIT; keys carry the original global numbers.  1 <= K <= 64.  One way
        on every index (last_stats() == [1, 0, 0, 0]).  flags: further flag bits as they are (every one of them raises)."""
        _check(query_topk_masked_c()(self._h, int(slot), int(m), int(K), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                                     ctypes.c_void_p(int(mask_dev)), ctypes.c_void_p(int(keys_dev)),
                                     ctypes.c_void_p(int(indices_dev)) if indices_dev is not None else None,
                                     ctypes.c_void_p(stream), (QUERY_INIT_KEYS if init_keys else 0) | int(flags)))

    def count_within_masked(self, m, queries_dev, max_dist2, mask_dev, counts_dev, stream=0, slot=0, init=False, flags=0):
        """Async (knn_index_count_within_masked): counts_dev[m] (uint32) += the rows of this shard whose mask bit is set and whose
        v0 squared distance is finite and <= max_dist2; init (KNN_QUERY_INIT_KEYS): = instead of +=."""
        _check(count_within_masked_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                                       ctypes.c_void_p(int(mask_dev)), ctypes.c_void_p(int(counts_dev)), ctypes.c_void_p(stream),
                                       (QUERY_INIT_KEYS if init else 0) | int(flags)))

    def query_topk_masked_host(self, queries, K, mask, max_dist2=float("inf")):
        """Synchronous masked top-K of this shard alone, mask: the uint32 words on the host: (indices int32 [m][K], dist2 float32
        [m][K] with +INF in padding, counts int32 [m]: the entries of each list that are not padding)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
        if w.size != mask_words(self.n):
            raise ValueError("mask: expected %d words, got %d" % (mask_words(self.n), w.size))
        m = q.size // self.k
        idx = np.empty((m, int(K)), dtype=np.int32)
        d2 = np.empty((m, int(K)), dtype=np.float32)
        counts = np.empty(m, dtype=np.int32)
        wp = w.ctypes.data_as(ctypes.c_void_p) if w.size else (ctypes.c_uint * 1)()
        _check(query_topk_masked_host_c()(self._h, m, int(K), q.ctypes.data_as(ctypes.c_void_p), float(max_dist2), wp,
                                          idx.ctypes.data_as(ctypes.c_void_p), d2.ctypes.data_as(ctypes.c_void_p),
                                          counts.ctypes.data_as(ctypes.c_void_p)))
        return idx, d2, counts

    def list_within_masked(self, m, queries_dev, max_dist2, mask_dev, offsets_dev, fill_dev, keys_dev, stream=0, slot=0, init=False,
                           flags=0):
        """Async (knn_index_list_within_masked): list_within over the rows the mask admits — every row of this shard whose bit is
        set in mask_dev (uint32 [mask_words(n)], bit i % 32 of word i // 32 = local row i) and whose v0 squared distance to query j
        is finite and <= max_dist2 reserves place p = fill_dev[j]++ and, when p is below the room of segment [offsets_dev[j],
        offsets_dev[j + 1]), stores its packed key at keys_dev[offsets_dev[j] + p]; init (KNN_QUERY_INIT_KEYS): fill_dev is zeroed
        first, else the call appends.  The third step of count_within_masked -> counts_to_offsets -> this -> keys_sort_segments.
        flags: further flag bits as they are (every one of them raises)."""
        _check(list_within_masked_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                                      ctypes.c_void_p(int(mask_dev)), ctypes.c_void_p(int(offsets_dev)),
                                      ctypes.c_void_p(int(fill_dev)), ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream),
                                      (QUERY_INIT_KEYS if init else 0) | int(flags)))

    def list_within_masked_host(self, queries, max_dist2, mask):
        """Synchronous masked lists of this shard alone (knn_index_list_within_masked_host), mask: the uint32 words on the host:
        (offsets int64 [m + 1], indices int32 [total], dist2 float32 [total]); query j's admitted rows, nearest first, are entries
        offsets[j] .. offsets[j + 1] - 1."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
        if w.size != mask_words(self.n):
            raise ValueError("mask: expected %d words, got %d" % (mask_words(self.n), w.size))
        m = q.size // self.k
        offsets = np.empty(m + 1, dtype=np.int64)
        ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
        wp = w.ctypes.data_as(ctypes.c_void_p) if w.size else ctypes.cast((ctypes.c_uint * 1)(), ctypes.c_void_p)
        _check(list_within_masked_host_c()(self._h, m, q.ctypes.data_as(ctypes.c_void_p), float(max_dist2), wp,
                                           offsets.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ind), ctypes.byref(d2)))
        total = int(offsets[m])
        free = ctypes.CDLL(None).free
        free.argtypes = [ctypes.c_void_p]
        try:
            indices = np.ctypeslib.as_array(ind, shape=(max(total, 1),))[:total].astype(np.int32, copy=True)
            dist2 = np.ctypeslib.as_array(d2, shape=(max(total, 1),))[:total].astype(np.float32, copy=True)
        finally:
            free(ind)
            free(d2)
        return offsets, indices, dist2

    def query_topk_large_masked(self, m, K, queries_dev, mask_dev, keys_dev, max_dist2=float("inf"), stream=0, slot=0,
                                init_keys=False, indices_dev=None, flags=0):
        """Async (knn_index_query_topk_large_masked): query_topk_large over the rows the mask admits, 1 <= K <= 4096 —
        keys_dev[m][K] <- the K smallest keys of (this shard's rows whose mask bit is set and whose v0 squared distance is finite
        and <= max_dist2 and, unless init_keys, the K sorted keys per query keys_dev already holds, which are not clipped), sorted,
        padded with KEY_INIT; keys carry the original global numbers.  One way on every index (last_stats()[0] == 1; [2] == 1: some
        query's cut fell inside a class of equal distances).  flags: further flag bits as they are (every one of them raises)."""
        _check(query_topk_large_masked_c()(self._h, int(slot), int(m), int(K), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                                           ctypes.c_void_p(int(mask_dev)), ctypes.c_void_p(int(keys_dev)),
                                           ctypes.c_void_p(int(indices_dev)) if indices_dev is not None else None,
                                           ctypes.c_void_p(stream), (QUERY_INIT_KEYS if init_keys else 0) | int(flags)))

    def query_topk_large_masked_host(self, queries, K, mask, max_dist2=float("inf")):
        """Synchronous masked large top-K of this shard alone, mask: the uint32 words on the host: (indices int32 [m][K], dist2
        float32 [m][K] with +INF in padding, counts int32 [m]: the entries of each list that are not padding)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(mask, dtype=np.uint32).reshape(-1)
        if w.size != mask_words(self.n):
            raise ValueError("mask: expected %d words, got %d" % (mask_words(self.n), w.size))
        m = q.size // self.k
        idx = np.empty((m, int(K)), dtype=np.int32)
        d2 = np.empty((m, int(K)), dtype=np.float32)
        counts = np.empty(m, dtype=np.int32)
        wp = w.ctypes.data_as(ctypes.c_void_p) if w.size else ctypes.cast((ctypes.c_uint * 1)(), ctypes.c_void_p)
        _check(query_topk_large_masked_host_c()(self._h, m, int(K), q.ctypes.data_as(ctypes.c_void_p), float(max_dist2), wp,
                                                idx.ctypes.data_as(ctypes.c_void_p), d2.ctypes.data_as(ctypes.c_void_p),
                                                counts.ctypes.data_as(ctypes.c_void_p)))
        return idx, d2, counts

    def self_topk(self, row_first, rows, K, keys_dev, max_dist2=float("inf"), stream=0, slot=0, init_keys=False, indices_dev=None,
                  grid=False, frames=False, flags=0):
        """Async (knn_index_self_topk): the K nearest OTHER rows of the local rows row_first .. row_first + rows - 1 —
        keys_dev[rows][K] <- the K smallest keys of (this shard's rows but the query's own, with a finite v0 squared distance <=
        max_dist2, and, unless init_keys, the K sorted keys per row keys_dev already holds, which are not clipped), sorted, padded
        with KEY_INIT.  1 <= K <= 64.  The way is the plain top-K's for K + 1 (grid / frames as query_topk; last_stats() reports
        it); the exact self-scan where that is the exact scan and for K = 64.  flags: further flag bits as they are."""
        _check(self_topk_c()(self._h, int(slot), int(row_first), int(rows), int(K), float(max_dist2), ctypes.c_void_p(int(keys_dev)),
                             ctypes.c_void_p(int(indices_dev)) if indices_dev is not None else None, ctypes.c_void_p(stream),
                             (QUERY_INIT_KEYS if init_keys else 0) | (QUERY_TOPK_GRID if grid else 0) |
                             (QUERY_TOPK_FRAMES if frames else 0) | int(flags)))

    def self_count_within(self, row_first, rows, max_dist2, counts_dev, stream=0, slot=0, init=False, flags=0):
        """Async (knn_index_self_count_within): counts_dev[rows] (uint32) += the OTHER rows of this shard whose v0 squared distance
        to local row row_first + j is finite and <= max_dist2; init: = instead of +=.  flags: further flag bits as they are
        (every one of them raises)."""
        _check(self_count_within_c()(self._h, int(slot), int(row_first), int(rows), float(max_dist2), ctypes.c_void_p(int(counts_dev)),
                                     ctypes.c_void_p(stream), (QUERY_INIT_KEYS if init else 0) | int(flags)))

    def self_list_within(self, row_first, rows, max_dist2, offsets_dev, fill_dev, keys_dev, stream=0, slot=0, init=False, flags=0):
        """Async (knn_index_self_list_within): list_within for the queries that are the local rows row_first .. row_first + rows - 1,
        each without itself.  The third step of self_count_within -> counts_to_offsets -> this -> keys_sort_segments."""
        _check(self_list_within_c()(self._h, int(slot), int(row_first), int(rows), float(max_dist2), ctypes.c_void_p(int(offsets_dev)),
                                    ctypes.c_void_p(int(fill_dev)), ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream),
                                    (QUERY_INIT_KEYS if init else 0) | int(flags)))

    def self_topk_host(self, K, max_dist2=float("inf")):
        """Synchronous kNN graph of this shard (knn_index_self_topk_host): (indices int32 [n][K], dist2 float32 [n][K] with +INF in
        padding, counts int32 [n]: the entries of each list that are not padding)."""
        n = int(self.n)
        idx = np.empty((n, int(K)), dtype=np.int32)
        d2 = np.empty((n, int(K)), dtype=np.float32)
        counts = np.empty(n, dtype=np.int32)
        _check(self_topk_host_c()(self._h, int(K), float(max_dist2), idx.ctypes.data_as(ctypes.c_void_p),
                                  d2.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p)))
        return idx, d2, counts

    def self_count_within_each(self, row_first, rows, max_dist2_dev, counts_dev, cap=float("inf"), stream=0, slot=0, init=False,
                               flags=0):
        """Async (knn_index_self_count_within_each): self_count_within with a radius per row — max_dist2_dev[j] (float32, on the
        device) belongs to local row row_first + j; another row counts when its v0 squared distance is finite, <= that radius and
        <= cap.  A NaN or negative radius counts nothing."""
        _check(self_count_within_each_c()(self._h, int(slot), int(row_first), int(rows), ctypes.c_void_p(int(max_dist2_dev)), float(cap),
                                          ctypes.c_void_p(int(counts_dev)), ctypes.c_void_p(stream),
                                          (QUERY_INIT_KEYS if init else 0) | int(flags)))

    def self_list_within_each(self, row_first, rows, max_dist2_dev, offsets_dev, fill_dev, keys_dev, cap=float("inf"), stream=0,
                              slot=0, init=False, flags=0):
        """Async (knn_index_self_list_within_each): self_list_within under self_count_within_each's rule.  The third step of
        self_count_within_each -> counts_to_offsets -> this -> keys_sort_segments."""
        _check(self_list_within_each_c()(self._h, int(slot), int(row_first), int(rows), ctypes.c_void_p(int(max_dist2_dev)), float(cap),
                                         ctypes.c_void_p(int(offsets_dev)), ctypes.c_void_p(int(fill_dev)),
                                         ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream),
                                         (QUERY_INIT_KEYS if init else 0) | int(flags)))

    def self_count_within_routed(self, row_first, rows, counts_dev, cap=float("inf"), max_dist2_dev=None, stream=0, slot=0, init=False,
                                 grid=False, cells=False, flags=0):
        """Async (knn_index_self_count_within_routed): self_count_within (max_dist2_dev None: every row's radius is cap) or
        self_count_within_each (max_dist2_dev: float32 on the device, a radius per row, under cap) on the way count_within would
        take for `rows` queries at cap: grid / cells ask for the grid index / the cell-pruned scan (QUERY_COUNT_GRID /
        QUERY_COUNT_CELLS); without them the exact self-scan.  flags: further flag bits as they are (every one of them raises)."""
        _check(self_count_within_routed_c()(self._h, int(slot), int(row_first), int(rows),
                                            ctypes.c_void_p(int(max_dist2_dev)) if max_dist2_dev is not None else None, float(cap),
                                            ctypes.c_void_p(int(counts_dev)), ctypes.c_void_p(stream),
                                            (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) |
                                            (QUERY_COUNT_CELLS if cells else 0) | int(flags)))

    def self_list_within_routed(self, row_first, rows, offsets_dev, fill_dev, keys_dev, cap=float("inf"), max_dist2_dev=None, stream=0,
                                slot=0, init=False, grid=False, cells=False, flags=0):
        """Async (knn_index_self_list_within_routed): self_list_within / self_list_within_each on self_count_within_routed's way.
        The third step of self_count_within_routed -> counts_to_offsets -> this -> keys_sort_segments."""
        _check(self_list_within_routed_c()(self._h, int(slot), int(row_first), int(rows),
                                           ctypes.c_void_p(int(max_dist2_dev)) if max_dist2_dev is not None else None, float(cap),
                                           ctypes.c_void_p(int(offsets_dev)), ctypes.c_void_p(int(fill_dev)),
                                           ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream),
                                           (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) |
                                           (QUERY_COUNT_CELLS if cells else 0) | int(flags)))

    def count_within_masked_routed(self, m, queries_dev, max_dist2, mask_dev, counts_dev, stream=0, slot=0, init=False, grid=False,
                                   cells=False, flags=0):
        """Async (knn_index_count_within_masked_routed): count_within_masked on the way count_within would take for m queries at
        max_dist2: grid / cells ask for the grid index / the cell-pruned scan (QUERY_COUNT_GRID / QUERY_COUNT_CELLS); without them
        the exact masked scan.  flags: further flag bits as they are (every one of them raises)."""
        _check(count_within_masked_routed_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                                              ctypes.c_void_p(int(mask_dev)), ctypes.c_void_p(int(counts_dev)), ctypes.c_void_p(stream),
                                              (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) |
                                              (QUERY_COUNT_CELLS if cells else 0) | int(flags)))

    def list_within_masked_routed(self, m, queries_dev, max_dist2, mask_dev, offsets_dev, fill_dev, keys_dev, stream=0, slot=0,
                                  init=False, grid=False, cells=False, flags=0):
        """Async (knn_index_list_within_masked_routed): list_within_masked on count_within_masked_routed's way.  The third step of
        count_within_masked_routed -> counts_to_offsets -> this -> keys_sort_segments."""
        _check(list_within_masked_routed_c()(self._h, int(slot), int(m), ctypes.c_void_p(int(queries_dev)), float(max_dist2),
                                             ctypes.c_void_p(int(mask_dev)), ctypes.c_void_p(int(offsets_dev)),
                                             ctypes.c_void_p(int(fill_dev)), ctypes.c_void_p(int(keys_dev)), ctypes.c_void_p(stream),
                                             (QUERY_INIT_KEYS if init else 0) | (QUERY_COUNT_GRID if grid else 0) |
                                             (QUERY_COUNT_CELLS if cells else 0) | int(flags)))

    def self_cluster_within(self, max_dist2, min_pts, labels_dev, core_dev=None, stream=0, slot=0, grid=False, flags=0):
        """Async (knn_index_self_cluster_within): density clusters (DBSCAN) of this shard's rows on the radius graph.  labels_dev:
        int32 [n] on the device — LOCAL row numbers: a core row's is the smallest core row of its component, a border row's its
        nearest core row's, CLUSTER_NOISE for the rest; core_dev: None, or (n + 31) // 32 uint32 words that receive the core rows
        as a mask for the masked calls.  grid asks for the grid index (QUERY_COUNT_GRID); without it the exact self-scan.
        flags: further flag bits as they are (every one of them raises)."""
        _check(self_cluster_within_c()(self._h, int(slot), float(max_dist2), int(min_pts), ctypes.c_void_p(int(labels_dev)),
                                       ctypes.c_void_p(int(core_dev)) if core_dev is not None else None, ctypes.c_void_p(stream),
                                       (QUERY_COUNT_GRID if grid else 0) | int(flags)))

    def self_cluster_within_host(self, max_dist2, min_pts, grid=False, flags=0):
        """Synchronous (knn_index_self_cluster_within_host): (labels int32 [n] — clusters 0 .. C - 1 in ascending order of their
        smallest core row, -1 noise —, core bool [n], info dict(clusters, core, border, noise))."""
        n = int(self.n)
        labels = np.empty(n, dtype=np.int32)
        core = np.zeros(n, dtype=np.uint8)
        info = (ctypes.c_longlong * 4)()
        _check(self_cluster_within_host_c()(self._h, float(max_dist2), int(min_pts), (QUERY_COUNT_GRID if grid else 0) | int(flags),
                                            labels.ctypes.data_as(ctypes.c_void_p), core.ctypes.data_as(ctypes.c_void_p), info))
        return labels, core.astype(bool), dict(zip(("clusters", "core", "border", "noise"), list(info)))

    def self_cluster_within_routed(self, max_dist2, min_pts, labels_dev, core_dev=None, slot=0, stream=0, grid=False, cells=False,
                                   flags=0):
        """Async (knn_index_self_cluster_within_routed): self_cluster_within's answer, bit for bit, on the way the routed self count
        takes for the shard's rows at cap = max_dist2 — grid asks for the grid index (QUERY_COUNT_GRID), cells for the cell-pruned
        scan (QUERY_COUNT_CELLS), without either the exact self-scan.  flags: further flag bits as they are (every one raises)."""
        _check(self_cluster_within_routed_c()(self._h, int(slot), float(max_dist2), int(min_pts), ctypes.c_void_p(int(labels_dev)),
                                              ctypes.c_void_p(int(core_dev)) if core_dev is not None else None,
                                              ctypes.c_void_p(stream),
                                              (QUERY_COUNT_GRID if grid else 0) | (QUERY_COUNT_CELLS if cells else 0) | int(flags)))

    def self_cluster_within_routed_host(self, max_dist2, min_pts, grid=False, cells=False, flags=0):
        """Synchronous (knn_index_self_cluster_within_routed_host): self_cluster_within_host's (labels, core, info) on the routed ways."""
        n = int(self.n)
        labels = np.empty(n, dtype=np.int32)
        core = np.zeros(n, dtype=np.uint8)
        info = (ctypes.c_longlong * 4)()
        _check(self_cluster_within_routed_host_c()(self._h, float(max_dist2), int(min_pts),
                                                   (QUERY_COUNT_GRID if grid else 0) | (QUERY_COUNT_CELLS if cells else 0) | int(flags),
                                                   labels.ctypes.data_as(ctypes.c_void_p), core.ctypes.data_as(ctypes.c_void_p), info))
        return labels, core.astype(bool), dict(zip(("clusters", "core", "border", "noise"), list(info)))

    def self_forest_within(self, max_dist2, labels_dev, edge_keys_dev, edge_hi_dev, count_dev, stream=0, slot=0, grid=False, flags=0):
        """Async (knn_index_self_forest_within): the minimum spanning forest of this shard's rows on the radius graph (max_dist2
        may be inf: the spanning tree).  labels_dev: int32 [n], the smallest LOCAL row of every row's component; edge e <
        count_dev[0] is edge_keys_dev[e] = (distance bits << 32 | i), edge_hi_dev[e] = j, i < j, in no particular order
        (uint64 [n], uint32 [n]); count_dev: uint32 [2] = edges, rounds that added one.  grid asks for the grid index
        (QUERY_COUNT_GRID); without it the exact self-scan.  flags: further flag bits as they are (every one of them raises)."""
        _check(self_forest_within_c()(self._h, int(slot), float(max_dist2), ctypes.c_void_p(int(labels_dev)),
                                      ctypes.c_void_p(int(edge_keys_dev)), ctypes.c_void_p(int(edge_hi_dev)),
                                      ctypes.c_void_p(int(count_dev)), ctypes.c_void_p(stream),
                                      (QUERY_COUNT_GRID if grid else 0) | int(flags)))

    def self_forest_within_host(self, max_dist2, grid=False, flags=0, want_labels=True, want_dist2=True):
        """Synchronous (knn_index_self_forest_within_host): (labels int32 [n] or None, lo int32 [edges], hi int32 [edges], dist2
        float32 [edges] or None, info dict(edges, components, rounds, gave_up)), the edges sorted ascending by (distance, lo, hi):
        the order single linkage merges in."""
        n = int(self.n)
        labels = np.empty(n, dtype=np.int32) if want_labels else None
        lo = np.empty(n, dtype=np.int32)
        hi = np.empty(n, dtype=np.int32)
        dist2 = np.empty(n, dtype=np.float32) if want_dist2 else None
        info = (ctypes.c_longlong * 4)()
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
        _check(self_forest_within_host_c()(self._h, float(max_dist2), (QUERY_COUNT_GRID if grid else 0) | int(flags), ptr(labels),
                                           ptr(lo), ptr(hi), ptr(dist2), info))
        e = int(info[0])
        return (labels, lo[:e].copy(), hi[:e].copy(), dist2[:e].copy() if want_dist2 else None,
                dict(zip(("edges", "components", "rounds", "gave_up"), list(info))))

    def self_list_within_routed_host(self, cap, max_dist2=None, grid=False, cells=False, flags=0):
        """Synchronous radius graph of this shard on the routed self calls (knn_index_self_list_within_routed_host), in
        self_list_within_host's CSR form.  max_dist2: None, or a radius per row (float32 [n]) under cap."""
        n = int(self.n)
        offsets = np.empty(n + 1, dtype=np.int64)
        rad = None if max_dist2 is None else np.ascontiguousarray(max_dist2, dtype=np.float32).reshape(-1)
        if rad is not None and rad.size != n:
            raise ValueError("max_dist2 must hold one radius per row of the shard")
        ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
        _check(self_list_within_routed_host_c()(self._h, rad.ctypes.data_as(ctypes.c_void_p) if rad is not None else None, float(cap),
                                                (QUERY_COUNT_GRID if grid else 0) | (QUERY_COUNT_CELLS if cells else 0) | int(flags),
                                                offsets.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ind), ctypes.byref(d2)))
        total = int(offsets[n])
        free = ctypes.CDLL(None).free
        free.argtypes = [ctypes.c_void_p]
        try:
            indices = np.ctypeslib.as_array(ind, shape=(max(total, 1),))[:total].astype(np.int32, copy=True)
            dist2 = np.ctypeslib.as_array(d2, shape=(max(total, 1),))[:total].astype(np.float32, copy=True)
        finally:
            free(ind)
            free(d2)
        return offsets, indices, dist2

    def self_list_within_host(self, max_dist2):
        """Synchronous radius graph of this shard (knn_index_self_list_within_host) in CSR form: (offsets int64 [n + 1], indices
        int32 [total], dist2 float32 [total]); row j's neighbours, nearest first, are entries offsets[j] .. offsets[j + 1] - 1."""
        n = int(self.n)
        offsets = np.empty(n + 1, dtype=np.int64)
        ind, d2 = ctypes.POINTER(ctypes.c_int)(), ctypes.POINTER(ctypes.c_float)()
        _check(self_list_within_host_c()(self._h, float(max_dist2), offsets.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ind),
                                         ctypes.byref(d2)))
        total = int(offsets[n])
        free = ctypes.CDLL(None).free
        free.argtypes = [ctypes.c_void_p]
        try:
            indices = np.ctypeslib.as_array(ind, shape=(max(total, 1),))[:total].astype(np.int32, copy=True)
            dist2 = np.ctypeslib.as_array(d2, shape=(max(total, 1),))[:total].astype(np.float32, copy=True)
        finally:
            free(ind)
            free(d2)
        return offsets, indices, dist2

    def query_topk_host(self, queries, K):
        """Synchronous top-K of this shard alone: (indices int32 [m][K], dist2 float32 [m][K])."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1)
        m = q.size // self.k
        idx = np.empty((m, int(K)), dtype=np.int32)
        d2 = np.empty((m, int(K)), dtype=np.float32)
        _check(lib().knn_index_query_topk_host(self._h, m, int(K), q.ctypes.data_as(ctypes.c_void_p),
                                               idx.ctypes.data_as(ctypes.c_void_p), d2.ctypes.data_as(ctypes.c_void_p)))
        return idx, d2

    def last_stats(self):
        st = (ctypes.c_longlong * 4)()
        _check(lib().knn_index_last_stats(self._h, st))
        return list(st)

    def debug_counters(self):
        """[seed cells empty, dense cells, cells, rows of the largest cell] of the last cell-pruned batch."""
        out = (ctypes.c_longlong * 4)()
        f = lib().knn_index_debug_counters
        f.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
        _check(f(self._h, out))
        return list(out)

    def debug_cells_fetch(self, m, slot=0, tables=False):
        """Test hook (knn_debug_cells_fetch): what the match launch of the last cell-pruned batch of m queries on `slot` wrote —
        dict(ncells, cap, nl, nh, cell_base, counts[ncells], lists[ncells][cap]: the first min(count, cap) entries of a row are
        the cell's queries) and, with tables, what it read: lo[m_padded][nl], hi[nh][m_padded], lo_min[nl / 64][m_padded],
        dup[m_padded].  Waits for the device."""
        import numpy as np
        f = lib().knn_debug_cells_fetch
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
        dims = (ctypes.c_longlong * 6)()
        _check(f(self._h, int(slot), 0, None, 0, dims))
        ncells, cap, nl, nh, m_cap, cell_base = (int(v) for v in dims)
        mp = (int(m) + 31) // 32 * 32
        if mp > m_cap:
            raise ValueError("debug_cells_fetch: the slot's tables are smaller than m")

        def fetch(what, dtype, shape):
            a = np.empty(shape, dtype=dtype)
            _check(f(self._h, int(slot), what, a.ctypes.data, a.nbytes, dims))
            return a
        out = dict(ncells=ncells, cap=cap, nl=nl, nh=nh, cell_base=cell_base, counts=fetch(1, np.uint32, (ncells,)),
                   lists=fetch(2, np.uint16, (ncells, cap)))
        if tables:
            out.update(lo=fetch(3, np.float32, (mp, nl)), hi=fetch(4, np.float32, (nh, mp)), lo_min=fetch(5, np.float32, (nl // 64, mp)),
                       dup=fetch(6, np.float32, (mp,)))
        return out

    def debug_filter_scores(self, m, queries_dev, scores_dev, qnorm_dev):
        """Test hook (knn_debug_filter_scores): returns the 8 bound constants."""
        consts = (ctypes.c_double * 8)()
        _check(lib().knn_debug_filter_scores(self._h, int(m), ctypes.c_void_p(int(queries_dev)),
                                             ctypes.c_void_p(int(scores_dev)), ctypes.c_void_p(int(qnorm_dev)),
                                             consts))
        return list(consts)

    def timing(self, enable):
        """True / N > 0: bracket every (N-th) dominant-kernel launch with HIP events; False / 0: stop."""
        _check(lib().knn_index_timing(self._h, int(enable)))

    def timing_read(self):
        """(launches, total_ms) of the dominant kernel since timing(True) / the last read."""
        n, ms = ctypes.c_int(), ctypes.c_double()
        _check(lib().knn_index_timing_read(self._h, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def close(self):
        if self._h:
            lib().knn_index_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._keep = self._layer = None   # (the borrowed buffers may go now)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def keys_init(keys_dev, m, device=0, stream=0):
    _check(lib().knn_keys_init(int(device), ctypes.c_void_p(int(keys_dev)), int(m), ctypes.c_void_p(stream)))


def keys_to_indices(keys_dev, m, out_dev, device=0, stream=0):
    _check(lib().knn_keys_to_indices(int(device), ctypes.c_void_p(int(keys_dev)), int(m),
                                     ctypes.c_void_p(int(out_dev)), ctypes.c_void_p(stream)))


def keys_topk_merge(a_dev, b_dev, m, K, device=0, stream=0):
    """b[j] <- the K smallest of a[j] and b[j] (device arrays of m sorted lists of K keys; knn_keys_topk_merge)."""
    _check(lib().knn_keys_topk_merge(int(device), int(m), int(K), ctypes.c_void_p(int(a_dev)), ctypes.c_void_p(int(b_dev)),
                                     ctypes.c_void_p(stream)))


def keys_allreduce_min(devices, keys_dev, m, streams=None):
    """RCCL min-reduction of one key array per GPU of this process (knn_keys_allreduce_min)."""
    n = len(devices)
    devs = (ctypes.c_int * n)(*[int(d) for d in devices])
    ptrs = (ctypes.c_void_p * n)(*[int(p) for p in keys_dev])
    strs = (ctypes.c_void_p * n)(*[int(s) for s in streams]) if streams is not None else None
    f = lib().knn_keys_allreduce_min
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p), ctypes.c_int,
                  ctypes.POINTER(ctypes.c_void_p)]
    _check(f(n, devs, ptrs, int(m), strs))


def synth_fill_device(dst_dev, count, seed, first=0, device=0, stream=0):
    _check(lib().knn_synth_fill_device(int(device), ctypes.c_void_p(int(dst_dev)), int(count), int(seed),
                                       int(first), ctypes.c_void_p(stream)))
