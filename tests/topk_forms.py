"""The dense filter's compiled forms as top-K calls reach them (test infrastructure): the (k, m) cases of
tests/test_topk_forms_gpu.py — the forms tests/test_topk_gpu.py's LAYOUTS leave out: kt 8 as register pieces is THAT file's
filter_k128, not a case here —, the form knn_filter_query_plan gives each — checked on the CPU by tests/test_topk_forms_logic.py —
and the (case, K) pairs that fall back to the exact top-K by design."""
PIECES, TILED, CHUNKED = 0, 1, 2     # FilterForm (knn_common.h)
N_FORMS = 66000                       # rows of every case's shard, as tests/test_topk_gpu.py's LAYOUTS
M_DISTINCT = 48                       # the m = 512 batches are 48 distinct queries tiled
KS_FORMS = (1, 8, 17, 64)


def kt_of(k):
    """knn_kt_of (knn_common.h) for k <= 4096."""
    return 1 if k <= 16 else 2 if k <= 32 else 4 if k <= 64 else 8 if k <= 128 else 16 if k <= 256 else 32 if k <= 512 else \
        8 * ((k + 127) // 128)


# (name, k, m, kt, form)
FORMS = [
    ("kt4_pieces_k33", 33, 40, 4, PIECES),
    ("kt4_pieces_k64", 64, 40, 4, PIECES),
    ("kt4_tiled_k64", 64, 512, 4, TILED),
    ("kt8_tiled_k128", 128, 512, 8, TILED),
    ("kt16_k129", 129, 33, 16, TILED),
    ("kt16_k256", 256, 33, 16, TILED),
    ("kt32_k257", 257, 33, 32, TILED),
    ("kt32_k512", 512, 33, 32, TILED),
    ("chunked_k513", 513, 33, 40, CHUNKED),
]
# (case name, K) -> the reason, for the pairs whose batch falls back to the exact top-K BY DESIGN on a shard of N_FORMS rows.  None
# today: every form's sample pass has at least 64 blocks with a real row at every K of KS_FORMS (tests/test_topk_forms_logic.py
# restates that from the plan), and on an MI355X no (case, K) of FORMS raised the fallback.  K = 1 and K = 8 may never be listed.
FALLS_BACK_BY_DESIGN = {}
