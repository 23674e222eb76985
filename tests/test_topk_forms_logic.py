"""The cases of tests/test_topk_forms_gpu.py against the plan (knn_filter_query_plan through knn_debug_filter_query_plan), on the
CPU: each listed (k, m) really plans the compiled form its name says, with the options a top-K call hands the plan — so a later
change of the plan's thresholds cannot silently move a case to another form — and the cases, with the dense-filter layouts of
tests/test_topk_gpu.py, cover every form a top-K call can reach for k <= 640."""
import pytest

import multicore_hw2_amd as pkg
from tests.test_topk_gpu import LAYOUTS
from tests.topk_forms import CHUNKED, FALLS_BACK_BY_DESIGN, FORMS, KS_FORMS, N_FORMS, PIECES, TILED, kt_of

NUM_CU = 256   # MI355X


def existing_dense_layouts():
    """(k, m, n) of tests/test_topk_gpu.py's layouts on the dense filter (`cells` 2), with that test's rule for m."""
    return [(k, 96 if k <= 32 else 40, n) for _, k, n, opts in LAYOUTS if opts.get("path") == 2 and opts.get("cells") == 2]


def topk_plan(k, m, K, n=N_FORMS):
    """The plan of a top-K call (query_topk in knn_api.cpp: running thresholds off, no sample stride, topk = K).  rec_cap is what a
    workspace holds, KNN_RECORD_CAPACITY, whatever the batch: debug_scan_plan only reports it."""
    rec_cap = pkg.debug_scan_plan(NUM_CU, 2, 100, m)["rec_cap"]
    assert rec_cap == pkg.debug_scan_plan(NUM_CU, 2, 100, 1)["rec_cap"] == 1 << 22
    return pkg.debug_filter_query_plan(kt=kt_of(k), ntiles=(n + 31) // 32, m=m, num_cu=NUM_CU, rec_cap=rec_cap, topk=K,
                                       filter_qt=0, filter_rounds=0, filter_chain=0, run_thresholds=2, sample_stride=0)


@pytest.mark.parametrize("name,k,m,kt,form", FORMS, ids=[c[0] for c in FORMS])
def test_each_case_plans_the_form_it_names(name, k, m, kt, form):
    assert kt_of(k) == kt
    for K in KS_FORMS:
        p = topk_plan(k, m, K)
        assert p["ok"] == 1 and p["form"] == form and p["kt"] == kt and p["topk"] == K, (name, K, p)
        assert p["thr_nb"] == 1 and p["scan_running"] == 0, (name, K, p)   # the K-th minimum feeds the thresholds, none running
        # the sample pass has at least K blocks (fewer with a real row raise FALLBACK), unless the pair is listed as by design
        assert (p["sample_blocks"] >= K) != ((name, K) in FALLS_BACK_BY_DESIGN), (name, K, p["sample_blocks"])
    if form == PIECES:
        assert [pc["qt"] for pc in topk_plan(k, m, 8)["pieces"]] == [4]


def existing_forms():
    """{(kt, form)} the existing layouts plan, the same at every K of tests/test_topk_gpu.py."""
    seen = set()
    for k, m, n in existing_dense_layouts():
        plans = [topk_plan(k, m, K, n=n) for K in (1, 2, 8, 17, 64)]
        assert all(p["ok"] == 1 and p["kt"] == kt_of(k) and p["form"] == plans[0]["form"] for p in plans), (k, m, n)
        seen.add((kt_of(k), plans[0]["form"]))
    return seen


def test_the_existing_layouts_plan_the_forms_the_coverage_counts_on():
    """kt 1 and 2 (pieces), kt 8 as register pieces (k 128, m 40 — no case of FORMS has that form) and the chunked scan."""
    assert sorted(k for k, _, _ in existing_dense_layouts()) == [3, 16, 32, 128, 600]
    assert existing_forms() == {(1, PIECES), (2, PIECES), (8, PIECES), (40, CHUNKED)}


def test_the_cases_cover_every_form_a_top_k_call_reaches_up_to_k_640():
    seen = {(kt, form) for _, _, _, kt, form in FORMS} | existing_forms()
    assert (8, PIECES) not in {(kt, form) for _, _, _, kt, form in FORMS}              # (that one is the existing filter_k128's)
    assert {kt for kt, _ in seen} == {kt_of(k) for k in range(1, 641)}                  # every value knn_kt_of returns
    assert {(4, PIECES), (4, TILED), (8, PIECES), (8, TILED)} <= seen                  # both forms where the batch size decides
    assert {(16, TILED), (32, TILED), (40, CHUNKED)} <= seen
    # the chunked scan: k 513 walks five chunks of 128 dimensions like k 600 (the existing layout: the same kt), but its last chunk
    # holds a single real dimension
    assert kt_of(513) == kt_of(600) == 40 and 513 % 128 == 1


def test_the_seam_between_pieces_and_tiled_is_where_the_cases_assume():
    for k in (64, 128):
        assert topk_plan(k, 480, 8)["form"] == PIECES and topk_plan(k, 481, 8)["form"] == TILED
