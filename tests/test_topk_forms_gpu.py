"""Top-K on every compiled form: one test per instantiation of the exact top-K scan (knn_exact_topk_kernel<KC, LIM>:
nine KC, plain and radius) and per form of the MFMA filter a top-K call can reach and tests/test_topk_gpu.py's layouts do not
(knn_filter_query_topk: kt 4 as register pieces, kt 4 and 8 LDS-tiled, kt 16, kt 32, chunked; kt 8 as register pieces is that
file's filter_k128), on the GPU against the numpy restatement of v0 (tests/topk_oracle.py) — clipped at
the radius (tests/within_helper.clip) for a radius call.  Bar: bit-exact keys, the way knn_index_last_stats names, and for the
filter forms no fallback where none is by design (a form whose batches always fall back shows the exact scan, not the form)."""
import numpy as np
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.test_within_exact_gpu import spread_queries
from tests.topk_forms import FALLS_BACK_BY_DESIGN, FORMS, KS_FORMS, M_DISTINCT, N_FORMS
from tests.topk_oracle import topk_keys
from tests.within_helper import clip, plain, radii, within

pytestmark = pytest.mark.gpu
OPTIONS = ("path", "cells")
# (k + 15) / 16 picks KNN_TOPK_SCAN(n): every n = 1 .. 8 with a full last chunk (k = 16 n) and a partial one, k = 129 KC 0
KS_EXACT = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128, 129)


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    for name in OPTIONS:
        pkg.set_option(name, 0)


@pytest.mark.parametrize("k", KS_EXACT)
def test_the_exact_scan_at_every_chunk_count_plain_and_within_a_radius(k):
    """n = 2500: three slices of the scan, the last one short; m = 70: one full wave of queries and six lanes of a second whose
    other lanes are clamped to the last query; a NaN row, a +INF row, and a row duplicated 1100 rows on — a tie across slices that
    query 3, which sits next to it, holds in its first two places."""
    rng = np.random.default_rng(7100 + k)
    n, m, base = 2500, 70, 13
    R = rng.random((n, k), dtype=np.float32)
    R[40, k // 2] = np.nan
    R[41, 0] = np.inf
    R[1700] = R[600]
    Q = spread_queries(rng, m, k, 1.5 if k <= 32 else 4.0)
    Q[3] = R[600]
    Q[3, 0] += np.float32(2.0 ** -20)
    want64 = topk_keys(Q, R, k, 64, base=base)
    assert (want64[3, :2] & np.uint64(0xFFFFFFFF)).tolist() == [base + 600, base + 1700] and want64[3, 0] >> np.uint64(32) == \
        want64[3, 1] >> np.uint64(32)
    pkg.set_option("path", 1)
    ix = pkg.KnnIndex(k, R, base_index=base)
    try:
        for K in (1, 5, 64):
            want = want64[:, :K]
            np.testing.assert_array_equal(plain(ix, Q, K), want, err_msg=f"k={k} K={K} plain")
            assert ix.last_stats()[0] == 1, ix.last_stats()
            for name, r2 in radii(want):
                got = within(ix, Q, K, r2)
                assert ix.last_stats()[0] == 1, ix.last_stats()
                np.testing.assert_array_equal(got, clip(want, r2), err_msg=f"k={k} K={K} {name} r2={r2}")
    finally:
        ix.close()


@pytest.mark.parametrize("name,k,m,kt,form", FORMS, ids=[c[0] for c in FORMS])
def test_the_filter_forms_answer_top_k_without_falling_back(name, k, m, kt, form):
    """Every K of KS_FORMS as a plain call and within one radius.  K = 1 and K = 8 must be answered by the form itself ([2] == 0,
    records re-ranked); a larger K may fall back only where tests/topk_forms.py lists the pair, with its reason.  The m = 512
    batches repeat 48 distinct queries (the oracle is computed for those)."""
    rng = np.random.default_rng(N_FORMS + k + m)
    base = 11
    R = rng.random((N_FORMS, k), dtype=np.float32)
    m0 = min(m, M_DISTINCT)
    Q0 = spread_queries(rng, m0, k, 0.6)
    rep = np.arange(m) % m0
    Q = Q0[rep]
    pkg.set_option("path", 2)
    pkg.set_option("cells", 2)
    ix = pkg.KnnIndex(k, R, base_index=base)
    try:
        want64 = topk_keys(Q0, np.asfortranarray(R), k, 64, base=base)   # (column-major: the oracle walks the dimensions)
        wrong = []
        for K in KS_FORMS:
            want = want64[:, :K]
            r2 = radii(want)[0][1]
            for call, exp in (("plain", want), ("within", clip(want, r2))):
                got = plain(ix, Q, K) if call == "plain" else within(ix, Q, K, r2)
                st = ix.last_stats()
                print(f"{name} K={K} {call}: last_stats {st}")
                np.testing.assert_array_equal(got, exp[rep], err_msg=f"{name} K={K} {call}")
                assert st[0] == 2, (name, K, call, st)
                by_design = (name, K) in FALLS_BACK_BY_DESIGN
                if not (st[2] != 0 if by_design else st[2] == 0 and st[1] > 0):
                    wrong.append((name, K, call, st))
        assert not wrong, f"fell back (or did not) against tests/topk_forms.py: {wrong}"
        assert all(K not in (1, 8) for _, K in FALLS_BACK_BY_DESIGN)
    finally:
        ix.close()
