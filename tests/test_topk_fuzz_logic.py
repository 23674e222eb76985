"""The generator of tools/fuzz_topk.py alone, on the CPU: what it draws is reproducible, the K values at the list kernels' edges
are among each family's seeded run, and what it makes of every drawn case is a valid call — a radius that is >= 0 and not NaN,
held keys that are sorted and whose global numbers are disjoint from the shard's.  The radii and held keys are made here from a
3000-row prefix of each shard (ROWS_CAP), so what is checked is the range of radius_of() and of the fold's construction on every
drawn (kind, u, batch), not the very values the GPU run hands the library (those come from the full shard's lists; run_batch
asserts r2 >= 0 on each as it calls).  Nothing here loads the library."""
import numpy as np
import pytest

import multicore_hw2_amd as pkg
from tests.fuzz_topk_loader import load_fuzz
from tests.topk_oracle import KEY_INIT, keys_index

fuzz = load_fuzz()
ROWS_CAP = 3000


@pytest.fixture(autouse=True)
def _no_library(monkeypatch):
    def refuse():
        raise AssertionError("the generator must not load libknn_mi355x.so")
    monkeypatch.setattr(pkg, "lib", refuse)


@pytest.mark.parametrize("family", fuzz.FAMILIES)
def test_the_same_seed_gives_the_same_cases(family):
    seed, count = fuzz.SUITE_RUNS[family]
    assert fuzz.draw_run(seed, family, count) == fuzz.draw_run(seed, family, count)
    assert fuzz.draw_run(seed, family, count)[1] != fuzz.draw_run(seed + 1, family, count)[1]
    rng_a, rng_b = np.random.default_rng(5), np.random.default_rng(5)
    assert fuzz.one_case(rng_a, 0, family) == fuzz.one_case(rng_b, 0, family)


@pytest.mark.parametrize("family", fuzz.FAMILIES)
def test_the_drawn_cases_stay_inside_what_the_family_names(family):
    seed, count = fuzz.SUITE_RUNS[family]
    indexes, cases = fuzz.draw_run(seed, family, count)
    rows, dims, nidx = fuzz.SHAPES[family]
    assert len(indexes) == nidx and len(cases) == count
    for ix in indexes:
        assert ix["n"] in rows and ix["k"] in dims and ix["layout"] in fuzz.LAYOUTS
        assert ix["k"] <= 16 or ix["layout"] not in ("bins", "centred")
    Ks = [b["K"] for c in cases for b in c["batches"]]
    assert all(1 <= K <= 64 for K in Ks)
    assert 1 in Ks and 64 in Ks and {31, 32, 33} & set(Ks), sorted(set(Ks))
    for c in cases:
        first, second = c["batches"]
        assert first["slot"] == second["slot"] and first["slot"] in (0, 1) and first["data_seed"] != second["data_seed"]
        for b in c["batches"]:
            assert b["m"] in fuzz.MS or (family == "cells" and b["m"] == fuzz.M_TILED)
            assert b["grid"] <= (family == "grid") and b["frames"] <= (c["spec"]["layout"] == "centred")
    # the inputs that fall back by design are drawn with fixed probabilities that sum to a quarter at most
    assert fuzz.P_BY_DESIGN_KIND + fuzz.P_BAD_QUERY + fuzz.P_FAR_QUERY <= 0.25


@pytest.mark.parametrize("family", fuzz.FAMILIES)
def test_every_radius_and_every_fold_is_a_valid_call(family):
    seed, count = fuzz.SUITE_RUNS[family]
    indexes, cases = fuzz.draw_run(seed, family, count)
    rows = [fuzz.materialise_index(ix, rows_cap=ROWS_CAP) for ix in indexes]
    folds = radii = 0
    for c in cases:
        ix, R = c["spec"], rows[c["index"]]
        for b in c["batches"]:
            mat = fuzz.materialise_batch(ix, R, b)
            assert mat["Q"].shape == (mat["m0"], ix["k"]) and mat["expect"].shape == (mat["m0"], b["K"])
            assert (np.diff(mat["expect"].astype(object), axis=1) >= 0).all()
            if b["call"] == "within":
                radii += 1
                assert mat["r2"] >= 0.0 and not np.isnan(mat["r2"]) and np.float32(mat["r2"]) == mat["r2"], (c, mat["r2"])
            if b["fold"]:
                folds += 1
                held = mat["held"]
                assert (np.diff(held.astype(object), axis=1) >= 0).all()
                real = keys_index(held[held != KEY_INIT]).astype(np.int64) & 0xFFFFFFFF
                assert ((real < ix["base"]) | (real >= ix["base"] + ix["n"])).all(), c
                assert mat["held_base"] >= ix["base"] + ix["n"]
    assert radii and folds


def test_every_kind_of_radius_is_non_negative_on_lists_with_padding_and_zero_distances():
    want = np.full((3, 4), KEY_INIT, dtype=np.uint64)
    for kind in fuzz.RADII:
        assert fuzz.radius_of(kind, 0.5, want) == 0.0            # no finite distance at all
    want[0, :2] = [np.uint64(5), (np.uint64(np.float32(0.25).view(np.uint32)) << np.uint64(32)) | np.uint64(9)]   # distance 0 and 0.25
    for kind in fuzz.RADII:
        for u in (0.0, 0.3, 0.999999):
            r2 = fuzz.radius_of(kind, u, want)
            assert 0.0 <= r2 <= 0.25, (kind, u, r2)
    assert fuzz.radius_of("held", 0.9, want) == 0.25 and 0 < fuzz.radius_of("below", 0.9, want) < 0.25
    assert fuzz.radius_of("under_all", 0.9, want) == 0.0
