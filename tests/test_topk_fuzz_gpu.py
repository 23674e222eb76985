"""tools/fuzz_topk.py in the suite: one seeded run per family of index (the exact top-K scan, the dense MFMA filter, the
cell-pruned scan, the grid index) on the GPU against the numpy restatement of v0 (tests/topk_oracle.py).  Bar: every call
bit-exact — keys and the indices unpacked from them — whatever way answered it, and at least half of a family's calls answered by
the family's own way without a fallback (else the run quietly tests the exact scan only)."""
import pytest
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.fuzz_topk_loader import load_fuzz

pytestmark = pytest.mark.gpu
fuzz = load_fuzz()


@pytest.fixture(autouse=True)
def _options():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield
    fuzz.reset_options()


@pytest.mark.parametrize("family", fuzz.FAMILIES)
def test_seeded_cases_are_bit_exact_and_mostly_on_the_familys_own_way(family):
    seed, count = fuzz.SUITE_RUNS[family]
    runner = fuzz.Runner()
    try:
        for case in fuzz.draw_run(seed, family, count)[1]:
            assert runner.run(case), case
    finally:
        runner.close()
    print(f"fuzz {family} (seed {seed}, {count} cases, two calls each): {runner.tally()}")
    assert 2 * runner.intended >= runner.calls, runner.tally()
