"""The one argument ladder of the top-K forms (knn_api.cpp: topk_check) without a GPU: the eight entries that answer one message per
rule — knn_index_query_topk_large, _masked, _large_masked, knn_index_self_topk and their four *_host calls — replayed against
tests/golden/topk_arg_errors.json, the table tools/arg_error_table.py recorded from the commit BEFORE the entries were moved onto
the ladder (their rules then spelled out entry by entry).  Every call names a NULL index, so nothing behind the rules is reached:
one call with everything valid, one per broken rule, one per pair of broken rules.  Equality case by case: the code, the text
byte for byte — the entry's name in front —, and with two rules broken the rule that spoke then is the rule that speaks now
(knn_index_query_topk_large and its host call look at K, m and m * K first, the others at radius, flags and slot first).
The range rule of knn_index_self_topk needs an index: tests/test_self_logic.py and tests/test_self_gpu.py hold it."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("knn_index_query_topk_large", "knn_index_query_topk_large_host", "knn_index_query_topk_masked",
           "knn_index_query_topk_masked_host", "knn_index_query_topk_large_masked", "knn_index_query_topk_large_masked_host",
           "knn_index_self_topk", "knn_index_self_topk_host")


def _tool():
    spec = importlib.util.spec_from_file_location("arg_error_table", os.path.join(ROOT, "tools", "arg_error_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(os.path.join(ROOT, "tests", "golden", "topk_arg_errors.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_table_holds_every_entry_rule_and_pair():
    """The golden table is the one the tool would ask for today: the same calls in the same order, none dropped."""
    assert [(g["entry"], g["broken"]) for g in GOLDEN] == [(name, broken) for name, _, broken, _ in TOOL.cases()]
    assert tuple(dict.fromkeys(g["entry"] for g in GOLDEN)) == ENTRIES
    for name, _, _, _, rules in TOOL.entries():
        singles = [g for g in GOLDEN if g["entry"] == name and len(g["broken"]) == 1]
        pairs = [g for g in GOLDEN if g["entry"] == name and len(g["broken"]) == 2]
        assert [g["broken"][0] for g in singles] == list(rules)
        # (all pairs but m with m * K and K with m * K, which contend for one argument)
        assert len(pairs) == len(rules) * (len(rules) - 1) // 2 - (2 if "mK" in rules else 0)
        assert all(g["code"] == -1 and g["text"].startswith(name + ": ") for g in singles + pairs)
        assert [g["text"] for g in GOLDEN if g["entry"] == name and not g["broken"]] == [name + ": null index"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_rule_and_every_pair_of_rules_answers_as_before_the_ladder(entry):
    got = {(r["entry"], tuple(r["broken"])): (r["code"], r["text"]) for r in TOOL.table() if r["entry"] == entry}
    want = {(g["entry"], tuple(g["broken"])): (g["code"], g["text"]) for g in GOLDEN if g["entry"] == entry}
    assert want and got.keys() == want.keys()
    for case in want:
        assert got[case] == want[case], case
