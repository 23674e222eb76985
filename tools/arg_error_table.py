#!/usr/bin/env python3
"""The argument rules of the eight top-K entries that answer one message per rule — knn_index_query_topk_large, _masked,
_large_masked, knn_index_self_topk and their four *_host calls (include/knn_mi355x.h 2f .. 2i) — as a table, for comparing two
builds of the library rule for rule and, where two rules are broken at once, for which of them speaks.

Every rule but the self entry's range rule is decided before the index is looked at, so the entries are called with a NULL index
and dummy pointers that nothing reads: no GPU is needed.  Per entry: one call with everything valid (it answers "null index"),
one per broken rule, and one per unordered pair of broken rules that do not contend for the same argument.  One breaking value
per rule: radius -1, the unadmitted flag bit 64, slot 8, m (rows) 0, row_first -1, K 0, m * K just above INT_MAX with K at the
form's limit, and every pointer argument null.

  python3 tools/arg_error_table.py [--out FILE]
prints (or writes) the table as JSON: [{"entry", "broken": [rule, ...], "code", "text"}, ...] in a fixed order.
KNN_MI355X_LIB names the build to ask (another commit's .so), as for tools/topk_launches.py;
tests/golden/topk_arg_errors.json is this table of the commit before the entries were moved onto one ladder, and
tests/test_topk_ladder_logic.py replays it against the library under test."""
import ctypes
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INT_MAX = 2**31 - 1
Q, MASK, KEYS, OUT = 0x1000, 0x2000, 0x3000, 0x4000   # dummies: a null index is refused before anything is read


def entries():
    """[(entry, accessor in the package, argument names in the C order, valid values, {rule: the values that break it})]."""
    out = []
    for name, kmax, masked in (("knn_index_query_topk_large", 4096, False), ("knn_index_query_topk_masked", 64, True),
                               ("knn_index_query_topk_large_masked", 4096, True)):
        K = 100 if kmax > 64 else 5
        args = ["slot", "m", "K", "queries", "max_dist2"] + (["mask"] if masked else []) + ["keys", "indices", "stream", "flags"]
        valid = dict(slot=0, m=7, K=K, queries=Q, max_dist2=1.0, mask=MASK, keys=KEYS, indices=None, stream=None, flags=1)
        rules = dict(radius=dict(max_dist2=-1.0), flags=dict(flags=1 | 64), slot=dict(slot=8), m=dict(m=0), K=dict(K=0),
                     mK=dict(m=INT_MAX // kmax + 1, K=kmax), null_queries=dict(queries=None), null_keys=dict(keys=None))
        if masked:
            rules["null_mask"] = dict(mask=None)
        out.append((name, name[len("knn_index_"):] + "_c", args, valid, rules))
        hargs = ["m", "K", "queries", "max_dist2"] + (["mask"] if masked else []) + ["indices", "dist2", "counts"]
        hvalid = dict(m=7, K=K, queries=Q, max_dist2=1.0, mask=MASK, indices=OUT, dist2=None, counts=None)
        hrules = dict(radius=dict(max_dist2=-1.0), m=dict(m=0), K=dict(K=0), mK=dict(m=INT_MAX // kmax + 1, K=kmax),
                      null_queries=dict(queries=None), null_indices=dict(indices=None))
        if masked:
            hrules["null_mask"] = dict(mask=None)
        out.append((name + "_host", name[len("knn_index_"):] + "_host_c", hargs, hvalid, hrules))
    out.append(("knn_index_self_topk", "self_topk_c", ["slot", "row_first", "rows", "K", "max_dist2", "keys", "indices", "stream", "flags"],
                dict(slot=0, row_first=7, rows=20, K=5, max_dist2=1.0, keys=KEYS, indices=None, stream=None, flags=1),
                dict(radius=dict(max_dist2=-1.0), flags=dict(flags=1 | 64), slot=dict(slot=8), rows=dict(rows=0),
                     row_first=dict(row_first=-1), K=dict(K=0), mK=dict(rows=INT_MAX // 64 + 1, K=64), null_keys=dict(keys=None))))
    out.append(("knn_index_self_topk_host", "self_topk_host_c", ["K", "max_dist2", "indices", "dist2", "counts"],
                dict(K=5, max_dist2=1.0, indices=OUT, dist2=None, counts=None),
                dict(radius=dict(max_dist2=-1.0), K=dict(K=0), null_indices=dict(indices=None))))
    return out


def cases():
    """[(entry, accessor, [broken rules], argument values after the index)] in the table's order."""
    out = []
    for name, accessor, args, valid, rules in entries():
        names = list(rules)
        sets = [()] + [(r,) for r in names] + [p for p in itertools.combinations(names, 2) if not set(rules[p[0]]) & set(rules[p[1]])]
        for broken in sets:
            values = dict(valid)
            for r in broken:
                values.update(rules[r])
            out.append((name, accessor, list(broken), [values[a] for a in args]))
    return out


def table():
    """The table of the library the package loads (KNN_MI355X_LIB, else the tree's build)."""
    import multicore_hw2_amd as pkg

    rows = []
    for name, accessor, broken, values in cases():
        code = getattr(pkg, accessor)()(None, *values)
        rows.append(dict(entry=name, broken=broken, code=int(code), text=pkg.lib().knn_last_error().decode()))
    return rows


if __name__ == "__main__":
    text = json.dumps(table(), indent=0) + "\n"
    if len(sys.argv) == 3 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
