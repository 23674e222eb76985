"""The dense filter query's plan (knn_filter_query_plan, multicore_hw2_amd/csrc/knn_filter.hip) on the CPU: every choice and size
one batch on the dense layouts launches with — the scan's form, its pieces and grids, the record lists, the sample pass, the
thresholds and the slots' chain — against the rules the query applied inline before the plan had a function of its own."""
import itertools
import random

import pytest

KMAX_LISTS, SAMPLE_BLOCKS_MAX, CHK_KC, CHK_T, CHK_QT = 1 << 16, 512, 8, 4, 2   # knn_common.h / knn_filter.hip
PIECES, TILED, CHUNKED = 0, 1, 2
KTS = (1, 2, 4, 8, 16, 32, 40, 64)                   # k 16, 32, 64, 128, 256, 512, 600, 1024
QTILES = (1, 2, 3, 8, 9, 16, 17, 18, 19, 32, 35, 2048)
NTILES = (1, 7, 255, 4096, (1 << 19) - 1, 1 << 19)
NUM_CUS = (8, 256, 304)
KS = (0, 1, 5, 64)
OPTIONS = dict(filter_qt=(0, 2, 8, 16, 32), filter_rounds=(0, 1, 3), filter_chain=(0, 1, 2), run_thresholds=(0, 1, 2),
               sample_stride=(0, 1, 8, 1024))
# the instantiations the code object holds: (form, KT, QT) of knn_filter_kernel / knn_filter_sample_kernel (pieces),
# knn_filter_tiled_kernel in its sample and scan forms (tiled), knn_filter_chunked_kernel<true / false> (any kt, CHK_QT)
INSTANTIATIONS = ({(PIECES, 1, qt) for qt in (2, 8, 16, 32)} | {(PIECES, 2, 8), (PIECES, 2, 16), (PIECES, 4, 4), (PIECES, 8, 2)} |
                  {(TILED, 4, 4), (TILED, 8, 4), (TILED, 16, 2), (TILED, 32, 1)} | {(CHUNKED, 0, CHK_QT)})


def cdiv(a, b):
    return (a + b - 1) // b


def parent_pieces(kt, qtiles, force_qt):
    """plan_pieces: (qt, first tile, tiles) of every piece."""
    out, pos, rem = [], 0, qtiles

    def push(qt, cnt):
        nonlocal pos, rem
        out.append((qt, pos, cnt))
        pos += cnt
        rem -= cnt
    if force_qt > 0 and kt == 1:
        push(force_qt, rem)
    elif kt == 1:
        if rem >= 32:
            push(32, rem // 32 * 32)
        if rem > 18:
            push(32, rem)
        elif rem > 16:
            push(16, 16)
            push(2, rem)
        elif rem > 8:
            push(16, rem)
        elif rem > 2:
            push(8, rem)
        elif rem > 0:
            push(2, rem)
    elif kt == 2:
        if rem >= 16:
            push(16, rem // 16 * 16)
        if rem > 8:
            push(16, rem)
        elif rem > 0:
            push(8, rem)
    elif kt == 4:
        push(4, rem)
    else:
        push(2, rem)
    return out


def parent_filter_plan(kt, ntiles, m, num_cu, rec_cap, topk, filter_qt, filter_rounds, filter_chain, run_thresholds,
                       sample_stride):
    """The rules launch_scan_for_kt, launch_filter<KT>, launch_filter_tiled<KT, QT> and launch_filter_chunked applied inline."""
    qtiles = cdiv(m, 32)
    m_padded = qtiles * 32
    target = num_cu * 8
    if kt in (1, 2) or (kt in (4, 8) and qtiles < 16):
        form = PIECES
    elif kt in (4, 8, 16, 32):
        form = TILED
    else:
        form = CHUNKED
        if kt % CHK_KC:
            return dict(ok=0)
    pieces, nlists, gy_sum = [], 0, 0
    if form == PIECES:
        for qt, begin, count in parent_pieces(kt, qtiles, filter_qt):
            qk = qt * kt
            gy = cdiv(count, qt)
            waves = num_cu * (8 if qk > 16 else 12 if qk == 16 else 20 if qk <= 2 else 16)
            waves *= filter_rounds if filter_rounds > 0 else 1
            waves = min(waves, ntiles)
            gx = (waves + 3) // 4
            if gy > 1 and gx * gy > target:
                gx = cdiv(target, gy)
            gx = max(gx, 1)
            while gx * 4 * gy > KMAX_LISTS // 4 and gx > 1:
                gx = (gx + 1) // 2
            pieces.append(dict(qt=qt, begin=begin, count=count, gx=gx, gy=gy, list_base=nlists))
            nlists += gx * 4 * gy
            gy_sum += gy
        if nlists == 0 or nlists > KMAX_LISTS:
            return dict(ok=0)
    else:
        qt = {4: 4, 8: 4, 16: 2, 32: 1}.get(kt, CHK_QT)
        gy = cdiv(qtiles, 4 * qt)
        if form == TILED:
            gx = min(cdiv(target, gy), ntiles)
        else:
            gx = min(max(16, cdiv(num_cu * 4, gy)), cdiv(ntiles, CHK_T))
        gx = max(gx, 1)
        while gx * 4 * gy > KMAX_LISTS and gx > 1:
            gx = (gx + 1) // 2
        if gx * 4 * gy > KMAX_LISTS:
            return dict(ok=0)
        nlists = gx * 4 * gy
        pieces.append(dict(qt=qt, begin=0, count=qtiles, gx=gx, gy=gy, list_base=0))
    stride = min(16, max(1, ntiles // 256))
    if form == TILED:
        if kt >= 8 and run_thresholds != 2:
            stride = min(32, max(1, ntiles // 64))
        if sample_stride > 0:
            stride = min(sample_stride, max(1, ntiles // 16))
    if topk > 0:
        stride = max(1, stride // topk)
    ns = cdiv(ntiles, stride)
    if form == PIECES:
        sb = min(num_cu * 2, SAMPLE_BLOCKS_MAX)
        if gy_sum > 1 and sb * gy_sum > target:
            sb = cdiv(target, gy_sum)
        if sb * 32 > ns:
            sb = cdiv(ns, 32)
        sb = max(sb, 1)
        if topk > 0:
            sb = max(sb, min(ns, SAMPLE_BLOCKS_MAX, 4 * topk))
    elif form == TILED:
        sb = min(gx, ns)
    else:
        sb = min(gx, cdiv(ns, CHK_T))
    no_chain = filter_chain == 2 or (filter_chain == 0 and ntiles < (1 << 19))
    if form == PIECES:
        rr = (len(pieces), tuple(p["list_base"] for p in pieces) + (0xFFFFFFFF,) * (4 - len(pieces)),
              tuple(p["begin"] * 32 for p in pieces) + (0,) * (4 - len(pieces)))
    else:
        rr = (1, (0,) + (0xFFFFFFFF,) * 3, (0,) * 4)
    return dict(ok=1, form=form, kt=kt, npieces=len(pieces), nlists=nlists, slice=rec_cap // nlists, stride=stride, sample_blocks=sb,
                umin_floats=sb * m_padded, topk=topk, thr_nb=1 if topk > 0 else sb, thr_running=int(form == TILED),
                scan_running=int(form == TILED and run_thresholds != 2), in_chain=int(form != CHUNKED),
                chained=int(form != CHUNKED and not no_chain), has_rows=int(form != PIECES), pieces=pieces, rerank=rr)


def size_grid():
    for kt, qtiles, ntiles, num_cu, topk in itertools.product(KTS, QTILES, NTILES, NUM_CUS, KS):
        yield dict(kt=kt, ntiles=ntiles, m=qtiles * 32 - (qtiles * 7) % 32, num_cu=num_cu, topk=topk)


def option_sets():
    """Each option over its values with the others at 0 (the full product: a fixed-seed sample, in a test of its own)."""
    zero = {n: 0 for n in OPTIONS}
    yield zero
    for name, values in OPTIONS.items():
        for v in values[1:]:
            yield dict(zero, **{name: v})


def plan(pkg, rec_cap, **inputs):
    return pkg.debug_filter_query_plan(rec_cap=rec_cap, **inputs)


@pytest.fixture(scope="module")
def rec_cap():
    import multicore_hw2_amd as pkg
    return pkg.debug_scan_plan(256, 2, 100, 1)["rec_cap"]


def check_invariants(got, inputs, rec_cap):
    qtiles = cdiv(inputs["m"], 32)
    pieces = got["pieces"]
    assert 1 <= got["npieces"] <= 4 and len(pieces) == got["npieces"], inputs
    pos = lists = 0
    for pc in pieces:   # the pieces tile [0, qtiles) in order, each with its own run of record lists
        assert pc["begin"] == pos and pc["count"] >= 1 and pc["list_base"] == lists, inputs
        assert pc["gx"] >= 1 and pc["gy"] == cdiv(pc["count"], pc["qt"] if got["form"] == PIECES else 4 * pc["qt"]), inputs
        pos += pc["count"]
        lists += pc["gx"] * 4 * pc["gy"]
    assert pos == qtiles and lists == got["nlists"], inputs
    assert 1 <= got["nlists"] <= KMAX_LISTS and got["slice"] >= 1 and got["nlists"] * got["slice"] <= rec_cap, inputs
    assert got["sample_blocks"] >= 1 and got["umin_floats"] == got["sample_blocks"] * qtiles * 32, inputs
    assert got["stride"] >= 1 and got["thr_nb"] == (1 if inputs["topk"] else got["sample_blocks"]), inputs
    if inputs["topk"] and got["form"] == PIECES:   # well over K blocks for the K-th smallest minimum, as far as the sampled tiles go
        sampled = cdiv(inputs["ntiles"], got["stride"])
        assert got["sample_blocks"] >= min(sampled, SAMPLE_BLOCKS_MAX, 4 * inputs["topk"]), inputs
    assert got["chained"] <= got["in_chain"] and got["scan_running"] <= got["thr_running"], inputs
    for pc in pieces:
        assert (got["form"], 0 if got["form"] == CHUNKED else got["kt"], pc["qt"]) in INSTANTIATIONS, inputs


@pytest.mark.parametrize("kt", KTS)
def test_plan_reproduces_the_rules_the_query_applied(kt, rec_cap):
    """knn_filter_query_plan against the parent's inline rules over the sizes, K and every value of each option."""
    import multicore_hw2_amd as pkg
    for sizes in size_grid():
        if sizes["kt"] != kt:
            continue
        for opts in option_sets():
            inputs = dict(sizes, **opts)
            got = plan(pkg, rec_cap, **inputs)
            want = parent_filter_plan(rec_cap=rec_cap, **inputs)
            assert got["ok"] == want["ok"], inputs
            if not want["ok"]:
                continue
            assert {n: got[n] for n in want} == want, inputs
            check_invariants(got, inputs, rec_cap)


def test_plan_matches_a_sample_of_the_full_product(rec_cap):
    """A fixed-seed sample of every size, K and option value together."""
    import multicore_hw2_amd as pkg
    rng = random.Random(20261016)
    sizes = list(size_grid())
    for _ in range(20000):
        inputs = dict(rng.choice(sizes), **{n: rng.choice(v) for n, v in OPTIONS.items()})
        got = plan(pkg, rec_cap, **inputs)
        want = parent_filter_plan(rec_cap=rec_cap, **inputs)
        assert got["ok"] == want["ok"] == 1, inputs
        assert {n: got[n] for n in want} == want, inputs
        check_invariants(got, inputs, rec_cap)


def test_plan_refuses_what_the_query_refused(rec_cap):
    """ok = 0 where the query returned hipErrorInvalidValue: kt beyond 32 that is not a multiple of CHK_KC (nothing else gets
    there: knn_kt_of rounds k > 512 up to 128 dimensions), and more record lists than a workspace counts."""
    import multicore_hw2_amd as pkg
    base = dict(ntiles=4096, m=1024, num_cu=256, topk=0, **{n: 0 for n in OPTIONS})
    for kt in (3, 12, 36, 44):
        assert plan(pkg, rec_cap, kt=kt, **base)["ok"] == 0
    assert plan(pkg, rec_cap, kt=24, **base)["ok"] == 1 and plan(pkg, rec_cap, kt=24, **base)["form"] == CHUNKED
    # 2^23 queries at k 256 (one range per group of 8 query tiles: 2^17 lists), 2^25 at k 16 (one wave per 32 query tiles: 2^17)
    for kt, m in ((16, 1 << 23), (1, 1 << 25)):
        huge = dict(base, m=m, ntiles=1 << 19)
        assert plan(pkg, rec_cap, kt=kt, **huge)["ok"] == 0
        assert parent_filter_plan(rec_cap=rec_cap, kt=kt, **huge)["ok"] == 0
        assert plan(pkg, rec_cap, kt=kt, **dict(huge, m=m // 2))["ok"] == 1
    for bad in (dict(kt=0), dict(topk=65), dict(filter_qt=4), dict(filter_chain=3), dict(sample_stride=1025), dict(m=0)):
        with pytest.raises(pkg.KnnError):
            plan(pkg, rec_cap, **dict(dict(base, kt=1), **bad))


def test_plan_reaches_exactly_the_instantiations_the_code_object_holds(rec_cap):
    """The (form, KT, QT) the plan can produce — each a sample and a scan launch — are the instantiations the code holds."""
    import multicore_hw2_amd as pkg
    seen = set()
    for kt, qtiles, fqt in itertools.product(KTS, QTILES, OPTIONS["filter_qt"]):
        got = plan(pkg, rec_cap, kt=kt, ntiles=4096, m=qtiles * 32, num_cu=256, topk=0, filter_qt=fqt, filter_rounds=0,
                   filter_chain=0, run_thresholds=0, sample_stride=0)
        seen |= {(got["form"], 0 if got["form"] == CHUNKED else got["kt"], pc["qt"]) for pc in got["pieces"]}
    assert seen == INSTANTIATIONS and len(seen) == 13


def test_chain_and_running_thresholds_follow_the_form(rec_cap):
    """The chunked scan (k > 512) stays outside the slots' chain whatever the option says; the pieces and LDS-tiled scans chain
    from 2^19 tiles under the automatic policy.  Running thresholds: written by the thresholds kernel of every LDS-tiled batch,
    handed to the scan unless run_thresholds = 2, and they thin the sample pass out at KT >= 8 only."""
    import multicore_hw2_amd as pkg
    zero = {n: 0 for n in OPTIONS}
    for kt, m in ((1, 1024), (8, 200), (8, 1024), (16, 32), (64, 1024)):
        for chain, ntiles in ((0, (1 << 19) - 1), (0, 1 << 19), (1, 7), (2, 1 << 19)):
            got = plan(pkg, rec_cap, kt=kt, ntiles=ntiles, m=m, num_cu=256, topk=0, **dict(zero, filter_chain=chain))
            assert got["in_chain"] == (kt <= 32), (kt, m)
            assert got["chained"] == (kt <= 32 and (chain == 1 or (chain == 0 and ntiles >= 1 << 19))), (kt, m, chain, ntiles)
    for kt, m, tiled in ((4, 480, 0), (4, 481, 1), (8, 480, 0), (8, 481, 1), (16, 1, 1), (32, 1, 1)):
        for rt in (0, 2):
            got = plan(pkg, rec_cap, kt=kt, ntiles=4096, m=m, num_cu=256, topk=0, **dict(zero, run_thresholds=rt))
            assert got["form"] == (TILED if tiled else PIECES) and got["thr_running"] == tiled, (kt, m)
            assert got["scan_running"] == (tiled and rt != 2), (kt, m, rt)
            assert got["stride"] == (32 if tiled and kt >= 8 and rt != 2 else 16), (kt, m, rt)
