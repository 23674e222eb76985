"""The chunk walk of the exact slice scans (csrc/knn_slice_launch.h) through knn_debug_slice_chunks, host arithmetic only: the
chunks tile the queries once and in order, no chunk holds more than 65536, the slices and the rows per slice are the count scan's
and the top-K scan's rules — restated here from the rules' own source text (knn_count_slices and knn_topk_slices, knn_exact.hip),
not read back from the library —, the slices cover the rows with none empty, the grid's other side is the chunk's waves of 64
queries, and the first chunk is what the self plan and the masked plan report."""
import itertools

import pytest

import multicore_hw2_amd as pkg

CHUNK, WAVE, PART_BYTES = 65536, 64, 128 << 20
MS = (1, 64, 65, 65536, 65537, 131077)
NS = (1, 1023, 1024, 10 ** 6, 2 ** 27)
KS = (0, 1, 16, 17, 64)            # 0: the count rule
CUS = (256, 8)


def divup(a, b):
    return (a + b - 1) // b


def even_cut(n, slices):
    """The rules' last two lines: slices of ceil(n / slices) rows, and as many of them as hold a row."""
    per = divup(n, slices)
    return divup(n, per)


def count_slices(mc, n, num_cu):
    slices = num_cu * 32 // divup(mc, WAVE)
    slices = min(slices, divup(n, 1024), 65535)
    return even_cut(n, max(slices, 1))


def topk_slices(mc, K, n, num_cu):
    slices = num_cu * (32 if K <= 16 else 8) // divup(mc, WAVE)
    slices = min(slices, divup(n, 1024), PART_BYTES // (mc * K * 8), 65535)
    return even_cut(n, max(slices, 1))


@pytest.mark.parametrize("num_cu", CUS)
@pytest.mark.parametrize("K", KS)
def test_chunks_tile_the_queries_and_cut_the_rows_by_the_rules(K, num_cu):
    for m, n in itertools.product(MS, NS):
        chunks = pkg.debug_slice_chunks(m, n, num_cu, K=K, rule="topk" if K else "count")
        assert len(chunks) == divup(m, CHUNK), (m, n)
        at = 0
        for ch in chunks:
            where = (m, n, K, num_cu, ch)
            assert ch["c0"] == at and 1 <= ch["mc"] <= CHUNK, where
            at += ch["mc"]
            slices = topk_slices(ch["mc"], K, n, num_cu) if K else count_slices(ch["mc"], n, num_cu)
            assert ch["slices"] == slices and ch["per"] == divup(n, slices), where
            assert ch["slices"] * ch["per"] >= n and (ch["slices"] - 1) * ch["per"] < n, where
            assert ch["grid_x"] == ch["slices"] and ch["grid_y"] == divup(ch["mc"], WAVE), where
        assert at == m, (m, n)
        assert all(ch["mc"] == CHUNK for ch in chunks[:-1]), (m, n)
        first = chunks[0]
        mp = pkg.debug_masked_plan(k=3, m=m, K=K, rows=n, num_cu=num_cu, init=1)
        assert (mp["chunks"], mp["chunk_m"], mp["slices"]) == (len(chunks), first["mc"], first["slices"]), (m, n, mp)
        assert mp["part_bytes"] == max(ch["slices"] * ch["mc"] * K * 8 for ch in (chunks[0], chunks[-1])), (m, n, mp)
        if n >= m:   # (a self call's rows are rows of the shard)
            sp = pkg.debug_self_plan(k=3, rows=m, K=K, shard_rows=n, num_cu=num_cu, init=1)
            assert (sp["chunks"], sp["chunk_rows"], sp["slices"], sp["groups"]) == \
                (len(chunks), first["mc"], first["slices"], first["grid_y"]), (m, n, sp)
            assert sp["part_bytes"] == mp["part_bytes"] and sp["lds_bytes"] == mp["lds_bytes"] == K * WAVE * 8, (m, n, sp)


def test_the_select_rule_and_the_argument_rules():
    # a histogram pass of the radix select: 4 blocks per CU over the chunk's waves, >= 1024 rows (128 per wave of 8) a slice
    for m, n in itertools.product(MS, NS):
        for ch in pkg.debug_slice_chunks(m, n, 256, rule="select"):
            slices = even_cut(n, max(min(256 * 4 // divup(ch["mc"], WAVE), divup(n, 1024), 65535), 1))
            assert ch["slices"] == slices and ch["per"] == divup(n, slices), (m, n, ch)
    large = pkg.debug_topk_large_plan(k=3, m=131077, K=100, rows=10 ** 6, num_cu=256, init=1)
    first = pkg.debug_slice_chunks(131077, 10 ** 6, 256, rule="select")[0]
    assert (large["chunks"], large["slices"]) == (3, first["slices"]), large
    for bad in (dict(m=0, n=5, num_cu=8), dict(m=5, n=0, num_cu=8), dict(m=5, n=5, num_cu=0), dict(m=5, n=5, num_cu=8, K=0, rule="topk"),
                dict(m=5, n=5, num_cu=8, K=65, rule="topk"), dict(m=5, n=2 ** 32 + 1, num_cu=8)):
        with pytest.raises(pkg.KnnError, match="knn_debug_slice_chunks: bad arguments"):
            pkg.debug_slice_chunks(**bad)
