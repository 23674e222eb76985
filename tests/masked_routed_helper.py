"""The routed masked calls (include/knn_mi355x.h 2l) — what their GPU tests share (test infrastructure): masks as words, the
oracle's distances under a mask, the device pipeline count -> offsets -> list -> sort through the routed masked calls and through
the existing masked calls, and the CPU-side checks that a batch proves what it claims.  Expectations always come from
tests/topk_oracle.v0_dist2 with the masked-out columns set to +INF, through tests/each_oracle.py's counts_of / lists_of."""
import numpy as np
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

from tests import each_oracle as eo
from tests.count_helper import dev
from tests.each_helper import assert_segments, pipeline

INF = np.float32(np.inf)


def words_of(bits, beyond=0):
    """uint32 [(n + 31) // 32]: bit i % 32 of word i // 32 = bits[i]; beyond = 1 sets every bit of the last word at and beyond n."""
    bits = np.asarray(bits, dtype=bool)
    n = bits.size
    padded = np.full((n + 31) // 32 * 32, bool(beyond))
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view(np.uint32).copy()


def dev_words(words):
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev())


def under(d, bits):
    """d [m][n] with the columns the mask does not admit set to +INF: no hit at any radius."""
    out = np.array(d, dtype=np.float32, copy=True)
    out[:, ~np.asarray(bits, dtype=bool)] = INF
    return out


def scalar(m, r2):
    return np.full(m, r2, dtype=np.float32)


def want_of(d, bits, r2, base=0, gids=None):
    """(counts uint32 [m], sorted lists) of the oracle under the mask at the scalar radius r2."""
    dm = under(d, bits)
    r = scalar(d.shape[0], r2)
    return eo.counts_of(dm, r), eo.lists_of(dm, r, gids=gids, base=base)


def assert_mask_bites(d, bits, r2, keeps=True):
    """Some query loses at least one unmasked hit to the mask and (keeps) keeps at least one; some query keeps none."""
    r = scalar(d.shape[0], r2)
    plain, masked = eo.counts_of(d, r), eo.counts_of(under(d, bits), r)
    if keeps:
        assert ((masked < plain) & (masked > 0)).any(), "no query loses a hit to the mask and keeps one: change the seed"
    else:
        assert (masked < plain).any()
    assert (masked == 0).any(), "every query keeps a hit: change the seed"


def routed_pipeline(shards, q_d, masks_d, m, r2, **flags):
    """(counts, offsets, fill, sorted keys, the stats after every call) of the routed masked calls folded over `shards`;
    masks_d[i]: shard i's mask words on the device."""
    at = {id(ix): w for ix, w in zip(shards, masks_d)}

    def count(ix, counts, init):
        ix.count_within_masked_routed(m, q_d.data_ptr(), r2, at[id(ix)].data_ptr(), counts.data_ptr(), init=init, **flags)

    def lst(ix, off, fill, keys, init):
        ix.list_within_masked_routed(m, q_d.data_ptr(), r2, at[id(ix)].data_ptr(), off.data_ptr(), fill.data_ptr(), keys.data_ptr(),
                                     init=init, **flags)

    return pipeline(shards, None, None, m, count=count, lst=lst)


def existing_pipeline(shards, q_d, masks_d, m, r2, **kw):
    """The same through knn_index_count_within_masked / knn_index_list_within_masked; kw: slot."""
    at = {id(ix): w for ix, w in zip(shards, masks_d)}

    def count(ix, counts, init):
        ix.count_within_masked(m, q_d.data_ptr(), r2, at[id(ix)].data_ptr(), counts.data_ptr(), init=init, **kw)

    def lst(ix, off, fill, keys, init):
        ix.list_within_masked(m, q_d.data_ptr(), r2, at[id(ix)].data_ptr(), off.data_ptr(), fill.data_ptr(), keys.data_ptr(), init=init,
                              **kw)

    return pipeline(shards, None, None, m, count=count, lst=lst)


def assert_same_answer(got, want, ref=None, msg=""):
    """got / ref: (counts, offsets, fill, keys, ...) of a pipeline; want: (counts, sorted lists) of the oracle."""
    counts, off, fill, keys = got[:4]
    np.testing.assert_array_equal(counts, want[0], err_msg=f"{msg} counts")
    np.testing.assert_array_equal(fill, counts, err_msg=f"{msg} fill")
    assert_segments(off, keys, want[1], msg=msg)
    if ref is not None:
        np.testing.assert_array_equal(counts, ref[0], err_msg=f"{msg} counts against the existing masked call")
        np.testing.assert_array_equal(keys, ref[3], err_msg=f"{msg} keys against the existing masked call")
