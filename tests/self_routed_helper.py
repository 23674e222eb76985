"""The routed self calls (include/knn_mi355x.h 2k) — what their GPU tests share (test infrastructure): the device pipeline count ->
offsets -> list -> sort through the routed calls and through the existing self calls, the duplicate arrangement of a window, and
the checks every answer gets.  Expectations always come from tests/each_oracle.py over tests/self_oracle.self_dist2."""
import numpy as np
import torch  # noqa: F401  imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

from tests import each_oracle as eo
from tests.each_helper import assert_segments, pipeline

INF = float("inf")
LOW = np.uint64(0xFFFFFFFF)


def routed_pipeline(ix, first, rows, cap, r_d=None, **flags):
    """(counts, offsets, fill, sorted keys, the stats after both calls) of the routed self calls; r_d: a device radius per row or
    None (the scalar form at cap)."""
    rp = r_d.data_ptr() if r_d is not None else None

    def count(ix, counts, init):
        ix.self_count_within_routed(first, rows, counts.data_ptr(), cap=cap, max_dist2_dev=rp, init=init, **flags)

    def lst(ix, off, fill, keys, init):
        ix.self_list_within_routed(first, rows, off.data_ptr(), fill.data_ptr(), keys.data_ptr(), cap=cap, max_dist2_dev=rp, init=init,
                                   **flags)

    return pipeline([ix], None, None, rows, count=count, lst=lst)


def existing_pipeline(ix, first, rows, cap, r_d=None):
    """The same through the existing self calls: self_count_within / self_list_within at cap, or their _each forms under cap."""
    def count(ix, counts, init):
        if r_d is None:
            ix.self_count_within(first, rows, cap, counts.data_ptr(), init=init)
        else:
            ix.self_count_within_each(first, rows, r_d.data_ptr(), counts.data_ptr(), cap=cap, init=init)

    def lst(ix, off, fill, keys, init):
        if r_d is None:
            ix.self_list_within(first, rows, cap, off.data_ptr(), fill.data_ptr(), keys.data_ptr(), init=init)
        else:
            ix.self_list_within_each(first, rows, r_d.data_ptr(), off.data_ptr(), fill.data_ptr(), keys.data_ptr(), cap=cap, init=init)

    return pipeline([ix], None, None, rows, count=count, lst=lst)


def plant_duplicates(R, first, inside=(20, 11), outside=50):
    """Row first + inside[0] copied to first + inside[1] (inside the window) and to row `outside` (outside it): three rows at one
    place.  With tests.each_oracle's kinds both window rows get a "zero" radius (20 % 9 == 11 % 9 == 2)."""
    assert eo.KINDS[inside[0] % 9] == "zero" and eo.KINDS[inside[1] % 9] == "zero"
    R[first + inside[1]] = R[first + inside[0]]
    R[outside] = R[first + inside[0]]
    return first + inside[0], first + inside[1], outside


def assert_same_answer(got, want_lists, ref=None, msg=""):
    """got / ref: (counts, offsets, fill, keys, ...) of a pipeline; want_lists: the oracle's sorted lists (or None)."""
    counts, off, fill, keys = got[:4]
    np.testing.assert_array_equal(fill, counts, err_msg=f"{msg} fill")
    if want_lists is not None:
        np.testing.assert_array_equal(counts, eo.lengths(want_lists), err_msg=f"{msg} counts")
        assert_segments(off, keys, want_lists, msg=msg)
    if ref is not None:
        np.testing.assert_array_equal(counts, ref[0], err_msg=f"{msg} counts against the existing self call")
        np.testing.assert_array_equal(off, ref[1], err_msg=f"{msg} offsets against the existing self call")
        np.testing.assert_array_equal(keys, ref[3], err_msg=f"{msg} keys against the existing self call")


def assert_own_row_absent(got, own_numbers, msg=""):
    """own_numbers[j]: the number query j's own row would carry in a key."""
    _, off, _, keys = got[:4]
    for j, own in enumerate(own_numbers):
        assert not ((keys[int(off[j]):int(off[j + 1])] & LOW) == np.uint64(own)).any(), (msg, j)


def segment_numbers(got, j):
    """The row numbers (low words) of query j's sorted segment, and its distances' bits (high words)."""
    _, off, _, keys = got[:4]
    seg = keys[int(off[j]):int(off[j + 1])]
    return (seg & LOW).astype(np.int64), (seg >> np.uint64(32)).astype(np.uint32)
