"""knn_index_list_within — what its GPU tests share (test infrastructure): device buffers, the call itself and how a segmented
answer is compared.  Expectations always come from tests/list_oracle.py."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import dev, dev_counts, host_counts
from tests.list_oracle import lengths, offsets_of

PAD = np.uint64(0xA5A5A5A5A5A5A5A5)     # what a key buffer holds before a call: no packed key of a finite distance


def dev_u64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).to(dev())


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def list_call(ix, Q, r2, offsets, fill=None, keys=None, total=None, init=True, slot=0, stream=0, **flags):
    """One call of list_within on segments `offsets` (numpy uint64 [m + 1]): (fill uint32 [m], keys uint64 [total]) after it.
    Without `fill` the call starts from a cursor that held 0xDEADBEEF (init) or zeros (appending); without `keys` it writes a
    buffer of `total` (default offsets[m]) entries that held PAD."""
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(dev())
    off_d = dev_u64(offsets)
    if fill is None:
        fill = dev_counts(m, fill=0xDEADBEEF if init else 0)
    if keys is None:
        keys = dev_u64(np.full(max(int(offsets[m]) if total is None else total, 1), PAD))
    torch.cuda.synchronize()
    ix.list_within(m, q_d.data_ptr(), r2, off_d.data_ptr(), fill.data_ptr(), keys.data_ptr(), init=init, slot=slot, stream=stream,
                   **flags)
    torch.cuda.synchronize()
    return host_counts(fill), host_u64(keys)


def segments(offsets, fill, keys):
    """[m] sorted arrays: the first min(fill, room) keys of every segment, sorted on the host (the order within one is unspecified)."""
    return [np.sort(keys[int(offsets[j]):int(offsets[j]) + min(int(fill[j]), int(offsets[j + 1] - offsets[j]))])
            for j in range(len(fill))]


def assert_lists(got, want, msg=""):
    assert len(got) == len(want), msg
    for j, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} query {j}")


def check_list(ix, Q, r2, want, msg="", **kw):
    """One init call on segments made from the expected lists' lengths: fill equals the count, the segments hold the expected keys."""
    off = offsets_of(lengths(want))
    fill, keys = list_call(ix, Q, r2, off, **kw)
    np.testing.assert_array_equal(fill, lengths(want), err_msg=f"{msg} fill")
    assert_lists(segments(off, fill, keys), want, msg)
    return fill, keys


def sorted_on_device(m, offsets, fill, keys):
    """keys_sort_segments on host arrays: the keys after it."""
    off_d, keys_d = dev_u64(offsets), dev_u64(keys)
    fill_d = dev_counts(m, fill=np.asarray(fill, dtype=np.uint32))
    torch.cuda.synchronize()
    pkg.keys_sort_segments(m, off_d.data_ptr(), fill_d.data_ptr(), keys_d.data_ptr())
    torch.cuda.synchronize()
    return host_u64(keys_d)
