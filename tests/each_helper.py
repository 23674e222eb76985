"""The calls with a radius per query — what their GPU tests share (test infrastructure): the calls themselves and the device
pipeline count -> offsets -> list -> sort.  Expectations always come from tests/each_oracle.py."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import dev, dev_counts, host_counts
from tests.list_helper import PAD, dev_u64, host_u64


def dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(-1)).to(dev())


def count_each(ix, Q, r, cap=float("inf"), counts=None, init=True, slot=0, **flags):
    """One call of count_within_each: the counts [m] (numpy uint32) after it."""
    q_d, r_d = dev_f32(Q), dev_f32(r)
    m = r_d.numel()
    if counts is None:
        counts = dev_counts(m, fill=0xDEADBEEF if init else 0)
    torch.cuda.synchronize()
    ix.count_within_each(m, q_d.data_ptr(), r_d.data_ptr(), counts.data_ptr(), cap=cap, init=init, slot=slot, **flags)
    torch.cuda.synchronize()
    return host_counts(counts)


def list_each(ix, Q, r, offsets, cap=float("inf"), fill=None, keys=None, init=True, slot=0, **flags):
    """One call of list_within_each on segments `offsets` (numpy uint64 [m + 1]): (fill uint32 [m], keys uint64) after it."""
    q_d, r_d = dev_f32(Q), dev_f32(r)
    m = r_d.numel()
    off_d = dev_u64(offsets)
    if fill is None:
        fill = dev_counts(m, fill=0xDEADBEEF if init else 0)
    if keys is None:
        keys = dev_u64(np.full(max(int(offsets[m]), 1), PAD))
    torch.cuda.synchronize()
    ix.list_within_each(m, q_d.data_ptr(), r_d.data_ptr(), off_d.data_ptr(), fill.data_ptr(), keys.data_ptr(), cap=cap, init=init,
                        slot=slot, **flags)
    torch.cuda.synchronize()
    return host_counts(fill), host_u64(keys)


def pipeline(shards, q_d, r_d, m, cap=float("inf"), count=None, lst=None, **flags):
    """count -> knn_counts_to_offsets -> list -> knn_keys_sort_segments on the device, folding over `shards` (index objects), with one
    host step: the total, which sizes the key buffer.  count / lst: the two calls as f(ix, counts_or_None, off, fill, keys, init) —
    default: count_within_each / list_within_each on q_d, r_d.  Returns (counts uint32 [m], offsets uint64 [m + 1], fill uint32
    [m], keys uint64 [total], the stats after every call)."""
    stats = []
    counts = dev_counts(m, fill=0xDEADBEEF)
    off = torch.empty(m + 1, dtype=torch.int64, device=dev())
    fill = dev_counts(m, fill=0xDEADBEEF)
    for i, ix in enumerate(shards):
        if count:
            count(ix, counts, i == 0)
        else:
            ix.count_within_each(m, q_d.data_ptr(), r_d.data_ptr(), counts.data_ptr(), cap=cap, init=(i == 0), **flags)
        stats.append(ix.last_stats())
    pkg.counts_to_offsets(counts.data_ptr(), m, off.data_ptr())
    torch.cuda.synchronize()
    total = int(off[m].item())
    keys = dev_u64(np.full(max(total, 1), PAD))
    for i, ix in enumerate(shards):
        if lst:
            lst(ix, off, fill, keys, i == 0)
        else:
            ix.list_within_each(m, q_d.data_ptr(), r_d.data_ptr(), off.data_ptr(), fill.data_ptr(), keys.data_ptr(), cap=cap,
                                init=(i == 0), **flags)
        stats.append(ix.last_stats())
    pkg.keys_sort_segments(m, off.data_ptr(), fill.data_ptr(), keys.data_ptr())
    torch.cuda.synchronize()
    return host_counts(counts), host_u64(off), host_counts(fill), host_u64(keys)[:total], stats


def assert_segments(off, keys, want, which=None, msg=""):
    """Sorted segments against the oracle's lists, bit for bit; which: the queries to look at (default: all)."""
    for j in (range(len(want)) if which is None else which):
        np.testing.assert_array_equal(keys[int(off[j]):int(off[j + 1])], want[j], err_msg=f"{msg} query {j}")
