"""knn_counts_to_offsets and knn_keys_sort_segments on the GPU against numpy: the 64-bit running sum across the chunks of the
offsets kernel, and the segment sort on every length at which it takes another path (nothing to do, in LDS, in global memory),
with repeated keys, a fill below, at and above the room, and everything outside the sorted part left as it was."""
import numpy as np
import pytest
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg
from tests.count_helper import dev, dev_counts
from tests.list_helper import dev_u64, host_u64, sorted_on_device
from tests.list_oracle import offsets_of

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    assert pkg.device_count() >= 1, "no GPU visible to libknn_mi355x.so"
    yield


@pytest.mark.parametrize("m", [1, 70, 1023, 1024, 1025, 2048, 2049, 5000])
def test_offsets_are_the_64_bit_prefix_sums(m):
    """(2048 counts are one chunk of the kernel's block: 2048 and 2049 sit on its edge.)"""
    rng = np.random.default_rng(m)
    c = rng.integers(0, 1000, m).astype(np.uint32)
    c[rng.random(m) < 0.3] = 0
    if m >= 70:
        c[[3, m - 2]] = 0xFFFFFFFF          # two of them: the total passes 2^33 - 2, the carry crosses 32 bits twice
    else:
        c[0] = 0xFFFFFFFF
    want = offsets_of(c)
    assert want[m] > 0xFFFFFFFF or m == 1
    c_d = dev_counts(m, fill=c)
    off_d = dev_u64(np.full(m + 2, 0x1111111111111111, dtype=np.uint64))      # one guard word behind offsets[m]
    torch.cuda.synchronize()
    pkg.counts_to_offsets(c_d.data_ptr(), m, off_d.data_ptr())
    torch.cuda.synchronize()
    got = host_u64(off_d)
    np.testing.assert_array_equal(got[:m + 1], want)
    assert got[m + 1] == 0x1111111111111111


def test_offsets_of_zeros_and_on_a_stream():
    m = 300
    c_d = dev_counts(m, fill=0)
    off_d = dev_u64(np.full(m + 1, 7, dtype=np.uint64))
    s = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    pkg.counts_to_offsets(c_d.data_ptr(), m, off_d.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (host_u64(off_d) == 0).all()


LENGTHS = [0, 1, 2, 63, 64, 65, 4096, 4097, 10000]


def _segments(rng, rooms):
    """Back-to-back segments of the given rooms and one entry behind the last that belongs to nobody; random keys with many
    repeated values."""
    offsets = np.zeros(len(rooms) + 1, dtype=np.uint64)
    for j, r in enumerate(rooms):
        offsets[j + 1] = offsets[j] + np.uint64(r)
    keys = rng.integers(0, 50, int(offsets[-1]) + 1).astype(np.uint64) << np.uint64(32) | rng.integers(0, 4, int(offsets[-1]) + 1).astype(np.uint64)
    return offsets, keys


@pytest.mark.parametrize("how", ["equal", "below", "above"])
def test_the_sort_on_every_length_in_one_call(how):
    """fill equal to the room, below it (the entries beyond keep their bytes) and above it (an overflowed segment: the room is sorted)."""
    rng = np.random.default_rng(11)
    rooms = LENGTHS + LENGTHS[::-1]
    if how == "below":                       # the sorted part has the lengths of the list, the rooms are larger
        rooms = [r + 1 + (r % 5) for r in rooms]
    offsets, keys = _segments(rng, rooms)
    want_len = LENGTHS + LENGTHS[::-1]
    fill = np.array(want_len if how != "above" else [r + 1 + 3 * (r % 4) for r in rooms], dtype=np.uint32)
    if how == "above":
        fill[2] = 0xFFFFFFFF
    assert len(set(keys.tolist())) < 250 < keys.size      # repeated values: equal keys meet in every comparator
    got = sorted_on_device(len(rooms), offsets, fill, keys)
    want = keys.copy()
    for j in range(len(rooms)):
        a = int(offsets[j])
        c = min(int(fill[j]), int(offsets[j + 1] - offsets[j]))
        want[a:a + c] = np.sort(keys[a:a + c])
    np.testing.assert_array_equal(got, want)
    assert sorted(min(int(f), r) for f, r in zip(fill, rooms)) == sorted(want_len)


def test_the_sort_leaves_gaps_and_neighbours_alone():
    """Offsets that skip entries between segments (a caller's own layout) and a segment whose fill is 0 in the middle: only
    [offsets[j], offsets[j] + min(fill, room)) changes.  A descending pair of offsets has no room."""
    rng = np.random.default_rng(12)
    offsets = np.array([5, 70, 70, 4200, 9000, 8000, 20000], dtype=np.uint64)     # (segment 4 descends: no room)
    fill = np.array([60, 9, 4096, 0, 50, 11000], dtype=np.uint32)
    keys = rng.integers(0, 1 << 62, 20010).astype(np.uint64)
    keys[4300:4400] = keys[4300]
    got = sorted_on_device(6, offsets, fill, keys)
    want = keys.copy()
    want[5:65] = np.sort(keys[5:65])
    want[70:70 + 4096] = np.sort(keys[70:70 + 4096])
    want[8000:19000] = np.sort(keys[8000:19000])
    np.testing.assert_array_equal(got, want)
