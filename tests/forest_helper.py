"""knn_index_self_forest_within — what its GPU tests share (test infrastructure): the call itself with poisoned outputs, the bar
every call is held to, and the rows with many equal distances.  Expectations always come from tests/forest_oracle.py."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

from tests import forest_oracle as fo
from tests.count_helper import dev

POISON64, POISON32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


class Outputs:
    """The four device arrays of one call, poisoned."""

    def __init__(self, n):
        self.n = n
        self.labels = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev())
        self.keys = torch.full((max(n, 1),), POISON64, dtype=torch.int64, device=dev())
        self.his = torch.full((max(n, 1),), POISON32, dtype=torch.int32, device=dev())
        self.count = torch.full((2,), 77, dtype=torch.int32, device=dev())

    def call(self, ix, max_dist2, slot=0, stream=0, **flags):
        ix.self_forest_within(max_dist2, self.labels.data_ptr(), self.keys.data_ptr(), self.his.data_ptr(), self.count.data_ptr(),
                              stream=stream, slot=slot, **flags)

    def read(self):
        """(labels int32 [n], table (bits, lo, hi) sorted, count [2]); the entries beyond count[0] must have kept their poison."""
        n = self.n
        count = self.count.cpu().numpy().view(np.uint32).tolist()
        e = count[0]
        assert e <= max(n - 1, 0), count
        keys = self.keys.cpu().numpy().view(np.uint64)
        his = self.his.cpu().numpy().view(np.uint32)
        assert (keys[e:] == np.uint64(POISON64)).all() and (his[e:] == np.uint32(POISON32)).all()
        assert count[1] <= fo.rounds_of(n), count
        return self.labels.cpu().numpy()[:n], fo.edge_table(keys[:e], his[:e]), count


def run_forest(ix, max_dist2, slot=0, **flags):
    """One call: (labels, table, count, last_stats)."""
    out = Outputs(ix.n)
    torch.cuda.synchronize()
    out.call(ix, max_dist2, slot=slot, **flags)
    torch.cuda.synchronize()
    st = ix.last_stats()
    return out.read() + (st,)


def assert_forest(labels, table, want):
    """Sorted edges == the oracle's, none twice, i < j; labels == the oracle's."""
    np.testing.assert_array_equal(table, fo.want_table(want))
    assert len(np.unique(table, axis=0)) == len(table) and (table[:, 1] < table[:, 2]).all()
    np.testing.assert_array_equal(labels, want["labels"])
    assert len(table) == len(labels) - np.unique(labels).size


def walks(n, k, rng, steps=(-1.0, 1.0)):
    """n integer-lattice rows in k dimensions: random walks of unit steps that restart from an earlier row now and then, in
    shuffled row order.  Consecutive rows of a walk lie at E == 1 exactly, revisits are duplicates, every squared distance is a
    small integer: ties everywhere, at every radius."""
    R = np.zeros((n, k), dtype=np.float32)
    for t in range(1, n):
        src = t - 1 if rng.random() < 0.9 else int(rng.integers(0, t))
        R[t] = R[src]
        R[t, int(rng.integers(0, k))] += np.float32(rng.choice(steps))
    return R[rng.permutation(n)]
