"""knn_index_self_cluster_within_routed — what its GPU tests share (test infrastructure): the call itself with poisoned outputs, as
tests/cluster_helper.run_cluster makes 2m's."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

from tests.count_helper import dev


def run_cluster_routed(ix, max_dist2, min_pts, want_core=True, slot=0, stream=0, sync=True, **flags):
    """One call: (labels int32 [n], core words uint32 [(n + 31) // 32] or None, last_stats) — outputs poisoned first.  sync False:
    the device tensors as they are, nothing waited for (the caller synchronises), and no statistics."""
    n = ix.n
    labels = torch.full((n,), -7, dtype=torch.int32, device=dev())
    core = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev()) if want_core else None
    torch.cuda.synchronize()
    ix.self_cluster_within_routed(max_dist2, min_pts, labels.data_ptr(), core_dev=core.data_ptr() if want_core else None, slot=slot,
                                  stream=stream, **flags)
    if not sync:
        return labels, core, None
    torch.cuda.synchronize()
    st = ix.last_stats()
    return labels.cpu().numpy(), (core.cpu().numpy().view(np.uint32) if want_core else None), st


def core_flags(words, n):
    """The mask's words as bool [n]."""
    return np.unpackbits(np.asarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)
