"""knn_index_count_within — what its GPU tests share (test infrastructure): the call itself.  Expectations always come from
tests/count_oracle.py."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process


def dev():
    return torch.device("cuda:0")


def dev_counts(m, fill=None):
    t = torch.empty(m, dtype=torch.int32, device=dev())
    if fill is not None:
        t.copy_(torch.from_numpy(np.array(np.broadcast_to(np.asarray(fill, dtype=np.uint32), (m,))).view(np.int32)))
    return t


def host_counts(t):
    return t.cpu().numpy().view(np.uint32)


def count(ix, Q, r2, counts=None, init=True, slot=0, stream=0, **flags):
    """One call of count_within: the counts [m] (numpy uint32) after it.  Without `counts` the call writes a buffer that held
    0xDEADBEEF (init) or zeros (a fold)."""
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(dev())
    if counts is None:
        counts = dev_counts(m, fill=0xDEADBEEF if init else 0)
    torch.cuda.synchronize()
    ix.count_within(m, q_d.data_ptr(), r2, counts.data_ptr(), init=init, slot=slot, stream=stream, **flags)
    torch.cuda.synchronize()
    return host_counts(counts)
