"""Radius-bounded top-K (knn_index_query_topk_within) — what its GPU tests share (test infrastructure): the expectation, always
built from tests/topk_oracle.py — `want = topk_keys(...)` with the entries whose distance exceeds the radius set to KEY_INIT —, the
radii, taken from the oracle's distances, and the call itself."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

from tests.topk_oracle import KEY_INIT, keys_dist2, keys_index

INF = np.float32(np.inf)
KS = (1, 8, 17, 64)


def clip(want, r2):
    """want with every entry beyond the radius (fp32 compare, equality inside) set to KEY_INIT."""
    out = np.array(want, dtype=np.uint64, copy=True)
    out[keys_dist2(out) > np.float32(r2)] = KEY_INIT
    return out


def lengths(want, r2):
    return (clip(want, r2) != KEY_INIT).sum(axis=1)


def kinds(want, r2):
    """(some list is empty, some holds between 1 and K - 1 entries, some is full) at this radius."""
    n, K = lengths(want, r2), want.shape[1]
    return bool((n == 0).any()), bool(((n > 0) & (n < K)).any()), bool((n == K).any())


def radii(want, need_partial=None):
    """The radii a test runs, from the oracle's lists want [m][K]: a value some row holds exactly (the boundary is inside), the
    next float below it (that row outside), 0, +INF and a radius below every distance.  The first two are chosen so that the
    expectation has empty lists, lists of 1 .. K - 1 entries (K > 1) and full lists among the queries — checked here, on the CPU:
    a clip that is wrong for one kind of list must not hide behind a batch that has none of that kind."""
    K = want.shape[1]
    if need_partial is None:
        need_partial = K > 1
    d = keys_dist2(want)
    held = np.unique(d[d < INF])
    assert held.size, "no query has a finite distance"
    order = np.argsort(np.abs(np.arange(held.size) - held.size // 2), kind="stable")   # from the median outwards
    at = None
    for v in held[order]:
        below = np.nextafter(v, np.float32(0))
        ok = [kinds(want, r) for r in (v, below)]
        if all(e and (p or not need_partial) and f for e, p, f in ok):
            at = v
            break
    assert at is not None, "no radius gives empty, partial and full lists among the queries: change the batch"
    least = d[d < INF].min()
    assert least > 0, "a query coincides with a row: no radius is below every distance"
    under = np.float32(least * np.float32(0.5))
    assert (lengths(want, under) == 0).all() and (lengths(want, 0.0) == 0).all() and (clip(want, INF) == want).all()
    assert (clip(want, at) != clip(want, np.nextafter(at, np.float32(0)))).any()
    return [("at", float(at)), ("below", float(np.nextafter(at, np.float32(0)))), ("zero", 0.0), ("inf", float("inf")),
            ("under_all", float(under))]


def dev():
    return torch.device("cuda:0")


def dev_keys(m, K, fill=None):
    t = torch.empty(m * K, dtype=torch.int64, device=dev())
    if fill is not None:
        t.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.uint64).reshape(-1).view(np.int64)))
    return t


def host_keys(keys, m, K):
    return keys.cpu().numpy().view(np.uint64).reshape(m, K)


def within(ix, Q, K, r2, keys=None, init=True, slot=0, stream=0, **flags):
    """One call of query_topk_within: keys [m][K] (numpy uint64) after it; the indices it unpacked are those of the keys."""
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(dev())
    if keys is None:
        keys = dev_keys(m, K)
    ind = torch.full((m * K,), -7, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    ix.query_topk_within(m, K, q_d.data_ptr(), r2, keys.data_ptr(), init_keys=init, indices_dev=ind.data_ptr(), slot=slot,
                         stream=stream, **flags)
    torch.cuda.synchronize()
    got = host_keys(keys, m, K)
    np.testing.assert_array_equal(ind.cpu().numpy().reshape(m, K), keys_index(got))
    return got


def plain(ix, Q, K, keys=None, init=True, slot=0, **flags):
    """The same call without a radius (query_topk)."""
    Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
    m = Qf.size // ix.k
    q_d = torch.from_numpy(Qf).to(dev())
    if keys is None:
        keys = dev_keys(m, K)
    ix.query_topk(m, K, q_d.data_ptr(), keys.data_ptr(), init_keys=init, slot=slot, **flags)
    torch.cuda.synchronize()
    return host_keys(keys, m, K)
