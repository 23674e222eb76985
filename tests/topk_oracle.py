"""numpy restatement of v0 for top-K (test infrastructure): the K smallest packed keys per query.

v0's distance (reference core.cu:44-49) is float32 d = d + (q_j - r_j)^2 accumulated in dimension order, one rounding per
operation; numpy evaluates each of these element-wise float32 operations on its own (it never fuses), so the restatement is
exact.  Keys are (float bits of d << 32) | global index, sorted as uint64; only rows whose distance is finite are candidates
(v0's strict `<` against +INF), and slots beyond them hold KEY_INIT = (+INF, 0)."""
import numpy as np

KEY_INIT = np.uint64(0x7F80000000000000)


def v0_dist2(Q, R, k):
    """float32 [m][n] squared distances with v0's arithmetic."""
    Q = np.asarray(Q, dtype=np.float32).reshape(-1, k)
    R = np.asarray(R, dtype=np.float32).reshape(-1, k)
    d = np.zeros((Q.shape[0], R.shape[0]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            diff = Q[:, j:j + 1] - R[None, :, j]
            d = d + diff * diff
    return d


def topk_keys(Q, R, k, K, gids=None, base=0, chunk=64):
    """uint64 [m][K]: the K smallest keys of each query, ascending; gids[row] (or base + row) is a row's global number."""
    Q = np.asarray(Q, dtype=np.float32).reshape(-1, k)
    R = np.asarray(R, dtype=np.float32).reshape(-1, k)
    n = R.shape[0]
    g = (np.arange(n, dtype=np.uint64) + np.uint64(base)) if gids is None else np.asarray(gids).astype(np.uint64)
    out = np.full((Q.shape[0], K), KEY_INIT, dtype=np.uint64)
    for c0 in range(0, Q.shape[0], chunk):
        d = v0_dist2(Q[c0:c0 + chunk], R, k)
        keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | g[None, :]
        keys[~(d < np.float32(np.inf))] = np.uint64(0xFFFFFFFFFFFFFFFF)   # NaN / +INF: never a candidate
        if n > K:
            keys = np.partition(keys, K - 1, axis=1)[:, :K]
        keys = np.sort(keys, axis=1)
        t = min(K, keys.shape[1])
        part = keys[:, :t]
        part[part == np.uint64(0xFFFFFFFFFFFFFFFF)] = KEY_INIT
        out[c0:c0 + chunk, :t] = part
    return out


def keys_dist2(keys):
    return (np.asarray(keys, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


def keys_index(keys):
    return (np.asarray(keys, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
