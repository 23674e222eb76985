"""numpy restatement of knn_index_self_cluster_within (include/knn_mi355x.h 2m) — test infrastructure, numpy only.

The definition, word for word: deg(i) = rows j != i (by local row number) with a finite v0 distance E(i, j) <= max_dist2; row i is
core when deg(i) + 1 >= min_pts; two core rows within the radius share a cluster, whose label is the smallest core row of the
connected component; a row that is not core takes the label of the core row with the smallest key (E's bits, row) within its
radius; every other row is noise (-1).  EVERY pair decision goes through tests.topk_oracle.v0_dist2.

For larger shards the pairs are pruned first: rows are sorted along axis 0 in float64 and a block of rows meets only the rows
whose first coordinate lies within the radius of the block's span, widened by a margin.  The pruning never decides a pair: it
only leaves out pairs that cannot pass — computed in fp32, E >= (a_0 - b_0)^2 (1 - 2^-24)^3 (a rounding for the difference, one
for the square, one per addition of non-negative terms), so a pair with E <= max_dist2 has |a_0 - b_0| <= sqrt(max_dist2) (1 +
2^-22), far inside the margin of 1e-3 of the radius (and 1e-30 absolute) — and whatever it lets through is decided by v0_dist2.
Rows with a non-finite coordinate are outside the sort: they meet, and are met by, every row."""
import numpy as np

from tests.topk_oracle import v0_dist2

NOISE = -1


def _pairs(R, k, max_dist2, block=256):
    """(a, b, bits): every ordered pair a != b with a finite v0 distance <= max_dist2, and that distance's bits."""
    R = np.asarray(R, dtype=np.float32).reshape(-1, k)
    n = R.shape[0]
    cap = np.float32(max_dist2)
    fin = np.isfinite(R).all(axis=1)
    rows_fin, rows_bad = np.flatnonzero(fin), np.flatnonzero(~fin)
    x0 = R[rows_fin, 0].astype(np.float64)
    order = np.argsort(x0, kind="stable")
    srt, x0s = rows_fin[order], x0[order]
    rad = float(np.sqrt(np.float64(cap))) if np.isfinite(cap) else np.inf
    reach = rad * (1.0 + 1e-3) + 1e-30
    out_a, out_b, out_bits = [], [], []

    def decide(qrows, crows):
        if qrows.size == 0 or crows.size == 0:
            return
        d = v0_dist2(R[qrows], R[crows], k)
        hit = (d < np.float32(np.inf)) & (d <= cap) & (qrows[:, None] != crows[None, :])
        qi, ci = np.nonzero(hit)
        out_a.append(qrows[qi])
        out_b.append(crows[ci])
        out_bits.append(d[qi, ci].view(np.uint32))

    for b0 in range(0, srt.size, block):
        q = srt[b0:b0 + block]
        lo = np.searchsorted(x0s, x0s[b0] - reach, side="left")
        hi = np.searchsorted(x0s, x0s[min(b0 + block, srt.size) - 1] + reach, side="right")
        decide(q, np.concatenate([srt[lo:hi], rows_bad]))
    decide(rows_bad, np.arange(n))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(out_a, np.int64), cat(out_b, np.int64), cat(out_bits, np.uint32)


def components(n, a, b):
    """Plain numpy union-find by label propagation: lab[x] = the smallest member of x's component under the edges (a, b)."""
    lab = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        while True:
            jumped = new[new]
            if (jumped == new).all():
                break
            new = jumped
        if (new == lab).all():
            return lab
        lab = new


def cluster(R, k, max_dist2, min_pts):
    """dict(labels int32 [n] (the device call's: representative LOCAL rows, -1 noise), core bool [n], deg int64 [n])."""
    R = np.asarray(R, dtype=np.float32).reshape(-1, k)
    n = R.shape[0]
    a, b, bits = _pairs(R, k, max_dist2)
    deg = np.bincount(a, minlength=n).astype(np.int64)
    core = deg + 1 >= int(min_pts)
    both = core[a] & core[b]
    lab = components(n, a[both], b[both])
    labels = np.where(core, lab, NOISE).astype(np.int64)
    # border rows: the smallest key (distance bits, row) of a core row within the radius
    sel = ~core[a] & core[b]
    keys = (bits[sel].astype(np.uint64) << np.uint64(32)) | b[sel].astype(np.uint64)
    best = np.full(n, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    np.minimum.at(best, a[sel], keys)
    border = best != np.uint64(0xFFFFFFFFFFFFFFFF)
    labels[border] = lab[(best[border] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    return dict(labels=labels.astype(np.int32), core=core, deg=deg, border=border)


def renumber(labels):
    """The host form's numbering: clusters 0 .. C - 1 in ascending order of their representative row; noise stays -1."""
    labels = np.asarray(labels, dtype=np.int64)
    reps = np.unique(labels[labels >= 0])
    out = np.full(labels.shape, NOISE, dtype=np.int32)
    out[labels >= 0] = np.searchsorted(reps, labels[labels >= 0]).astype(np.int32)
    return out


def core_mask_words(core):
    """The core flags as the device's mask: (n + 31) // 32 uint32 words, bit i % 32 of word i // 32, spare bits 0."""
    core = np.asarray(core, dtype=bool)
    pad = np.zeros((core.size + 31) // 32 * 32, dtype=np.uint8)
    pad[:core.size] = core
    return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
