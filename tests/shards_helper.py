"""N cell-range shards of one reference set on one GPU (test infrastructure): the flow a resident caller with several GPUs follows
— knn_geom_* from a sample, knn_geom_assign, knn_index_create_sharded per rank, the seed layer exported and attached — with the
exchange step as a minimum over the ranks' key arrays.  Shared by tests/test_shards_gpu.py and tests/test_filter_margin_gpu.py."""
import numpy as np
import torch  # imported BEFORE libknn_mi355x.so is dlopen'ed: one HIP runtime (torch's) per process

import multicore_hw2_amd as pkg


def _dev():
    return torch.device("cuda:0")


class Shards:
    """N cell-range shards of one reference set on one GPU."""

    def __init__(self, k, R_d, nranks, seed_tiles=0, attach=True, sample_rows=4096):
        n = R_d.shape[0]
        self.k, self.n, self.nranks = k, n, nranks
        stride = max(1, n // sample_rows)
        sample = R_d[::stride][:sample_rows].cpu().numpy()
        self.geom = pkg.KnnGeom(k, n, nranks, sample, seed_tiles)
        owner = torch.empty(n, dtype=torch.int32, device=_dev())
        self.geom.assign(R_d.data_ptr(), n, owner.data_ptr())
        torch.cuda.synchronize()
        self.owner = owner
        self.rows, self.gids, self.idx = [], [], []
        for r in range(nranks):
            g = torch.nonzero(owner == r).reshape(-1)                   # ascending global row numbers
            rows = R_d[g].contiguous()
            gids = g.to(torch.int32)
            self.rows.append(rows)
            self.gids.append(gids)
            self.idx.append(pkg.KnnIndex.sharded(self.geom, r, rows.data_ptr(), gids.data_ptr(), rows.shape[0]))
        self.layer = torch.zeros(self.geom.layer_bytes, dtype=torch.uint8, device=_dev())
        for ix in self.idx:
            ix.seed_export(self.layer.data_ptr())
        torch.cuda.synchronize()
        if attach:
            for ix in self.idx:
                ix.seed_attach(self.layer.data_ptr())

    def query(self, Q):
        Qf = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1)
        m = Qf.size // self.k
        q_d = torch.from_numpy(Qf).to(_dev())
        keys = torch.empty((self.nranks, m), dtype=torch.int64, device=_dev())
        for r, ix in enumerate(self.idx):
            ix.query_keys(m, q_d.data_ptr(), keys[r].data_ptr(), init_keys=True)
        torch.cuda.synchronize()
        stats = [ix.last_stats() for ix in self.idx]
        merged = keys.min(dim=0).values            # keys < 2^63 (distance bits of a non-negative float): int64 min == unsigned min
        return (merged & 0xFFFFFFFF).to(torch.int32).cpu().numpy(), keys, stats

    def close(self):
        for ix in self.idx:
            ix.close()
        self.geom.close()
