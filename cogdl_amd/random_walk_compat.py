"""`RandomWalker` with the interface of cogdl/utils/sampling.py:70-121 on this library's walk operators
(cogdl_amd/operators/walk.py): `install(random_walk=True)` binds it in place of the reference's class, whose walk is a
numba-jitted (or, without numba, interpreted) Python loop on the CPU.

Accepted graphs, as in the reference: a [2, E] edge-index tensor, a (row, col) tuple of tensors, a scipy sparse matrix.
The CSR is built with the library's own coo2csr_index; an edge index that lives on the GPU stays there, and so do the
walks until `walk` copies them back (it returns a numpy int64 array [len(start), walk_length], as the reference does);
`walk_tensor` returns the tensor on the graph's device without that copy.  `parallel` is accepted and ignored: every walk
runs in parallel.  Restart and dead-end rules: see cogdl_amd/operators/walk.py.
"""
import numpy as np
import torch

from .graph_build import coo2csr_index
from .operators import walk as _walk


class RandomWalker(object):
    def __init__(self, adj=None, num_nodes=None):
        self.indptr = None
        self.indices = None
        if adj is not None:
            self._build(adj, num_nodes)

    def _build(self, adj, num_nodes):
        if isinstance(adj, (torch.Tensor, tuple, list)):
            row, col = adj
            row, col = torch.as_tensor(row).long(), torch.as_tensor(col).long()
            if col.device != row.device:
                col = col.to(row.device)
            if num_nodes is None:
                num_nodes = int(max(row.max(), col.max())) + 1 if row.numel() else 0
            indptr, perm = coo2csr_index(row.contiguous(), col, int(num_nodes))
            self.indptr, self.indices = indptr, col[perm].contiguous()
        else:  # a scipy sparse matrix
            csr = adj.tocsr()
            self.indptr = torch.from_numpy(np.asarray(csr.indptr, dtype=np.int64))
            self.indices = torch.from_numpy(np.asarray(csr.indices, dtype=np.int64))

    def build_up(self, adj, num_nodes):
        if self.indptr is not None:
            return
        self._build(adj, num_nodes)

    @property
    def device(self):
        return self.indptr.device

    def _start(self, start):
        assert self.indptr is not None, "Please build the adj_list first"
        if not torch.is_tensor(start):
            start = torch.from_numpy(np.asarray(start).astype(np.int64, copy=False).reshape(-1))
        return start.to(device=self.indptr.device, dtype=torch.long)

    def walk_tensor(self, start, walk_length, restart_p=0.0, seed=None):
        """The walks as an int64 [len(start), walk_length] tensor on the graph's device."""
        return _walk.random_walk(self.indptr, self.indices, self._start(start), walk_length, restart_p, seed=seed)

    def walk(self, start, walk_length, restart_p=0.0, parallel=True, seed=None):
        return self.walk_tensor(start, walk_length, restart_p, seed=seed).cpu().numpy()

    def node2vec_walk(self, start, walk_length, p=1.0, q=1.0, seed=None):
        """Second-order walks (unweighted) as a tensor on the graph's device."""
        return _walk.node2vec_walk(self.indptr, self.indices, self._start(start), walk_length, p, q, seed=seed)
