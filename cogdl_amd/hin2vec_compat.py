"""The reference's Hin2vec model on this library's pair builder and scorer (cogdl_amd/operators/hin2vec.py):
`install(hin2vec=True)` binds `Hin2vec.forward` (cogdl/models/emb/hin2vec.py:173-220).

What changes: the whole forward.  The reference walks a networkx DiGraph in interpreted Python, builds the training rows with
a list append per walk position, hop and negative (a string join per positive, a rejection loop per negative), and scores a
batch through an [N, N] one-hot matrix and [B, N] x [N, d] products.  Here the CSR of the DiGraph is built on the device of
the run -- parallel edges count once, as DiGraph collapses them -- and cogdl_amd.embedding.hin2vec walks, builds the rows
and trains there.  The return value is the reference's: float32 numpy [num_node, hidden], row v for node v.

Opt-in, because the numbers are not the reference's: the draws are Philox's and torch's, not `random`'s and numpy's; relation
ids are the dense ranks of the type sequence, where the reference's `relation[meta_str] = len(meta_str)` gives every path of
one string length the same id and can index past Wr; `cpu=True` is honoured by keeping everything on the CPU (host twin and
torch composition), otherwise the run is on the GPU where there is one.  The per-batch loss.item() and the accuracy
bookkeeping are not reproduced.

What is not served reaches the reference's own forward (cogdl_amd/_rebind.original): a graph whose node ids are not exactly
0 .. N-1 all occurring in an edge, a `data.pos` that is not an integer list of types in [0, 64) covering every node,
hop > 8 (or < 1), walk_length <= hop, and a graph without edges.  A type with a single node raises BackendError (the reference
loops forever there).
"""
import sys

import torch

from . import _rebind
from .metapath_compat import digraph_csr

_MODULE, _CLASS = "cogdl.models.emb.hin2vec", "Hin2vec"
_MAX_TYPES, _MAX_HOP = 64, 8


def _served(self, data):
    row, col = data.edge_index
    if not torch.is_tensor(row) or row.numel() == 0 or row.is_floating_point():
        return None
    if not isinstance(self.hop, int) or not 1 <= self.hop <= _MAX_HOP or int(self.walk_length) <= self.hop:
        return None
    pos = getattr(data, "pos", None)
    if not torch.is_tensor(pos) or pos.dim() != 1 or pos.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
        return None
    ids = torch.unique(torch.cat([row.flatten(), col.flatten()]))
    n = ids.numel()
    if int(ids[0]) != 0 or int(ids[-1]) != n - 1 or pos.numel() < n:
        return None
    pos = pos[:n].long()
    if int(pos.min()) < 0 or int(pos.max()) >= _MAX_TYPES:
        return None
    return n, pos


def forward(self, data):
    served = _served(self, data)
    if served is None:
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, data)
    from . import embedding

    n, pos = served
    dev = torch.device("cpu" if self.cpu or not torch.cuda.is_available() else "cuda")
    row, col = data.edge_index
    indptr, indices, _ = digraph_csr(row.to(dev), col.to(dev), n)
    self.num_node = n
    emb = embedding.hin2vec((indptr, indices), pos.to(dev), dim=self.hidden_dim, walk_length=self.walk_length,
                            walk_num=self.walk_num, batch_size=self.batch_size, hop=self.hop, negative=self.negative,
                            epochs=self.epochs, lr=self.lr)
    return emb.cpu().numpy()


def install():
    _rebind.put("hin2vec", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    return True
