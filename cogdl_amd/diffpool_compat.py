"""The reference's DiffPool pooling layer on this library's ragged segment GEMMs (cogdl_amd/operators/segmm.py):
`install(diffpool=True)` binds `BatchedDiffPoolLayer.forward` (cogdl/models/nn/diffpool.py:152-180).

What changes: the reference builds a [N, B * K] block mask on the CPU with scipy's block_diag from a Python loop over the graphs,
runs two softmaxes of that size, multiplies [B * K, N] x [N, F] and [B * K, N] x [N, B * K] matrices that are zero outside one
[K, n_g] block per graph, and for the link loss materialises adj.to_dense() and result @ result.t() as [N, N].  Here
  S        the softmax of each node's own K-column block of `pooled`, gathered as [N, K];
  h, adj_blocks, gram   one `diffpool_coarsen` call: y = A S on csrspmm, then S_g^T embed_g, S_g^T y_g and S_g^T S_g for every
           graph from one three-panel segment_matmul_tn launch;
  adj_new  [B * K, B * K] with adj_blocks on the diagonal and exact zeros elsewhere (the reference's off-diagonal blocks are exact
           zeros too, and toBatchedGraph reads only the diagonal);
  adj_loss sqrt(max(|A|_F^2 - 2 SUM_g tr(adj_blocks_g) + SUM_g |gram_g|_F^2, 0)) / N^2 = |A - S S^T|_F / N^2, the three sums and
           the subtraction in float64; |A|_F^2 over the coalesced entries, without gradient.
Nothing of size [N, N] or [N, B * K] beyond the model's own logits, nothing through the host.  `embed`, `pooled`, the entropy
loss, the keys of loss_dict and the return order (adj_new, h) are the reference's lines.

Deviations from the reference's numbers: (1) it divides the masked softmax by its row sum + 1e-13, here the block softmax is
exact; (2) the sums are re-associated (per-graph MFMA tiles, float64 for the three scalars of the link loss, whose difference
cancels where the reference subtracts entry by entry); (3) N is x.shape[0], where the reference lets sparse_coo_tensor infer it
from the largest node id that occurs in an edge (and fails in the matrix product when trailing nodes have no edge); (4) no CPU
or scipy step.

The reference's own forward (cogdl_amd/_rebind.original) is called, and raises where it raised before, for: a `pooled` width
that the number of graphs does not divide; a `batch` that is not sorted; an edge_weight that requires grad; an x that is not 2-D
float32; a graph whose CSR does not describe its edge_index (the check of cogdl_amd/genconv_compat.py); and an edge between two
graphs of the batch, whose contribution the per-graph blocks could not hold.
"""
import collections
import sys

import torch
import torch.nn.functional as F

from . import _rebind
from .genconv_compat import _csr_describes
from .operators.segmm import diffpool_coarsen
from .plan import tensor_key

_MODULE, _CLASS = "cogdl.models.nn.diffpool", "BatchedDiffPoolLayer"

# (batch, row, col) -> is batch sorted, and does every edge stay inside one graph?  Memoised on the tensors' identity, which the
# entry keeps alive: one read-back per batch object
_BATCHED = collections.OrderedDict()
_MAX_BATCHED = 16


def _batch_describes(batch, row, col):
    key = tensor_key(batch) + tensor_key(row) + tensor_key(col)
    hit = _BATCHED.get(key)
    if hit is None:
        ok = batch.dim() == 1 and bool((batch[1:] >= batch[:-1]).all()) and bool((batch[row] == batch[col]).all())
        hit = (ok, batch, row, col)
        _BATCHED[key] = hit
        while len(_BATCHED) > _MAX_BATCHED:
            _BATCHED.popitem(last=False)
    else:
        _BATCHED.move_to_end(key)
    return hit[0]


def clear_plans():
    _BATCHED.clear()


def _reference(self, graph, x, batch):
    return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, graph, x, batch)


def forward(self, graph, x, batch):
    if x.dim() != 2 or x.dtype != torch.float32 or batch.numel() != x.shape[0] or x.shape[0] == 0:
        return _reference(self, graph, x, batch)
    embed = self.embd_gnn(graph, x)
    pooled = F.softmax(self.pool_gnn(graph, x), dim=-1)
    value_set, seg, value_counts = torch.unique(batch, return_inverse=True, return_counts=True)
    batch_size = len(value_set)
    row_ptr = getattr(getattr(graph, "_adj", None), "row_ptr", None)
    row, col = graph.edge_index
    weight = graph.edge_weight
    if (pooled.size(1) % batch_size != 0 or weight.requires_grad or row_ptr is None
            or not _csr_describes(row, row_ptr, x.shape[0]) or not _batch_describes(batch, row, col)):
        # (the two SAGE layers run again there: they hold no state, and these are the cases the reference mostly raises for)
        return _reference(self, graph, x, batch)
    k = pooled.size(1) // batch_size
    ptr = torch.zeros(batch_size + 1, dtype=torch.int64, device=x.device)
    ptr[1:] = torch.cumsum(value_counts, 0)
    own = seg.unsqueeze(1) * k + torch.arange(k, device=x.device)
    s = F.softmax(pooled.gather(1, own), dim=-1)

    h, adj_blocks, gram = diffpool_coarsen(row_ptr, col, weight.to(torch.float32), s, embed, ptr)
    adj_new = torch.block_diag(*adj_blocks)

    if self.use_link_pred:
        adj = torch.sparse_coo_tensor(torch.stack([row, col]), weight.detach(), (x.shape[0], x.shape[0])).coalesce()
        a2 = adj.values().double().pow(2).sum()
        cross = torch.diagonal(adj_blocks, dim1=1, dim2=2).double().sum()
        g2 = gram.double().pow(2).sum()
        adj_loss = (torch.sqrt(torch.clamp(a2 - 2 * cross + g2, min=0)) / float(len(batch)) ** 2).to(x.dtype)
        self.loss_dict["adj_loss"] = adj_loss
    entropy_loss = (torch.distributions.Categorical(probs=pooled).entropy()).mean()
    assert not torch.isnan(entropy_loss)
    self.loss_dict["entropy_loss"] = entropy_loss
    return adj_new, h


def install():
    _rebind.put("diffpool", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    return True
