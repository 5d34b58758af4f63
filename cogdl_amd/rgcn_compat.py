"""The reference's RGCNLayer on this library's RGCN operators (cogdl_amd/operators/rgcn.py): `install(rgcn=True)` binds
`RGCNLayer.basis_forward` and `RGCNLayer.bdd_forward` (cogdl/layers/rgcn_layer.py:118-168).  Both return a one-element list,
so the rest of `RGCNLayer.forward` -- the sum, dropout, layer norm, bias and self loop -- runs unchanged.

The reference's two methods do not compute a layer as they stand; what they were written to compute is the law of the paper,

    h[v] = sum over the edges e with row[e] == v of  n_e * x[col[e]] @ W[type[e]]            n_e = w_e / (sum of w over row v)

and that law is what is served.  Every deviation from the reference's text:

  * basis_forward returns from inside its loop over the edge types after the first type that has an edge
    (rgcn_layer.py:149); here every type contributes.
  * basis_forward aggregates h[edge_t] over the WHOLE graph (`spmm(graph, ..)`, rgcn_layer.py:147; the per-type graph `g` it
    builds, with padded self loops of weight 0.01, is never used); here a type's weight meets that type's edges only.
  * basis_forward reads `graph.edge_weight` before it calls `graph.row_norm()` (rgcn_layer.py:128-130), i.e. the weights of
    the call before; here the row-normalised weights of this call are used.
  * bdd_forward calls `row_normalization(x.shape[0], edge_index, edge_weight)` and `spmm(_edge_index_t, weight, h_t)`
    (rgcn_layer.py:157,165) -- neither function has that signature, the method raises; here n_e = 1 / (edges of row[e]).
  * the sums are re-associated: basis is sum_b (sum_e n_e alpha[t_e, b] x[col_e]) V[b] -- one aggregation to [N, B, in] and one
    [N, B * in] x [B * in, out] matmul instead of [R, N, out] and one spmm per type -- and bdd multiplies the SUM of a
    (row, type) run by the type's blocks instead of an einsum over all nodes and one spmm per type.  Float32 rounding apart,
    the same numbers as the law; HIP kernels for CUDA tensors (no float atomics, equal from run to run), the torch
    composition on the CPU.

A graph without `edge_attr` reaches the reference's own method, which raises what it always raised.
"""
import sys

import torch

from . import _rebind
from .operators.rgcn import rgcn_basis_aggregate, rgcn_bdd_aggregate

_MODULE, _CLASS = "cogdl.layers.rgcn_layer", "RGCNLayer"


def _reference(name):
    return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), name)


def basis_forward(self, graph, x):
    edge_type = graph.edge_attr
    if edge_type is None:
        return _reference("basis_forward")(self, graph, x)
    row, col = graph.edge_index
    graph.row_norm()
    alpha = self.alpha if self.num_bases < self.num_edge_types else None
    z = rgcn_basis_aggregate(x, alpha, row, col, edge_type.long(), graph.edge_weight, num_nodes=x.shape[0],
                             num_types=self.num_edge_types)
    return [z.reshape(x.shape[0], -1) @ self.weight.view(-1, self.out_feats)]


def bdd_forward(self, graph, x):
    edge_type = graph.edge_attr
    if edge_type is None:
        return _reference("bdd_forward")(self, graph, x)
    row, col = graph.edge_index
    norm = torch.bincount(row, minlength=x.shape[0]).to(x.dtype).reciprocal()[row]
    blocks = self.weight.view(self.num_edge_types, self.num_bases, self.block_in_feats, self.block_out_feats)
    return [rgcn_bdd_aggregate(x, blocks, row, col, edge_type.long(), norm, num_nodes=x.shape[0])]


def install():
    cls = getattr(sys.modules[_MODULE], _CLASS)
    _rebind.put("rgcn", cls, "basis_forward", basis_forward)
    _rebind.put("rgcn", cls, "bdd_forward", bdd_forward)
    return True
