"""The reference's DisenGCN layer on this library's fused neighbourhood routing (cogdl_amd/operators/disen.py):
`install(disengcn=True)` binds `DisenGCNLayer.forward` (cogdl/layers/disengcn_layer.py:40-91).

What changes: lines 46-71 of the reference -- split into channels, normalise, and per iteration two [E, K, d] gathers, their
product and reduction, edge_softmax with K heads, a third gather, the scaling, an int64 [K, E, d] index and scatter_add_ (float
atomics on a GPU), all kept by autograd for every iteration -- are one `neighbor_routing` call: per iteration one operator
whose forward and backward write nothing of size [E, .], no atomics, equal from run to run.  The softmax is an online softmax
with the row maximum carried, so the sums are re-associated against the reference's: the same numbers up to float32 rounding,
not the same bits.  The features stay in the [N, K d] layout of the matmul: no split, cat or permute.

What does not: the matmul, the bias and the activation are the reference's line 44.  The reference's own forward
(cogdl_amd/_rebind.original) is called
  * for a graph that holds no CSR when the layer is entered: the reference's edge_softmax then builds one in the middle of the
    layer, which re-sorts the graph's edges under the edge list the loop already holds;
  * for a graph whose CSR does not describe its edge_index (see cogdl_amd/genconv_compat.py: the reference softmaxes over the
    row pointer's segments and scatters by edge_index[0], a pairing no aggregation reproduces);
  * for an x that is not 2-D and for an out_feats that K does not divide (the reference's split then makes more than K
    channels): left to the reference's forward, whatever it does with them.
"""
import sys

import torch

from . import _rebind
from .genconv_compat import _csr_describes
from .operators.disen import neighbor_routing

_MODULE, _CLASS = "cogdl.layers.disengcn_layer", "DisenGCNLayer"


def _served(self, graph, x):
    if x.dim() != 2 or self.weight.shape[1] != self.K * self.factor_dim:
        return False
    row_ptr = getattr(getattr(graph, "_adj", None), "row_ptr", None)
    if row_ptr is None:
        return False
    row = graph.edge_index[0]  # (a graph built from its CSR expands the row pointer here, as the reference's line 55 would)
    return _csr_describes(row, row_ptr, x.shape[0])


def forward(self, graph, x):
    if not _served(self, graph, x):
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, graph, x)
    h = self.activation(torch.matmul(x, self.weight) + self.bias)
    row, col = graph.edge_index
    return neighbor_routing(h, row, col, self.K, self.iterations, self.tau)


def install():
    _rebind.put("disengcn", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    return True
