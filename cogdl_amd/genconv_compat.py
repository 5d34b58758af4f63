"""The reference's GENConv layer (DeeperGCN, RevGCN) on this library's fused aggregation (cogdl_amd/operators/genaggr.py):
`install(genconv=True)` binds `GENConv.forward` (cogdl/layers/deepergcn_layer.py:64-102).

What changes: lines 67-93 of the reference -- gather x[col] into [E, F], add the encoded edge features, relu + eps, beta *,
edge_softmax with one channel per column, multiply, scatter_add_ (float atomics on a GPU) -- are one `gen_aggregate` call:
no [E, F] tensor beyond the encoded edge features the layer itself computes, no atomics, equal from run to run.  The softmax
is an online softmax with the row maximum carried, so the sums are re-associated against the reference's -- the same numbers
up to float32 rounding, not the same bits -- and large beta * m neither overflows nor goes through the halving loop of the
reference's CPU softmax (cogdl/utils/spmm_utils.py:157-160).  `softmax_sg` uses the layer's beta parameter, `softmax` beta = 1,
`mean` the reference's 1 / deg with 0 for an empty row, every other name the plain sum, as the reference's `else` branch.

What does not: the edge encoder, message_norm, the residual and the MLP are the reference's lines.  The reference's own forward
(cogdl_amd/_rebind.original) is called
  * for the aggregators `powermean` and `max` (`max` is served by install(readout=True));
  * for an x that is not 2-D (left to the reference's forward, whatever it does with it);
  * for a graph that holds no CSR when the layer is entered: the reference's edge_softmax then builds one in the middle of the
    layer, which re-sorts the graph's edges under the messages already gathered;
  * for a graph whose CSR does not describe its edge_index (Graph.edge_index was assigned an edge list of the same length,
    which keeps the old row pointer, data.py:628-639; or the rows are not in CSR order): the reference softmaxes over the row
    pointer's segments and scatters by edge_index[0], and that pairing is not an aggregation this operator could reproduce.
"""
import collections
import sys

import torch

from . import _rebind
from .operators.genaggr import gen_aggregate
from .plan import tensor_key

_MODULE, _CLASS = "cogdl.layers.deepergcn_layer", "GENConv"
_ORIGINAL_ONLY = ("powermean", "max")

# (row, row_ptr) -> does the row pointer describe these rows?  Memoised on the identity of both tensors (which the entry keeps
# alive, so an address cannot be recycled under the same key): one read-back per graph, none on a later call.
_PAIRED = collections.OrderedDict()
_MAX_PAIRED = 16


def _csr_describes(row, row_ptr, num_nodes):
    key = tensor_key(row) + tensor_key(row_ptr) + (num_nodes,)
    hit = _PAIRED.get(key)
    if hit is None:
        ok = row_ptr.dim() == 1 and row_ptr.numel() == num_nodes + 1 and row.dim() == 1
        if ok and row.numel() > 0:
            ok = bool((row[1:] >= row[:-1]).all()) and int(row.min()) >= 0 and int(row.max()) < num_nodes
        if ok:
            counts = torch.bincount(row, minlength=num_nodes)
            ok = bool(int(row_ptr[0]) == 0 and torch.equal(row_ptr[1:].long() - row_ptr[:-1].long(), counts))
        hit = (ok, row, row_ptr)
        _PAIRED[key] = hit
        while len(_PAIRED) > _MAX_PAIRED:
            _PAIRED.popitem(last=False)
    else:
        _PAIRED.move_to_end(key)
    return hit[0]


def clear_plans():
    _PAIRED.clear()


def _served(self, graph, x):
    if self.aggr in _ORIGINAL_ONLY or x.dim() != 2:
        return False
    row_ptr = getattr(getattr(graph, "_adj", None), "row_ptr", None)
    if row_ptr is None:
        return False
    row = graph.edge_index[0]  # (a graph built from its CSR expands the row pointer here, as the reference's line 65 would)
    return _csr_describes(row, row_ptr, x.shape[0])


def forward(self, graph, x):
    if not _served(self, graph, x):
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, graph, x)
    row, col = graph.edge_index
    eterm = None
    if self.edge_encoder is not None and graph.edge_attr is not None:
        eterm = self.edge_encoder(graph.edge_attr)
    if self.aggr == "softmax_sg":
        aggr, beta = "softmax", self.beta
    elif self.aggr == "softmax":
        aggr, beta = "softmax", None
    else:
        aggr, beta = ("mean" if self.aggr == "mean" else "sum"), None
    h = gen_aggregate(x, row, col, eterm, aggr, beta, self.eps, num_nodes=x.shape[0])
    if self.use_msg_norm:
        h = self.message_norm(x, h)
    if self.residual:
        h = h + x
    return self.mlp(h)


def install():
    _rebind.put("genconv", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    return True
