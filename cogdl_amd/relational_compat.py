"""The reference's CompGCN layer on this library's relational operator (cogdl_amd/operators/relational.py):
`install(relational=True)` binds `CompGCNLayer.message_passing` (cogdl/models/nn/compgcn.py:124-140).

What changes: the reference gathers x[col] and rel_embed[edge_types] into two [E, in] tensors, combines them, multiplies the
[E, in] result by the direction's weight into [E, out], scales it per edge and scatter_add_s it (float atomics on a GPU).
The weight is shared by every edge of a direction, so  sum_e n_e (comp_e W) = (sum_e n_e comp_e) W:  the layer is one typed
aggregation to [N, in] (rel_gspmm: no [E, *] tensor, no atomics, equal from run to run) and one [N, in] x [in, out] matmul.
The sums are therefore re-associated against the reference's -- the same numbers up to float32 rounding, not the same bits.

What does not: `opn` "sub" and "mult" are served; any other composition reaches the reference's own method
(cogdl_amd/_rebind.original), which raises for it as before.  The reference's RGCNLayer is not served: its basis_forward
returns from inside the loop over the edge types after the first one and aggregates over the whole graph
(cogdl/layers/rgcn_layer.py:134-149), so there is no sound behaviour to reproduce.
"""
import sys

import torch.nn.functional as F

from . import _rebind
from .operators.relational import rel_gspmm

_MODULE, _CLASS = "cogdl.models.nn.compgcn", "CompGCNLayer"
_OPN = {"sub": "sub", "mult": "mul"}  # CompGCNLayer.rel_transform (compgcn.py:142-151)


def message_passing(self, x, rel_embed, edge_index, edge_types, mode, edge_weight=None):
    op = _OPN.get(self.opn)
    if op is None:
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "message_passing")(
            self, x, rel_embed, edge_index, edge_types, mode, edge_weight)
    weight = getattr(self, "weight_%s" % mode)
    embed = rel_gspmm(x, rel_embed, edge_index[0], edge_index[1], edge_types, edge_weight, op, num_nodes=x.shape[0]) @ weight
    return F.dropout(embed, p=self.dropout, training=self.training)


def install():
    _rebind.put("relational", getattr(sys.modules[_MODULE], _CLASS), "message_passing", message_passing)
    return True
