"""The reference's LINE model on this library's edge-sampled trainer (cogdl_amd/operators/line.py):
`install(line=True)` binds `LINE.forward` (cogdl/models/emb/line.py:62-118).

What changes: the whole forward.  The reference converts the graph to networkx, builds alias tables for the edges and the
nodes, and draws walk_length * walk_num * N edges and (1 + negative) targets each with an interpreted `alias_draw` call.
Here the undirected edge table networkx would hold -- one entry per unordered pair of edge_index, the weight of a repeated
pair being that of its last occurrence -- is built on the graph's device with torch sort / unique, and
cogdl_amd.embedding.line_from_edges trains there.  The return value is the reference's: float64 numpy [N, width] with
L2-normalised rows (order 3: the two halves of dimension // 2 side by side), or with return_dict=True the dict node id -> row.

Opt-in, because the numbers are not the reference's, and neither is the update.  The reference's `_update` receives
fancy-indexed copies (`self.emb_vertex[u]`, `self.emb_vertex[target]`), so its `vec_v += g * vec_u` changes a temporary:
target and context rows are never updated, and since its emb_context IS emb_vertex, its orders 1 and 2 are one computation.
The law served here (csrc/line_law.h) is the original LINE program's update: target rows are updated, the order-2 context
table is a table of its own that starts at zero.  Further differences: the draws are Philox's, by inverse CDF instead of
alias tables; the learning rate changes with every sample, not every 100 batches; a negative equal to either endpoint is
skipped; `batch_size` is ignored (the law has no batches); `self.dimension` is NOT halved by a call with order 3 (the
reference halves it on every call); weighted degrees stay float64 where the reference truncates them into an integer array
(this differs only for non-integer weights).

What does not: edge weights that are not all finite and positive, a graph without edges, an order outside {1, 2, 3} and
dimension < 2 with order 3 reach the reference's own forward (cogdl_amd/_rebind.original).
"""
import sys

import torch

from . import _rebind

_MODULE, _CLASS = "cogdl.models.emb.line", "LINE"


def _weight(graph):
    weight = getattr(graph, "edge_weight", None)
    return None if weight is None or weight.numel() == 0 else weight


def _served(self, graph):
    if graph.edge_index[0].numel() == 0:
        return False
    if self.order not in (1, 2, 3) or (self.order == 3 and int(self.dimension) < 2):
        return False
    weight = _weight(graph)
    return weight is None or bool((torch.isfinite(weight) & (weight > 0)).all())


def forward(self, graph, return_dict=False):
    if not _served(self, graph):
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, graph, return_dict=return_dict)
    from . import embedding
    from .install import _embedding_matrix

    n = graph.num_nodes
    weight = _weight(graph)
    if weight is not None and bool((weight == weight.flatten()[0]).all()):
        weight = None  # equal weights: the unit-weight draw, no table
    edges, weight = embedding.undirected_edges(graph.edge_index[0], graph.edge_index[1], n, weight)
    emb = embedding.line_from_edges(edges, n, weight, dim=self.dimension, samples=self.walk_length * self.walk_num * n,
                                    negative=self.negative, alpha=self.init_alpha, order=self.order)
    return _embedding_matrix(self, graph, return_dict, emb)


def install():
    _rebind.put("line", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    return True
