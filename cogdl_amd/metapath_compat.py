"""The reference's Metapath2vec model on this library's metapath walk and skip-gram operators:
`install(metapath=True)` binds `Metapath2vec.forward` (cogdl/models/emb/metapath2vec.py:66-85).

What changes: the walks.  The reference builds a networkx DiGraph of edge_index and, walk_num x nodes x metapaths x
walk_length times, runs an interpreted step that lists the neighbours of the current node and compares type strings
(metapath2vec.py:87-125).  Here the CSR of the DiGraph is built on the device of edge_index -- parallel edges count once,
as DiGraph collapses them -- and cogdl_amd.embedding.metapath2vec walks (typed row layout, one kernel launch; the OpenMP
host twin for a CPU graph) and trains there.  The return value is the reference's: a float32 numpy array with one row
per node of the DiGraph, that is per node that occurs in an edge, in networkx insertion order (first appearance in row[0],
col[0], row[1], col[1], ..).  A node that no walk visits has no vector in the reference's model: KeyError, as gensim raises.

Opt-in, because the numbers are not the reference's: the draws are Philox's (not `random`'s and gensim's); the start order
differs (per pass and metapath one shuffle of the nodes of the metapath's first type, where the reference shuffles all nodes
once per pass and loops over the metapaths inside); `worker` is ignored.

What is not served reaches the reference's own forward (cogdl_amd/_rebind.original): a schema item that is not an integer
in its plain decimal form (the reference compares strings: "01" never equals "1"), a metapath of fewer than two items or
whose first item differs from its last, a `data.pos` that is not an integer tensor with one non-negative entry per node
(at most 64 types), and a graph without edges.
"""
import sys

import torch

from . import _rebind

_MODULE, _CLASS = "cogdl.models.emb.metapath2vec", "Metapath2vec"
_MAX_TYPES = 64


def digraph_csr(row, col, num_nodes):
    """(row, col) -> (indptr, indices, order): the int64 CSR of the DiGraph (every (row, col) pair once) and the nodes that
    occur in an edge in networkx insertion order; on the tensors' device."""
    row, col = row.long(), col.long()
    keys = torch.unique(row * num_nodes + col)
    indptr = torch.zeros(num_nodes + 1, dtype=torch.long, device=keys.device)
    torch.cumsum(torch.bincount(keys // num_nodes, minlength=num_nodes), 0, out=indptr[1:])
    seen = torch.stack([row, col], 1).flatten()
    nodes, inverse = torch.unique(seen, return_inverse=True)
    first = torch.full((nodes.numel(),), seen.numel(), dtype=torch.long, device=seen.device)
    first.scatter_reduce_(0, inverse, torch.arange(seen.numel(), device=seen.device), "amin")
    return indptr, (keys % num_nodes).contiguous(), nodes[torch.argsort(first)]


def _parse(schema):
    """The schema as integer lists ("No": None), or False where the reference has to take it."""
    if not isinstance(schema, str):
        return False
    if schema == "No":
        return None
    paths = []
    for path in schema.split(","):
        items = path.split("-")
        if len(items) < 2 or items[0] != items[-1] or any(not (item.isdigit() and str(int(item)) == item) for item in items):
            return False
        paths.append([int(item) for item in items])
    return paths


def _served(data, paths):
    row = data.edge_index[0]
    if paths is False or not torch.is_tensor(row) or row.numel() == 0:
        return False
    if paths is None:
        return True
    pos = getattr(data, "pos", None)
    if (not torch.is_tensor(pos) or pos.dim() != 1 or pos.is_floating_point() or pos.is_complex() or pos.dtype == torch.bool
            or pos.numel() == 0 or int(pos.min()) < 0 or int(pos.max()) >= _MAX_TYPES):
        return False
    top = max(int(row.max()), int(data.edge_index[1].max()))
    return top < pos.numel() and int(min(int(row.min()), int(data.edge_index[1].min()))) >= 0


def forward(self, data):
    paths = _parse(self.schema)
    if not _served(data, paths):
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, data)
    from . import embedding

    row, col = data.edge_index
    if paths is None:
        num_nodes = int(max(int(row.max()), int(col.max()))) + 1
        node_type, schema = None, "No"
    else:
        num_nodes = data.pos.numel()
        node_type, schema = data.pos.to(row.device).long(), paths
    indptr, indices, order = digraph_csr(row, col, num_nodes)
    emb, walks = embedding.metapath2vec((indptr, indices), node_type, schema, dim=self.dimension, walk_length=self.walk_length,
                                        walk_num=self.walk_num, window=self.window_size, epochs=self.iteration, nodes=order,
                                        return_walks=True)
    visited = torch.zeros(num_nodes, dtype=torch.bool, device=walks.device)
    visited[walks[walks >= 0]] = True
    missing = order[~visited[order]]
    if missing.numel():
        raise KeyError("Key '%d' not present" % int(missing[0]))  # (no walk visits it: gensim's lookup fails the same way)
    return emb[order].detach().cpu().numpy()


def install():
    _rebind.put("metapath", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    return True
