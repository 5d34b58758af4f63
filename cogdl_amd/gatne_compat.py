"""The reference's GATNE model on this library's walk, multiplex-embedding and sampled-score operators:
`install(gatne=True)` binds `GATNE.forward` (cogdl/models/emb/gatne.py:111-194).

What changes: the whole forward.  The reference walks every layer in networkx one interpreted step at a time, builds every
training pair and every batch of 256 pairs (with its [B, T, S] neighbour list) from Python lists, runs GATNEModel.forward -- a
[B, T, S, T, U] gather of which the diagonal is kept, about fifteen small kernels, float atomics backward -- and reads the final
embeddings out one node at a time.  Here cogdl_amd.embedding.gatne does all of it on the device: the layers' undirected simple
graphs as CSR, the library's random_walk, pairs by tensor slicing, one [N, T, S] neighbour table, and per step one
multiplex_embed (cogdl_amd/operators/multiplex.py) and one sampled_scores call under torch.optim.Adam(lr=1e-4), as the reference
sets it.  The return value is the reference's: {edge_type_key: {node id (int): float32 numpy [dimension]}}, keys in
network_data's order, one entry per walked node.

Opt-in, because the numbers are not the reference's: the draws are Philox's and torch's (not `random`'s and numpy's); ties in the
vocabulary order (equal counts) go in ascending node id where the reference keeps first appearance; a trailing batch of one pair
and a network of one edge type train here, where the reference's module raises (a squeeze()); `worker` is ignored.  The skip
window is the reference's: its forward never hands `window_size` to generate_pairs, so the window is always 5.

What is not served reaches the reference's own forward (cogdl_amd/_rebind.original): a `schema` other than None (the reference
builds its walker without node types and fails there, as before), an empty network_data, a layer without edges, and node ids
that are not non-negative integers.
"""
import sys

from . import _rebind

_MODULE, _CLASS = "cogdl.models.emb.gatne", "GATNE"
_WINDOW = 5  # generate_pairs' default: GATNE.forward does not pass self.window_size


def _edge_lists(network_data):
    """-> list of int64 [E, 2] tensors, or None where the reference has to take the call."""
    import numpy as np
    import torch

    if not isinstance(network_data, dict) or not network_data:
        return None
    layers = []
    for edges in network_data.values():
        try:
            arr = np.asarray([(e[0], e[1]) for e in edges])
        except (TypeError, IndexError, ValueError):
            return None
        if arr.ndim != 2 or arr.shape[0] == 0 or arr.dtype.kind not in "iu" or int(arr.min()) < 0:
            return None
        layers.append(torch.from_numpy(arr.astype(np.int64)))
    return layers


def forward(self, network_data):
    layers = None if self.schema is not None else _edge_lists(network_data)
    if layers is None:
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, network_data)
    from . import embedding

    emb, nodes = embedding.gatne(layers, dim=self.embedding_size, walk_length=self.walk_length, walk_num=self.walk_num, window=_WINDOW,
                                 epochs=self.epochs, batch_size=self.batch_size, edge_dim=self.embedding_u_size, att_dim=self.dim_att,
                                 negative=self.num_sampled, neighbor_samples=self.neighbor_samples, lr=1e-4)
    emb, nodes = emb.detach().cpu().numpy(), nodes.cpu().tolist()
    return {key: {node: emb[t, k] for k, node in enumerate(nodes)} for t, key in enumerate(network_data)}


def install():
    _rebind.put("gatne", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    return True
