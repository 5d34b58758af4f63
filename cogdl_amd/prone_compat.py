"""The reference's ProNE model and its spectral filters on this library's operators: `install(prone=True)` binds
`ProNE.forward` (cogdl/models/emb/prone.py:46-64) and `propagate` (cogdl/utils/prone_utils.py:195-229, with its by-name
copy in cogdl.models.emb.pronepp, so ProNE++'s search and the `--enhance prone` / `prone++` post-processing inherit it).

What changes: ProNE.forward converts the graph to networkx and runs scipy / sklearn in float64 on the host; here the simple
symmetric structure the reference's `nx.Graph` holds is built on the graph's device and cogdl_amd.embedding.prone factorises,
propagates and embeds there.  `propagate` keeps its signature (a scipy matrix, a numpy embedding, the filter's name and the
optional parameter dict) and runs cogdl_amd.operators.spectral.spectral_filter: on the GPU when one is visible, on the host
twin otherwise; the result comes back as float64 numpy.

Opt-in, because the numbers are not the reference's: float32 instead of float64, the operator M applied as a fused step
instead of one assembled sparse matrix, the randomized SVD of cogdl_amd.operators.netsmf (torch's generator, CholeskyQR2)
instead of sklearn's, a node without edges gets a zero row of the factorisation.

What does not: a graph whose edge weights are not all equal, a graph with self loops, a graph without edges and step == 1
reach the reference's own forward; `propagate` with the "sc" filter, any other name, a parameter dict for "prone", a matrix
that is not square with unit entries and an empty diagonal, or an embedding that is not a 2-D array reaches the reference's
function (cogdl_amd/_rebind.original).
"""
import sys

import torch

from . import _rebind

_MODULE, _CLASS = "cogdl.models.emb.prone", "ProNE"
_UTILS, _HOLDER = "cogdl.utils.prone_utils", "cogdl.models.emb.pronepp"
_SPACE_KEYS = {"heat": ("t",), "ppr": ("alpha",), "gaussian": ("mu", "theta")}


def _served(model, graph):
    row, col = graph.edge_index
    if row.numel() == 0 or int(model.step) == 1 or bool((row == col).any()):
        return False
    weight = getattr(graph, "edge_weight", None)
    return weight is None or weight.numel() == 0 or bool((weight == weight.flatten()[0]).all())


def forward(self, graph, return_dict=False):
    if not _served(self, graph):
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "forward")(self, graph, return_dict=return_dict)
    from . import embedding
    from .install import _embedding_matrix
    from .netsmf_compat import symmetric_csr

    indptr, indices = symmetric_csr(graph.edge_index, graph.num_nodes)
    emb = embedding.prone((indptr, indices), dim=self.dimension, step=self.step, mu=self.mu, theta=self.theta)
    return _embedding_matrix(self, graph, return_dict, emb)  # (the reference's nx.Graph holds the nodes 0 .. N - 1 in order)


def _filter_inputs(mx, emb, stype, space):
    """-> (rowptr, colind, emb float32, params) as numpy / dict when spectral_filter serves the call, else None."""
    import numpy as np
    import scipy.sparse as sp

    if stype not in _SPACE_KEYS and stype != "prone":
        return None
    if space is not None and (stype == "prone" or any(k not in space for k in _SPACE_KEYS[stype])):
        return None
    if not sp.issparse(mx) or mx.shape[0] != mx.shape[1] or not isinstance(emb, np.ndarray) or emb.ndim != 2:
        return None
    if emb.shape[0] != mx.shape[0] or emb.shape[1] == 0 or mx.shape[0] == 0:
        return None
    csr = sp.csr_matrix(mx, copy=True)
    csr.sum_duplicates()
    csr.sort_indices()
    if csr.nnz >= 2 ** 31 - 2 ** 20 or not (csr.data == 1).all() or (csr.diagonal() != 0).any():
        return None
    params = {} if space is None else dict((k, float(space[k])) for k in _SPACE_KEYS[stype])
    return csr.indptr.astype(np.int32), csr.indices.astype(np.int32), np.ascontiguousarray(emb, dtype=np.float32), params


def propagate(mx, emb, stype, space=None):
    served = _filter_inputs(mx, emb, stype, space)
    if served is None:
        return _rebind.original(sys.modules[_UTILS], "propagate")(mx, emb, stype, space)
    import numpy as np

    from .operators.spectral import spectral_filter

    rowptr, colind, emb32, params = served
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    out = spectral_filter(stype, torch.from_numpy(rowptr).to(dev), torch.from_numpy(colind).to(dev),
                          torch.from_numpy(emb32).to(dev), **params)
    return out.cpu().numpy().astype(np.float64)


def install():
    _rebind.put("prone", getattr(sys.modules[_MODULE], _CLASS), "forward", forward)
    _rebind.put("prone", sys.modules[_UTILS], "propagate", propagate)
    holder = sys.modules.get(_HOLDER)
    if holder is not None and getattr(holder, "propagate", None) is not None:
        _rebind.put("prone", holder, "propagate", propagate)
    return True
