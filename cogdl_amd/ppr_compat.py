"""`ppr_topk`, `topk_ppr_matrix` and `build_topk_ppr_matrix_from_data` with the call shapes and return types of
cogdl/utils/ppr_utils.py:51-108 on this library's PPR operator (cogdl_amd/operators/ppr.py): `install(ppr=True)` binds them
in place of the reference's functions, whose push loop is numba-jitted (or, without numba, interpreted) Python on the CPU.

Conventions kept from the reference:
  * a (row, col) tuple or a [2, E] tensor becomes a scipy CSR matrix of ones over max id + 1 nodes, duplicates summed -- so
    a push goes to DISTINCT neighbours and the degree counts them; a scipy matrix is taken as it is (its stored structure);
  * the result is a scipy CSR matrix of shape (len(idx), N) with up to topk entries per row;
  * normalization "sym" / "col" scale by adj_matrix.sum(1) as ppr_utils.py:75-89 does (float64 data), "row" leaves the
    float32 scores.
Different from the reference: the values are those of the deterministic synchronous process (operators/ppr.py); both lie
within eps * deg of the exact PPR.  `device=None` runs on the GPU when one is visible, otherwise on the host twin.
"""
import numpy as np
import scipy.sparse as sp
import torch

from .operators import ppr as _ppr


def _device(device):
    if device is None:
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def ppr_topk(adj_matrix, alpha, epsilon, nodes, topk, device=None):
    """-> scipy COO matrix (len(nodes), N): per source the topk largest approximate PPR scores."""
    adj = sp.csr_matrix(adj_matrix)
    adj.sum_duplicates()
    dev = _device(device)
    nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
    indptr = torch.from_numpy(np.asarray(adj.indptr, dtype=np.int64)).to(dev)
    indices = torch.from_numpy(np.asarray(adj.indices, dtype=np.int64)).to(dev)
    nbr, val, count = _ppr.topk_ppr(indptr, indices, torch.from_numpy(nodes).to(dev), float(alpha), float(epsilon), int(topk))
    nbr, val, count = nbr.cpu().numpy(), val.cpu().numpy(), count.cpu().numpy()
    used = np.arange(nbr.shape[1])[None, :] < count[:, None]
    rows = np.repeat(np.arange(len(nodes)), count)
    return sp.coo_matrix((val[used], (rows, nbr[used])), shape=(len(nodes), adj.shape[0]))


def topk_ppr_matrix(adj_matrix, alpha, eps, idx, topk, normalization="row", device=None):
    """Create a sparse matrix where each node has up to the topk PPR neighbors and their weights."""
    if normalization not in ("sym", "col", "row"):
        raise ValueError(f"Unknown PPR normalization: {normalization}")
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    coo = ppr_topk(adj_matrix, alpha, eps, idx, topk, device=device)
    data = coo.data
    if normalization == "sym":  # assumes an undirected (symmetric) adjacency matrix
        deg = np.asarray(adj_matrix.sum(1)).reshape(-1)
        deg_sqrt = np.sqrt(np.maximum(deg, 1e-12))
        data = deg_sqrt[idx[coo.row]] * data * (1.0 / deg_sqrt)[coo.col]
    elif normalization == "col":
        deg = np.asarray(adj_matrix.sum(1)).reshape(-1)
        data = deg[idx[coo.row]] * data * (1.0 / np.maximum(deg, 1e-12))[coo.col]
    return sp.coo_matrix((data, (coo.row, coo.col)), shape=coo.shape).tocsr()


def build_topk_ppr_matrix_from_data(edge_index, *args, **kwargs):
    if isinstance(edge_index, (torch.Tensor, tuple, list)):
        row, col = edge_index
        row, col = torch.as_tensor(row).cpu().numpy(), torch.as_tensor(col).cpu().numpy()
        num_node = int(max(row.max(), col.max())) + 1
        adj_matrix = sp.csr_matrix((np.ones(row.shape[0]), (row, col)), shape=(num_node, num_node))
    else:
        adj_matrix = edge_index
    return topk_ppr_matrix(adj_matrix, *args, **kwargs)
