"""The small CSR graphs of the walk tests (tests/test_walk_host.py, tests/test_walk_gpu.py) and of the recorded arrays
(tests/golden/make_walk_pins.py).  Every builder returns (indptr, indices, number of nodes)."""
import numpy as np
import torch


def csr_of(row, col, n):
    """Stable CSR (rows keep their COO order, duplicates kept) as int64 tensors."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    order = np.argsort(row, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=indptr[1:])
    return torch.from_numpy(indptr), torch.from_numpy(col[order].copy())


def path_with_sink():
    n = 6
    return csr_of(np.arange(n - 1), np.arange(1, n), n) + (n,)


def star():
    leaves = np.arange(1, 5001)
    zeros = np.zeros(5000, dtype=np.int64)
    return csr_of(np.concatenate([zeros, leaves]), np.concatenate([leaves, zeros]), 5001) + (5001,)


def random_with_isolated():
    rng = np.random.default_rng(5)
    n = 400
    row, col = rng.integers(0, 300, 3000), rng.integers(0, n, 3000)  # nodes 300.. have no out-edges
    return csr_of(row, col, n) + (n,)


def duplicates():
    row = [0, 0, 0, 1, 1, 2, 2, 2, 2, 3]
    col = [1, 1, 2, 0, 0, 3, 3, 3, 0, 2]
    return csr_of(row, col, 4) + (4,)


GRAPHS = {"path": path_with_sink, "star": star, "random": random_with_isolated, "dup": duplicates}


def n2v_graph():
    """Symmetric.  At (t, v) = (0, 1) the neighbours of v are 0 (= t), 2 (adjacent to t), 3 and 4 (not adjacent to t)."""
    pairs = [(0, 1), (1, 2), (0, 2), (1, 3), (1, 4), (3, 4)]
    row = [a for a, b in pairs] + [b for a, b in pairs]
    col = [b for a, b in pairs] + [a for a, b in pairs]
    return csr_of(row, col, 5) + (5,)
