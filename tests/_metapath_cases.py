"""Small typed graphs and a brute-force checker for the metapath walk (tests/test_metapath_host.py, test_metapath_gpu.py,
tests/golden/make_golden_metapath.py).  A case is (indptr, indices, node_type, n): int64 CSR tensors (rows keep their COO
order, duplicates kept), int64 node types."""
import numpy as np
import torch


def csr_of(row, col, n):
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    order = np.argsort(row, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=n), out=indptr[1:])
    return torch.from_numpy(indptr), torch.from_numpy(col[order].copy())


def _case(row, col, types):
    n = len(types)
    return csr_of(row, col, n) + (torch.as_tensor(np.asarray(types, dtype=np.int64)), n)


def typed_path():
    """0 -> 1 -> .. -> 6 and back, types 0 1 0 1 ..; node 7 (type 1) is a sink that 6 points to; 8 is isolated."""
    row = list(range(6)) + list(range(1, 7)) + [6]
    col = list(range(1, 7)) + list(range(6)) + [7]
    return _case(row, col, [0, 1, 0, 1, 0, 1, 0, 1, 0])


def star():
    """Bipartite: hub 0 (type 0), 300 leaves (type 1), edges both ways."""
    leaves = np.arange(1, 301)
    zeros = np.zeros(300, dtype=np.int64)
    return _case(np.concatenate([zeros, leaves]), np.concatenate([leaves, zeros]), [0] + [1] * 300)


def random_typed():
    """200 nodes, 3 types.  Nodes 170.. have no out-edges (190.. no edges at all); nodes below 30 have no neighbour of type 2."""
    rng = np.random.default_rng(17)
    n = 200
    types = rng.integers(0, 3, n)
    row, col = rng.integers(0, 170, 1400), rng.integers(0, 190, 1400)
    keep = ~((row < 30) & (types[col] == 2))
    return _case(row[keep], col[keep], types)


def multigraph():
    """Parallel edges: node 0 (type 0) -> 1, 1, 1, 2 (type 1) and 3, 3 (type 2); everything points back to 0 twice."""
    row = [0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 3]
    col = [1, 3, 1, 2, 3, 1, 0, 0, 0, 0, 0, 0, 4]
    return _case(row, col, [0, 1, 1, 2, 2])


def corridor():
    """40 nodes, 3 types, directed; every node has AT MOST one neighbour of each type (about one in five is missing), so a
    metapath walk is deterministic: the reference's interpreted walk, recorded in tests/golden/metapath_corridor.npz, is
    the expected array itself."""
    rng = np.random.default_rng(2024)
    n = 40
    types = np.arange(n) % 3
    rng.shuffle(types)
    row, col = [], []
    for v in range(n):
        for t in range(3):
            if rng.random() < 0.8:
                row.append(v)
                col.append(int(rng.choice(np.flatnonzero(types == t))))
    order = rng.permutation(len(row))  # rows are not grouped by type
    return _case(np.asarray(row)[order], np.asarray(col)[order], types)


CASES = {"path": typed_path, "star": star, "random": random_typed, "multi": multigraph, "corridor": corridor}
CORRIDOR_SCHEMAS = ("0-1-0", "0-0", "1-0-2-0-1", "2-1-0-2", "0-1-2-1-0")


def starts_for(node_type, paths, repeat=1):
    """Every node of a metapath's first type, for every metapath, `repeat` times -> (start, walker_path) int64 / int32."""
    ty = np.asarray(node_type)
    start, which = [], []
    for _ in range(repeat):
        for p, items in enumerate(paths):
            nodes = np.flatnonzero(ty == items[0])
            start.append(nodes)
            which.append(np.full(nodes.size, p))
    return (torch.from_numpy(np.concatenate(start).astype(np.int64)),
            torch.from_numpy(np.concatenate(which).astype(np.int32)))


def check_walks(indptr, indices, node_type, start, paths, walker_path, walks, lengths=None):
    """Brute force, from the plain CSR: position 0 is the start; every consecutive pair of nodes is an edge; every position
    holds the wanted type items[i % (len(items) - 1)]; after a -1 only -1; the first -1 stands exactly where the previous node
    has no neighbour of the wanted type; lengths counts the positions that hold a node."""
    ip, ix, ty = np.asarray(indptr), np.asarray(indices), np.asarray(node_type).astype(np.int64)
    n = ip.size - 1
    t_count = int(ty.max()) + 1 if n else 1
    row = np.repeat(np.arange(n), np.diff(ip))
    edges = np.unique(row * n + ix)
    typed_degree = np.bincount(row * t_count + ty[ix], minlength=n * t_count)
    w = np.asarray(walks)
    n_walkers, length = w.shape
    start, walker_path = np.asarray(start), np.asarray(walker_path).astype(np.int64)
    assert start.shape == (n_walkers,) and walker_path.shape == (n_walkers,)
    assert np.array_equal(w[:, 0], start), "position 0 is not the start node"
    if n_walkers:
        assert w.min() >= -1 and w.max() < n
        first = np.asarray([items[0] for items in paths])[walker_path]
        assert np.array_equal(ty[start], first), "a start node of the wrong type"
    alive = np.ones(n_walkers, dtype=bool)
    held = np.ones(n_walkers, dtype=np.int64)
    for i in range(1, length):
        want = np.asarray([items[i % (len(items) - 1)] for items in paths], dtype=np.int64)[walker_path]
        x, prev = w[:, i], w[:, i - 1]
        assert (x[~alive] == -1).all(), "a node after the walk had ended (position %d)" % i
        idx = np.flatnonzero(alive)
        xa, pv, wa = x[idx], prev[idx], want[idx]
        has = typed_degree[pv * t_count + wa] > 0
        ended = xa == -1
        assert np.array_equal(ended, ~has), "position %d: a walk ended where a neighbour of the wanted type exists, or went on where none does" % i
        go = ~ended
        assert np.isin(pv[go] * n + xa[go], edges).all(), "position %d: a transition that is not an edge" % i
        assert np.array_equal(ty[xa[go]], wa[go]), "position %d: a node of the wrong type" % i
        alive[idx[ended]] = False
        held += alive
    if lengths is not None:
        assert np.array_equal(np.asarray(lengths).astype(np.int64), held), "lengths disagrees with the walks"
    return held
