"""The cases the LINE tests share (test_line_host.py, test_line_gpu.py, test_line_install_cpu.py): four small graphs, a grid
of about twenty (graph, S, D, K, order) cases, and the quality instance.

The grid holds the smallest shapes at which the kernel can go wrong: S = 1 (a group of one sample), 65 (a full group of 64
and a partial one) and 1000; D = 1 (one lane, a butterfly of width 1, and with the scaled init |f| >= 6), 7 (butterfly of 8),
64 (every lane once), 65 (lane 0 owns two elements) and 200 (four elements per lane, no register prefetch of the targets);
K = 1, 5 and 16 (all sixteen negative registers); both orders.  The triangle with a self-loop forces repeated negatives,
negatives equal to an endpoint, and in order 1 a target row that is the input row."""
import functools

import numpy as np
import torch

ALPHA = 0.05  # high enough that the context table leaves zero quickly


def _random_edges(v=500, m=2000, seed=0):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randint(0, v, (m,), generator=g), torch.randint(0, v, (m,), generator=g)
    b = torch.minimum(b, torch.randint(0, v, (m,), generator=g))  # unequal degrees
    return torch.stack([a, b], dim=1)


ZERO_EDGE = 777  # the edge of the weighted graph that has weight 0


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (edges int64 [M, 2], V, edge_weight float64 [M] or None); computed once, never modified."""
    if name == "single":
        return torch.tensor([[0, 1]]), 2, None
    if name == "triangle":
        return torch.tensor([[0, 1], [1, 2], [0, 2], [2, 2]]), 3, None
    if name == "random":
        return _random_edges(), 500, None
    if name == "weighted":
        g = torch.Generator().manual_seed(1)
        w = torch.tensor([0.5, 1.0, 3.0], dtype=torch.float64)[torch.randint(0, 3, (2000,), generator=g)]
        w[ZERO_EDGE] = 0.0
        return _random_edges(), 500, w
    raise KeyError(name)


# (graph, S, D, K, order)
GRID = [
    ("single", 1, 1, 1, 1), ("single", 65, 7, 5, 2),
    ("triangle", 65, 1, 1, 1), ("triangle", 1000, 7, 16, 1), ("triangle", 1000, 64, 5, 2), ("triangle", 65, 65, 16, 2),
    ("triangle", 1000, 200, 5, 1),
    ("random", 1, 64, 5, 1), ("random", 65, 64, 5, 2), ("random", 1000, 64, 16, 1), ("random", 1000, 65, 5, 2),
    ("random", 1000, 200, 1, 2), ("random", 65, 200, 16, 1), ("random", 1000, 7, 5, 1), ("random", 1000, 1, 16, 2),
    ("weighted", 1000, 64, 5, 1), ("weighted", 1000, 65, 16, 2), ("weighted", 65, 7, 1, 2), ("weighted", 1000, 200, 5, 1),
    ("weighted", 1, 1, 5, 2), ("weighted", 1000, 1, 1, 1),
]


def grid_id(case):
    return "%s-S%d-D%d-K%d-order%d" % case


def grid_init(case, device="cpu"):
    """The starting tables of a grid case: the law's init, for order 2 with a context table that is not zero (so that the
    first dot products are not all 0), and at D = 1 scaled by 8 so that |f| reaches 6."""
    from cogdl_amd.operators import sgns as sgns_mod

    name, s, d, k, order = case
    _, v, _ = graph(name)
    emb, _ = sgns_mod.init_tables(v, d, 11, "cpu")
    ctx, _ = sgns_mod.init_tables(v, d, 12, "cpu")
    scale = 8.0 * d if d == 1 else 1.0
    emb, ctx = (emb * scale).to(device), (ctx * scale).to(device)
    return emb if order == 1 else (emb, ctx)


def grid_run(case, device="cpu", **kw):
    """line_train on a grid case with the grid's init, serial unless told otherwise."""
    from cogdl_amd.operators import line_train

    name, s, d, k, order = case
    edges, v, w = graph(name)
    kw.setdefault("workers", 1)
    kw.setdefault("seed", 5)
    kw.setdefault("init", grid_init(case, device))
    return line_train(edges.to(device), v, d, order, s, negative=k, alpha=ALPHA, edge_weight=w, **kw)


# ------------------------------------------------------------------------------------------------------------- quality
QUALITY = dict(dim=32, negative=5, alpha=0.025)
SAMPLES_PER_NODE = 1600  # the reference's default: walk_length 80 * walk_num 20


@functools.lru_cache(maxsize=None)
def quality_edges():
    """The planted-partition graph of test_sgns_host as an undirected edge table -> (edges, N, community)."""
    from test_sgns_host import planted_partition

    from cogdl_amd.embedding import undirected_edges

    indptr, indices, n, community = planted_partition()
    row = torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])
    edges, _ = undirected_edges(row, indices, n)
    return edges, n, community


@functools.lru_cache(maxsize=None)
def twin_purity(order):
    """Neighbour purity of the serial host twin on the quality instance (once per test run); order 3 at width 64."""
    from test_sgns_host import neighbour_purity

    from cogdl_amd.embedding import line_from_edges

    edges, n, community = quality_edges()
    emb = line_from_edges(edges, n, None, dim=64 if order == 3 else QUALITY["dim"], samples=SAMPLES_PER_NODE * n,
                          negative=QUALITY["negative"], alpha=QUALITY["alpha"], order=order, seed=2, workers=1)
    return neighbour_purity(emb, community)


def reference_purity():
    """{order: purity} of the reference's own LINE on the quality instance (tests/golden/line_reference.json)."""
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "line_reference.json")) as f:
        rec = json.load(f)
    return {int(k): float(v) for k, v in rec["purity"].items()}
