"""Writes tests/golden/line_reference.json: the neighbour purity of the reference's own LINE (cogdl/models/emb/line.py) on the
quality instance of the LINE tests -- the planted-partition graph of tests/test_sgns_host.py (64 communities of 32 nodes) at
dimension 32 (orders 1 and 2) and 64 (order 3), negative 5, alpha 0.025, walk_length 80 x walk_num 20 = 1600 samples per node,
batch_size 1000.

Run in the build container only, where the reference package is checked out; it is driven unchanged and NOT rebound, through
tools/refpkg.setup(install=False), with `np.int = int` (alias_setup still says np.int) and numpy seeded with 0 before each
forward.  The interpreted alias_draw loop makes this take about three minutes on a CPU.  Only the recorded purities and the
parameters that produced them are stored."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARAMS = dict(communities=64, size=32, p_in=0.3, graph_seed=0, dim=32, dim_order3=64, walk_length=80, walk_num=20, negative=5,
              batch_size=1000, alpha=0.025, numpy_seed=0)


def main():
    import torch

    sys.path[:0] = [ROOT, os.path.dirname(HERE)]
    from tools import refpkg

    if not refpkg.available():
        raise SystemExit("the reference package is not available (oracle/_ref/pkg or $COGDL_REFERENCE)")
    refpkg.setup(install=False)
    if not hasattr(np, "int"):
        np.int = int
    from cogdl.data import Graph
    from cogdl.models.emb.line import LINE

    from test_sgns_host import neighbour_purity, planted_partition

    indptr, indices, n, community = planted_partition(PARAMS["communities"], PARAMS["size"], PARAMS["p_in"], PARAMS["graph_seed"])
    row = torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])
    graph = Graph(edge_index=torch.stack([row, indices]), num_nodes=n)
    purity = {}
    for order in (1, 2, 3):
        dim = PARAMS["dim_order3"] if order == 3 else PARAMS["dim"]
        model = LINE(dim, PARAMS["walk_length"], PARAMS["walk_num"], PARAMS["negative"], PARAMS["batch_size"], PARAMS["alpha"], order)
        np.random.seed(PARAMS["numpy_seed"])
        emb = model.forward(graph)
        assert emb.shape == (n, dim), emb.shape
        purity[str(order)] = round(neighbour_purity(torch.from_numpy(emb), community), 6)
        print("reference LINE order %d: neighbour purity %.4f" % (order, purity[str(order)]), flush=True)
    with open(os.path.join(HERE, "line_reference.json"), "w") as f:
        json.dump({"params": PARAMS, "purity": purity}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote line_reference.json")


if __name__ == "__main__":
    main()
