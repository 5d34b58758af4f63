"""Writes tests/golden/walk_pins.npz: what the HOST twin of the three walk operators returns for fixed seeds, 64 walkers x 20
positions per case, on the small graphs of tests/_walk_cases.py and tests/_metapath_cases.py (a path with a sink, a star,
a random graph with degree-0 nodes, parallel edges, the node2vec graph; three typed graphs with dead ends).

The record pins the arrays themselves: the other tests compare the GPU with the host and laws by chi-square, and would pass
if both sides changed together.  It was written by this script at the commit BEFORE the walks were split into rules and one
scaffold; tests/test_walk_pins.py asserts that `compute()` still returns exactly these arrays.  Rerun it only when a change
of the arrays is intended.

    random_walk     restart 0, 0.3, 1
    node2vec_walk   (p, q) = (0.25, 4), (4, 0.25), (1, 1); and NODE2VEC_TRIALS = 1 with its fallback counts
    metapath_walk   schema "0-1-0,0-2-0,1-0-2-0-1" with walker_path, and its lengths
Only arrays are stored (the inputs `start` / `walker_path` of a case next to its outputs)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)) if p not in sys.path]

WALKERS, LENGTH = 64, 20
RESTARTS = (0.0, 0.3, 1.0)
PQ = ((0.25, 4.0), (4.0, 0.25), (1.0, 1.0))
SCHEMA = "0-1-0,0-2-0,1-0-2-0-1"
TYPED = ("random", "multi", "corridor")  # the cases of _metapath_cases.py that have three node types


def compute():
    """-> {name: numpy array}, from the host twin."""
    import torch

    import _metapath_cases as cases
    import _walk_cases as plain
    from cogdl_amd.operators import metapath_walk, node2vec_walk, random_walk
    from cogdl_amd.operators import walk as walk_mod

    out = {}
    graphs = dict(plain.GRAPHS, n2v=plain.n2v_graph)
    for g, name in enumerate(sorted(graphs)):
        indptr, indices, n = graphs[name]()
        start = (torch.arange(WALKERS) * 7) % n  # (random: 301 .. 399 have no out-edges; path: the sink 5)
        out["%s.start" % name] = start.numpy()
        for restart in RESTARTS:
            walks = random_walk(indptr, indices, start, LENGTH, restart_p=restart, seed=100 + g)
            out["%s.random_walk.%g" % (name, restart)] = walks.numpy()
        for p, q in PQ:
            walks = node2vec_walk(indptr, indices, start, LENGTH, p=p, q=q, seed=200 + g)
            out["%s.node2vec.%g.%g" % (name, p, q)] = walks.numpy()
        saved = walk_mod.NODE2VEC_TRIALS
        walk_mod.NODE2VEC_TRIALS = 1
        try:
            walks, fallback = node2vec_walk(indptr, indices, start, LENGTH, p=0.25, q=4.0, seed=300 + g, return_fallback=True)
        finally:
            walk_mod.NODE2VEC_TRIALS = saved
        out["%s.node2vec.one_trial" % name] = walks.numpy()
        out["%s.node2vec.one_trial.fallback" % name] = fallback.numpy()
    paths = walk_mod.parse_schema(SCHEMA)
    for g, name in enumerate(TYPED):
        indptr, indices, node_type, n = cases.CASES[name]()
        start, which = cases.starts_for(node_type, paths, repeat=WALKERS)
        pick = np.random.default_rng(g).permutation(start.numel())[:WALKERS]  # a mixed walker_path
        start, which = start[pick], which[pick]
        walks, lengths = metapath_walk(indptr, indices, node_type, start, SCHEMA, LENGTH, walker_path=which, seed=400 + g,
                                       return_lengths=True)
        out.update({"%s.metapath.start" % name: start.numpy(), "%s.metapath.walker_path" % name: which.numpy(),
                    "%s.metapath" % name: walks.numpy(), "%s.metapath.lengths" % name: lengths.numpy()})
    return out


def main():
    out = compute()
    path = os.path.join(HERE, "walk_pins.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
