"""Writes tests/golden/metapath_corridor.npz: the corridor graph of tests/_metapath_cases.py and the walks that the reference's
own Metapath2vec._walk (cogdl/models/emb/metapath2vec.py:87-106) takes on it.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs.
The reference module imports gensim; where that is absent cogdl_amd.gensim_compat stands in for the import (nothing of it
runs: only _walk is called).  The model is NOT rebound.

On the corridor graph every node has at most one neighbour of each type, so `random.choice(candidates)` has one candidate
and the reference's walk is deterministic.  For every schema of CORRIDOR_SCHEMAS one walk of LENGTH positions is started at
every node of the schema's first type, in node order.  Recorded: row, col (the edges as given to networkx), node_type,
and per schema k: schema_k (the string as bytes), start_k, walks_k (int64 [starts, LENGTH], -1 after an early end).  Only
arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "")
LENGTH = 14


def main():
    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "cogdl")):
        raise SystemExit("set COGDL_REFERENCE to a checkout of the reference package")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    try:
        import gensim  # noqa: F401
    except ImportError:
        from cogdl_amd import gensim_compat

        gensim_compat.register()
    import networkx as nx
    from cogdl.models.emb.metapath2vec import Metapath2vec

    import _metapath_cases as cases

    indptr, indices, node_type, n = cases.corridor()
    row = np.repeat(np.arange(n), np.diff(indptr.numpy()))
    col, types = indices.numpy(), node_type.numpy()
    model = Metapath2vec(8, LENGTH, 1, 3, 1, 1, ",".join(cases.CORRIDOR_SCHEMAS))
    model.G = nx.DiGraph()
    model.G.add_edges_from(list(zip(row, col)))
    model.node_type = [str(a) for a in types.tolist()]
    out = {"row": row, "col": col, "node_type": types, "length": np.asarray(LENGTH)}
    for k, schema in enumerate(cases.CORRIDOR_SCHEMAS):
        first = schema.split("-")[0]
        start = [v for v in range(n) if model.node_type[v] == first and v in model.G]
        walks = np.full((len(start), LENGTH), -1, dtype=np.int64)
        for r, v in enumerate(start):
            walk = model._walk(v, LENGTH, schema)
            walks[r, :len(walk)] = walk
        out.update({"schema_%d" % k: np.frombuffer(schema.encode(), dtype=np.uint8), "start_%d" % k: np.asarray(start, dtype=np.int64),
                    "walks_%d" % k: walks})
        ends = int((walks[:, -1] < 0).sum())
        print("%-12s %3d walks, %d end early" % (schema, len(start), ends))
    path = os.path.join(HERE, "metapath_corridor.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
