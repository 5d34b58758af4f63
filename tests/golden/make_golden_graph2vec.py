"""Writes tests/golden/graph2vec_wl.npz: a few small graphs and the WL words the reference's own Graph2Vec.feature_extractor
(cogdl/models/emb/graph2vec.py:50-78) gives them, as integers.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs.
The reference module imports gensim.models.doc2vec, which this image lacks: cogdl_amd.gensim_compat is registered for the
import (TaggedDocument is a namedtuple there as in gensim); feature_extractor and wl_iterations run as they are.

Graphs: with and without x, duplicate and one-directional edges, a self-loop, an id that occurs in no edge, a row of x that
occurs in no edge, two graphs of one structure under different node orders (shared words), two rounds.  The word strings
(degree strings, numpy's printed rows, md5 digests) are NOT stored: per word its id by first occurrence over all documents,
its round and its node, in the reference's order (round 0: every row of x, or the nodes in networkx insertion order; then
per round the nodes in insertion order).  Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "")
ROUNDS = 2

GRAPHS = [
    # (edges as (row, col) pairs, x or None)
    ([(0, 1), (1, 0), (1, 2), (2, 4), (4, 4), (4, 5), (1, 2), (5, 2)], None),            # node 3 occurs in no edge; a self-loop
    ([(5, 4), (4, 2), (2, 0), (0, 0), (0, 1), (1, 2), (4, 5)], None),                     # the same structure, other ids
    ([(0, 1), (1, 2), (2, 0), (2, 3)], None),                                             # a triangle with a pendant
    ([(0, 1), (1, 2), (2, 3), (3, 3), (4, 0)], [[0.5, 1.0], [0.5, 1.0], [1.25, -2.0], [0.5, 1.0], [1.25, -2.0], [0.5, 1.0]]),
    ([(0, 1), (0, 2), (0, 3), (3, 4)], [[1.25, -2.0], [0.5, 1.0], [0.5, 1.0], [0.5, 1.0], [1.25, -2.0]]),
    ([(0, 1), (0, 2), (0, 3), (0, 4)], None),                                             # a star
]


def main():
    import networkx as nx
    import torch

    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "cogdl")):
        raise SystemExit("set COGDL_REFERENCE to a checkout of the reference package")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [ROOT, os.path.join(HERE, "_stubs"), scratch]
    try:
        import gensim  # noqa: F401
    except ImportError:
        from cogdl_amd import gensim_compat

        gensim_compat.register()
    from cogdl.data import Graph
    from cogdl.models.emb.graph2vec import Graph2Vec

    ids, word, rnd, node, doc_ptr = {}, [], [], [], [0]
    edges, edge_ptr, xs, x_ptr, has_x = [], [0], [], [0], []
    for k, (pairs, x) in enumerate(GRAPHS):
        ei = torch.tensor(pairs, dtype=torch.long).t().contiguous()
        xt = None if x is None else torch.tensor(x, dtype=torch.float32)
        data = Graph(edge_index=ei, x=xt)
        doc = Graph2Vec.feature_extractor(data, ROUNDS, str(k))
        assert doc.tags == ["g_%d" % k]
        order = list(nx.from_edgelist(np.array(ei.t(), dtype=int)).nodes)  # networkx insertion order, as the reference walks it
        where = [(0, v) for v in (range(len(x)) if x is not None else order)]
        where += [(r, v) for r in range(1, ROUNDS + 1) for v in order]
        assert len(where) == len(doc.words), (len(where), len(doc.words))
        for w, (r, v) in zip(doc.words, where):
            word.append(ids.setdefault(w, len(ids)))
            rnd.append(r)
            node.append(int(v))
        doc_ptr.append(len(word))
        edges.append(ei.numpy())
        edge_ptr.append(edge_ptr[-1] + ei.shape[1])
        has_x.append(x is not None)
        if x is not None:
            xs.append(xt.numpy())
        x_ptr.append(x_ptr[-1] + (0 if x is None else len(x)))
    out = dict(word=np.asarray(word, dtype=np.int64), round=np.asarray(rnd, dtype=np.int64), node=np.asarray(node, dtype=np.int64),
               doc_ptr=np.asarray(doc_ptr, dtype=np.int64), edges=np.concatenate(edges, 1).astype(np.int64),
               edge_ptr=np.asarray(edge_ptr, dtype=np.int64), x=np.concatenate(xs, 0).astype(np.float32),
               x_ptr=np.asarray(x_ptr, dtype=np.int64), has_x=np.asarray(has_x), rounds=np.asarray(ROUNDS))
    path = os.path.join(HERE, "graph2vec_wl.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(word), "words,", len(ids), "distinct")
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
