"""Writes tests/golden/netsmf.npz: what the reference's own NetSMF (cogdl/models/emb/netsmf.py) computes on two small graphs.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs and
`np.int = int` (alias_setup still says np.int), and NOT rebound.  NetSMF.forward runs as it stands, in ONE process: the
module's `Pool` is replaced by a stand-in whose apply_async calls the function at once (worker = 1, so _random_walk_matrix(0)
seeds numpy with 0 and takes every sample), and _get_embedding_rand is wrapped to record the matrix it is handed.

  1. The 12-ring with seven chords of tests/_netsmf_cases.py (the 12-node component of G15), num_round = 2000, window_size = 3,
     negative = 1: `matrix` (what _random_walk_matrix returned, dense float64 [12, 12]) and `M` (what lines 90-106 made of it,
     dense float64 [12, 12]).
  2. A stochastic block model of 4 blocks of 32 nodes (p_in 0.4, p_out 0.02, numpy default_rng(7)): `sbm_edges` (the undirected
     edge list, int16 [E, 2]) and `sbm_purity`, the purity of the reference's embedding (dimension 8, window_size 5,
     num_round 100): the fraction of nodes whose nearest neighbour by cosine lies in their own block.  numpy is seeded with 0
     before the forward (sklearn's randomized_svd draws from numpy's global state).  The script asserts purity >= 0.9.
Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "")
WINDOW, NUM_ROUND, NEGATIVE = 3, 2000, 1


class SerialPool:
    """multiprocessing.Pool's three methods NetSMF.forward uses, in the calling process."""

    class Result:
        def __init__(self, value):
            self.value = value

        def get(self):
            return self.value

    results = []

    def __init__(self, processes=None):
        pass

    def apply_async(self, func, args=()):
        res = SerialPool.Result(func(*args))
        SerialPool.results.append(res.value)
        return res

    def close(self):
        pass

    def join(self):
        pass


def sbm_edges():
    rng = np.random.default_rng(7)
    block = np.arange(128) // 32
    iu, ju = np.triu_indices(128, 1)
    prob = np.where(block[iu] == block[ju], 0.4, 0.02)
    keep = rng.random(iu.size) < prob
    return np.stack([iu[keep], ju[keep]], 1).astype(np.int16)


def main():
    import torch

    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "cogdl")):
        raise SystemExit("set COGDL_REFERENCE to a checkout of the reference package")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    if not hasattr(np, "int"):
        np.int = int
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    from cogdl.data import Graph
    from cogdl.models.emb import netsmf as ref

    import _netsmf_cases as cases

    ref.Pool = SerialPool
    handed = []
    inner = ref.NetSMF._get_embedding_rand

    def recording(self, matrix):
        handed.append(matrix.copy())
        return inner(self, matrix)

    ref.NetSMF._get_embedding_rand = recording

    def graph_of(pairs, n):
        pairs = np.asarray(pairs, dtype=np.int64)
        ei = torch.from_numpy(np.concatenate([pairs, pairs[:, ::-1]]).T.copy())
        return Graph(edge_index=ei, num_nodes=n)

    out = {"window": np.int64(WINDOW), "num_round": np.int64(NUM_ROUND), "negative": np.int64(NEGATIVE)}
    model = ref.NetSMF(4, WINDOW, NEGATIVE, NUM_ROUND, 1)
    model.forward(graph_of(cases.RING_CHORDS, 12))
    assert len(SerialPool.results) == 1 and len(handed) == 1
    out["matrix"] = np.asarray(SerialPool.results[0].todense(), dtype=np.float64)
    out["M"] = np.asarray(handed[0].todense(), dtype=np.float64)
    assert out["matrix"].shape == (12, 12) and np.isfinite(out["M"]).all()

    edges = sbm_edges()
    block = np.arange(128) // 32
    np.random.seed(0)
    emb = ref.NetSMF(8, 5, 1, 100, 1).forward(graph_of(edges, 128))
    p = cases.purity(emb, block)
    print("reference purity on the SBM: %.4f (%d edges)" % (p, len(edges)))
    assert p >= 0.9
    out["sbm_edges"] = edges
    out["sbm_purity"] = np.float64(p)
    np.savez_compressed(os.path.join(HERE, "netsmf.npz"), **out)
    print("wrote netsmf.npz:", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
