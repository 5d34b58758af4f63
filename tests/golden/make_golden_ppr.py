"""Writes tests/golden/ppr.npz: small graphs and what the reference's ppr_utils.py computes on them.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py).  The
reference module is loaded with the no-op numba stub of tests/golden/_stubs and `np.int = int` (it still says np.int).

Graphs (300 nodes): 1,200 random pairs plus a hub (node 0 joined to 100 random nodes), self-pairs dropped;
  sym       symmetrised and coalesced
  iso       the same with nodes 298 and 299 cut off (isolated)
  directed  the pairs as drawn (coalesced, not symmetrised): nodes without out-edges receive mass
Per configuration (alpha, eps, topk) in CONFIGS and every third node as source: the reference's FULL p from
_calc_ppr_node, and topk_ppr_matrix(...) for "sym", "col", "row" (sym graph only) as COO triples.
The script asserts that the share of the reference's top-k entries that are missing from the top-k of the EXACT pi stays
below the cap the tests use (0.15) for the first two configurations."""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "/root/reference")
CONFIGS = ((0.5, 1e-4, 32), (0.4, 1e-4, 8), (0.25, 1e-3, 16))
N = 300
CAP = 0.15


def load_reference():
    import importlib.util

    sys.path.insert(0, os.path.join(HERE, "_stubs"))
    if not hasattr(np, "int"):
        np.int = int
    spec = importlib.util.spec_from_file_location("ref_ppr_utils", os.path.join(REFERENCE_ROOT, "cogdl", "utils", "ppr_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def graphs():
    rng = np.random.default_rng(20240)
    r, c = rng.integers(0, N, 1200), rng.integers(0, N, 1200)
    hub = rng.choice(np.arange(1, N), 100, replace=False)
    r, c = np.concatenate([r, np.zeros(100, dtype=np.int64)]), np.concatenate([c, hub])
    keep = r != c
    r, c = r[keep], c[keep]

    def csr(rows, cols):
        a = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(N, N))
        a.sum_duplicates()
        a.data[:] = 1.0
        a.sort_indices()
        return a

    sym = csr(np.concatenate([r, c]), np.concatenate([c, r]))
    m = (r < N - 2) & (c < N - 2)
    iso = csr(np.concatenate([r[m], c[m]]), np.concatenate([c[m], r[m]]))
    return {"sym": sym, "iso": iso, "directed": csr(r, c)}


def exact_ppr(a, alpha, sources):
    deg = np.diff(a.indptr).astype(np.float64)
    dinv = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0)
    m = np.eye(a.shape[0]) - (1.0 - alpha) * (sp.diags(dinv) @ a).toarray()
    return alpha * np.linalg.inv(m)[sources]


def main():
    ref = load_reference()
    out = {"configs": np.asarray(CONFIGS, dtype=np.float64), "sources": np.arange(0, N, 3, dtype=np.int64)}
    sources = out["sources"]
    for name, a in graphs().items():
        out[name + "_indptr"] = a.indptr.astype(np.int64)
        out[name + "_indices"] = a.indices.astype(np.int64)
        deg = np.diff(a.indptr)
        for ci, (alpha, eps, topk) in enumerate(CONFIGS):
            topk = int(topk)
            p = np.zeros((len(sources), N), dtype=np.float32)
            for i, s in enumerate(sources):
                js, vals = ref._calc_ppr_node(int(s), a.indptr, a.indices, deg, np.float32(alpha), np.float32(eps))
                p[i, np.asarray(js, dtype=np.int64)] = np.asarray(vals, dtype=np.float32)
            out["%s_c%d_p" % (name, ci)] = p
            if name != "sym":
                continue
            pi = exact_ppr(a, alpha, sources)
            for norm in ("sym", "col", "row"):
                mat = ref.topk_ppr_matrix(a, alpha, eps, sources, topk, normalization=norm).tocoo()
                assert mat.shape == (len(sources), N)
                out["%s_c%d_%s_row" % (name, ci, norm)] = mat.row.astype(np.int64)
                out["%s_c%d_%s_col" % (name, ci, norm)] = mat.col.astype(np.int64)
                out["%s_c%d_%s_val" % (name, ci, norm)] = mat.data.astype(np.float64)
                if norm == "row":
                    missing = 0
                    for i in range(len(sources)):
                        top = set(np.lexsort((np.arange(N), -pi[i]))[:topk].tolist())
                        missing += sum(1 for j in mat.col[mat.row == i] if int(j) not in top)
                    share = missing / max(1, mat.nnz)
                    print("config %d: %.3f of the reference's entries are not in the exact top-%d" % (ci, share, topk))
                    if ci < 2:
                        assert share < CAP, share
    path = os.path.join(HERE, "ppr.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
