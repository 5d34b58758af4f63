"""Writes tests/golden/prone/*.npz: what the reference's own functions compute on the two graphs of tests/_prone_cases.py.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs,
PYTHONDONTWRITEBYTECODE=1, and NOT rebound.

  filters_<graph>.npz   propagate(A, a, stype) of cogdl/utils/prone_utils.py for stype in prone / gaussian / heat / ppr with the
                        default parameters (space=None), A the graph's scipy adjacency, a = embedding_input(N, 8) float64
                        -> `a` and one float64 [N, 8] array per kind.
  prefact_ragged.npz    the matrix ProNE._pre_factorization hands to its tSVD (models/emb/prone.py:74-92), captured by
                        replacing _get_embedding_rand: float64 `data` in the CSR order of the graph's own (rowptr, colind).
  dense.npz             get_embedding_dense(dense_input(), 8): `x` and `emb`.
Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "")


def main():
    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "cogdl")):
        raise SystemExit("set COGDL_REFERENCE to a checkout of the reference package")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    import contextlib
    import io

    from cogdl.models.emb import prone as ref_model
    from cogdl.utils import prone_utils as ref

    import _prone_cases as cases

    out_dir = os.path.join(HERE, "prone")
    os.makedirs(out_dir, exist_ok=True)
    for name, make in cases.GRAPHS.items():
        rowptr, colind = make()
        mx = cases.scipy_of(rowptr, colind)
        a = cases.embedding_input(rowptr.size - 1, 8)
        out = {"a": a}
        for kind in cases.KINDS:
            with contextlib.redirect_stdout(io.StringIO()):  # (ProNE.__call__ prints a banner)
                out[kind] = np.asarray(ref.propagate(mx, a.copy(), kind), dtype=np.float64)
            assert out[kind].shape == a.shape and np.isfinite(out[kind]).all()
        np.savez_compressed(os.path.join(out_dir, "filters_%s.npz" % name), **out)

    rowptr, colind = cases.ragged()
    mx = cases.scipy_of(rowptr, colind)
    handed = []
    ref_model.ProNE._get_embedding_rand = lambda self, matrix: handed.append(matrix.copy())
    ref_model.ProNE(8, 5, 0.2, 0.5)._pre_factorization(mx, mx)
    f = handed[0].tocsr()
    f.sort_indices()
    assert np.array_equal(f.indptr, rowptr) and np.array_equal(f.indices, colind), "the pattern is the graph's"
    np.savez_compressed(os.path.join(out_dir, "prefact_ragged.npz"), data=np.asarray(f.data, dtype=np.float64))

    x = cases.dense_input()
    emb = ref.get_embedding_dense(x.copy(), 8)
    np.savez_compressed(os.path.join(out_dir, "dense.npz"), x=x, emb=np.asarray(emb, dtype=np.float64))
    print("wrote", sorted(os.listdir(out_dir)))


if __name__ == "__main__":
    main()
