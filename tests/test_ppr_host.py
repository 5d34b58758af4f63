"""Top-k personalised PageRank, host twin (csrc/host_ppr.cpp) and the ppr_utils shim: the guarantees of the contract
(include/cogdl_hip.h) against an exact float64 solve and against what the reference's own function returned on the same
graphs (tests/golden/ppr.npz, written by tests/golden/make_golden_ppr.py).  No GPU.

Tolerance: 2^-23 covers the float32 rounding of an output value (values <= 1: at most 2^-25) plus the flooring loss that
csrc/ppr_fixed.h proves below 2^-24."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from cogdl_amd import _lib
from cogdl_amd.operators import full_ppr, topk_ppr
from cogdl_amd.operators import ppr as ppr_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "ppr.npz"))
CONFIGS = [(float(a), float(e), int(k)) for a, e, k in GOLDEN["configs"]]
SOURCES = GOLDEN["sources"]
TOL = 2.0 ** -23
GRAPH_NAMES = ("sym", "iso", "directed")


def graph(name):
    return torch.from_numpy(GOLDEN[name + "_indptr"]), torch.from_numpy(GOLDEN[name + "_indices"])


def scipy_graph(name):
    indptr, indices = GOLDEN[name + "_indptr"], GOLDEN[name + "_indices"]
    n = len(indptr) - 1
    return sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))


def exact_ppr(a, alpha, sources):
    deg = np.diff(a.indptr).astype(np.float64)
    dinv = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0)
    m = np.eye(a.shape[0]) - (1.0 - alpha) * (sp.diags(dinv) @ a).toarray()
    return alpha * np.linalg.inv(m)[sources]


def dense_full(name, alpha, eps, sources=SOURCES):
    indptr, indices = graph(name)
    rowptr, nbr, val = full_ppr(indptr, indices, torch.from_numpy(np.asarray(sources)), alpha, eps)
    p = np.zeros((len(sources), indptr.numel() - 1), dtype=np.float64)
    for i in range(len(sources)):
        lo, hi = int(rowptr[i]), int(rowptr[i + 1])
        p[i, nbr[lo:hi].numpy()] = val[lo:hi].numpy()
    return p, (rowptr, nbr, val)


@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("config", range(3))
def test_full_mode_against_the_exact_solve(name, config):
    alpha, eps, _ = CONFIGS[config]
    a = scipy_graph(name)
    deg = np.diff(a.indptr).astype(np.float64)
    p, _ = dense_full(name, alpha, eps)
    diff = exact_ppr(a, alpha, SOURCES) - p
    print("%s config %d: min(pi - p) = %.3e, max (pi - p) / (eps deg) = %.3f"
          % (name, config, diff.min(), (diff / np.maximum(eps * deg, 1e-300)[None, :])[:, deg > 0].max()))
    assert diff.min() >= -TOL
    if name != "directed":
        assert bool((diff < eps * deg[None, :] + TOL).all())


@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("config", range(3))
def test_full_mode_against_the_reference_scores(name, config):
    alpha, eps, _ = CONFIGS[config]
    deg = np.diff(GOLDEN[name + "_indptr"]).astype(np.float64)
    p, _ = dense_full(name, alpha, eps)
    p_ref = GOLDEN["%s_c%d_p" % (name, config)].astype(np.float64)
    union = (p > 0) | (p_ref > 0)
    gap = np.abs(p - p_ref)
    print("%s config %d: max |p - p_ref| / (eps deg + tol) = %.3f over %d entries"
          % (name, config, (gap / (eps * deg[None, :] + TOL))[union].max(), int(union.sum())))
    if name != "directed":  # (both lie in (pi - eps deg, pi] only on a symmetric structure)
        assert bool((gap < eps * deg[None, :] + TOL)[union].all())
    else:
        assert bool((p_ref[:, deg == 0] > 0).any()) and bool((p[:, deg == 0] > 0).any())  # a deg-0 receiver was pushed


@pytest.mark.parametrize("name", GRAPH_NAMES)
@pytest.mark.parametrize("config", range(3))
def test_termination_by_one_exact_propagation_step(name, config):
    """(P1): the residual that p implies, r = alpha e_s + (1 - alpha) (D^-1 A)^T p - p, is below alpha eps deg everywhere.
    Slack: p is known to 2^-25 per entry after the float32 rounding, and r sums at most in-degree + 1 of them, each scaled
    by at most 1, so the slack is (in-degree + 2) * 2^-25; nodes of degree 0 must have r <= slack."""
    alpha, eps, _ = CONFIGS[config]
    a = scipy_graph(name)
    deg = np.diff(a.indptr).astype(np.float64)
    indeg = np.asarray((a != 0).sum(0)).reshape(-1).astype(np.float64)
    dinv = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0)
    p, _ = dense_full(name, alpha, eps)
    r = (1.0 - alpha) * (a.T @ (p * dinv[None, :]).T).T - p
    r[np.arange(len(SOURCES)), SOURCES] += alpha
    slack = (indeg + 2.0) * 2.0 ** -25
    assert bool((r < alpha * eps * deg[None, :] + slack[None, :]).all())
    assert bool((r > -slack[None, :]).all())


@pytest.mark.parametrize("topk", [1, 8, 32, 64, 1000])
def test_topk_is_the_head_of_the_full_output(topk):
    alpha, eps, _ = CONFIGS[0]
    for name in GRAPH_NAMES:
        indptr, indices = graph(name)
        _, (rowptr, f_nbr, f_val) = dense_full(name, alpha, eps)
        nbr, val, count = topk_ppr(indptr, indices, torch.from_numpy(SOURCES), alpha, eps, topk)
        assert nbr.dtype == torch.int64 and val.dtype == torch.float32 and count.dtype == torch.int32
        assert tuple(nbr.shape) == (len(SOURCES), topk) == tuple(val.shape)
        for i in range(len(SOURCES)):
            lo, hi = int(rowptr[i]), int(rowptr[i + 1])
            k = min(topk, hi - lo)
            assert int(count[i]) == k
            assert torch.equal(nbr[i, :k], f_nbr[lo:lo + k]) and torch.equal(val[i, :k], f_val[lo:lo + k])
            assert bool((nbr[i, k:] == -1).all()) and bool((val[i, k:] == 0).all())
            # the order: score descending (the tie rule acts on the fixed-point scores, two of which may round to one
            # float32: test_ties_go_to_the_smaller_id checks it where the scores are equal by symmetry)
            v = f_val[lo:hi].numpy()
            assert bool((v[:-1] >= v[1:]).all()) and bool((v > 0).all())


def test_determinism():
    alpha, eps, topk = CONFIGS[0]
    indptr, indices = graph("sym")
    src = torch.from_numpy(SOURCES)
    a = topk_ppr(indptr, indices, src, alpha, eps, topk)
    b = topk_ppr(indptr, indices, src, alpha, eps, topk)
    perm = torch.randperm(len(src), generator=torch.Generator().manual_seed(0))
    c = topk_ppr(indptr, indices, src[perm].contiguous(), alpha, eps, topk)
    d = topk_ppr(indptr, indices, torch.cat([src[:5], src[:5]]), alpha, eps, topk)
    for x, y, z, w in zip(a, b, c, d):
        assert x.numpy().tobytes() == y.numpy().tobytes()
        assert x[perm].numpy().tobytes() == z.numpy().tobytes()
        assert torch.equal(w[:5], w[5:]) and torch.equal(w[:5], x[:5])


def test_thread_count_does_not_show():
    script = ("import sys, numpy as np, torch; sys.path.insert(0, %r)\n"
              "from cogdl_amd.operators import topk_ppr\n"
              "g = np.load(%r)\n"
              "out = topk_ppr(torch.from_numpy(g['sym_indptr']), torch.from_numpy(g['sym_indices']), torch.from_numpy(g['sources']),"
              " 0.5, 1e-4, 32)\n"
              "sys.stdout.write(''.join(t.numpy().tobytes().hex() for t in out))\n"
              % (ROOT, os.path.join(ROOT, "tests", "golden", "ppr.npz")))
    outs = []
    for threads in ("1", "8"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        proc = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
        assert proc.returncode == 0, proc.stderr[-2000:]
        outs.append(proc.stdout)
    assert len(outs[0]) > 1000 and outs[0] == outs[1]


def test_edges_of_the_contract():
    alpha, eps, _ = CONFIGS[0]
    # an isolated source: p = {s: alpha}
    indptr, indices = graph("iso")
    n = indptr.numel() - 1
    nbr, val, count = topk_ppr(indptr, indices, torch.tensor([n - 1]), alpha, eps, 4)
    assert count.tolist() == [1] and nbr[0].tolist() == [n - 1, -1, -1, -1] and val[0].tolist() == [alpha, 0, 0, 0]
    # a hub source, topk > N, S = 0
    indptr, indices = graph("sym")
    nbr, val, count = topk_ppr(indptr, indices, torch.tensor([0]), alpha, eps, n + 50)
    assert 100 < int(count[0]) <= n and int(nbr[0, 0]) == 0 and bool((nbr[0, int(count[0]):] == -1).all())
    nbr, val, count = topk_ppr(indptr, indices, torch.empty(0, dtype=torch.long), alpha, eps, 8)
    assert tuple(nbr.shape) == (0, 8) and tuple(val.shape) == (0, 8) and count.numel() == 0
    rowptr, f_nbr, f_val = full_ppr(indptr, indices, torch.empty(0, dtype=torch.long), alpha, eps)
    assert rowptr.tolist() == [0] and f_nbr.numel() == 0 and f_val.numel() == 0


def test_errors_are_raised_not_read_out_of_bounds():
    alpha, eps, _ = CONFIGS[0]
    indptr, indices = graph("sym")
    n = indptr.numel() - 1
    for bad_source in (n, -1, 2 ** 40):
        with pytest.raises(_lib.BackendError, match="source id"):
            topk_ppr(indptr, indices, torch.tensor([3, bad_source]), alpha, eps, 8)
    bad = indices.clone()
    bad[int(indptr[0])] = n + 7
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        topk_ppr(indptr, bad, torch.tensor([0]), alpha, eps, 8)
    bad_ptr = indptr.clone()
    bad_ptr[11] = indices.numel() + 1000
    with pytest.raises(_lib.BackendError, match="indptr"):
        topk_ppr(bad_ptr, indices, torch.tensor([10]), alpha, eps, 8)
    with pytest.raises(_lib.BackendError, match="table overflowed"):
        topk_ppr(*graph_with_big_hub(), torch.tensor([0]), 0.5, 0.5, 8, max_source_degree=0)
    for a, e in ((0.0, 1e-4), (1.0, 1e-4), (0.5, 0.0), (0.5, -1.0), (float("nan"), 1e-4), (0.5, 1e-7), (1e-4, 1e-3)):
        with pytest.raises(ValueError):
            topk_ppr(indptr, indices, torch.tensor([0]), a, e, 8)
    with pytest.raises(ValueError):
        topk_ppr(indptr, indices, torch.tensor([0]), alpha, eps, 0)
    with pytest.raises(_lib.BackendError):
        topk_ppr(indptr.int(), indices, torch.tensor([0]), alpha, eps, 8)
    assert ppr_mod.plan(n, indices.numel(), 100, 0.5, 1e-4)["budget"] == 20001


def test_ties_go_to_the_smaller_id():
    """A star: the leaves are exchangeable, so their scores are equal and the ids decide."""
    indptr, indices = graph_with_big_hub()
    nbr, val, count = topk_ppr(indptr, indices, torch.tensor([0, 7]), 0.5, 1e-4, 10)
    assert nbr[0].tolist() == list(range(10)) and bool((val[0, 1:] == val[0, 1]).all())
    assert nbr[1, :2].tolist() == [7, 0] and nbr[1, 2:].tolist() == [1, 2, 3, 4, 5, 6, 8, 9]


def graph_with_big_hub():
    """A star of 2,000 leaves: with a degree bound of 0 and a budget of 5 the table holds 512 nodes."""
    n = 2001
    row = np.concatenate([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)])
    col = np.concatenate([np.arange(1, n), np.zeros(n - 1, dtype=np.int64)])
    a = sp.csr_matrix((np.ones(len(row)), (row, col)), shape=(n, n))
    return torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int64))


@pytest.mark.parametrize("config", [0, 1])
@pytest.mark.parametrize("norm", ["sym", "col", "row"])
def test_compat_matrix_against_the_reference_matrix(config, norm):
    from cogdl_amd import ppr_compat

    alpha, eps, topk = CONFIGS[config]
    a = scipy_graph("sym")
    deg = np.diff(a.indptr).astype(np.float64)
    key = "sym_c%d_%s_" % (config, norm)
    ref = sp.coo_matrix((GOLDEN[key + "val"], (GOLDEN[key + "row"], GOLDEN[key + "col"])), shape=(len(SOURCES), a.shape[0])).tocsr()
    row, col = (torch.from_numpy(x.astype(np.int64)) for x in a.nonzero())
    # a (row, col) tuple too; with duplicate pairs (coalesced: distinct neighbours) where adj.sum(1) does not enter
    dup = 50 if norm == "row" else 0
    for adj in (a, (torch.cat([row, row[:dup]]), torch.cat([col, col[:dup]]))):
        got = ppr_compat.build_topk_ppr_matrix_from_data(adj, alpha, eps, SOURCES, topk, norm, device="cpu")
        assert sp.isspmatrix_csr(got) and got.shape == ref.shape
        # float32 scores times float64 degrees for "sym" / "col", the float32 scores themselves for "row" (what the
        # reference's code yields with numba's float32; the fixture was written with the no-op stub and is all float64)
        assert got.dtype == (np.float32 if norm == "row" else np.float64)
        assert bool((np.diff(got.indptr) == np.minimum(topk, np.diff(ref.indptr))).all())  # a full row wherever the reference has one
        both = got.astype(bool).multiply(ref.astype(bool)).tocoo()
        left_out = 1.0 - both.nnz / ref.nnz
        print("config %d %s: %.3f of the reference's entries are not in this top-%d" % (config, norm, left_out, topk))
        assert left_out <= 0.15
        s, t = SOURCES[both.row], both.col
        scale = {"sym": np.sqrt(deg[s] * deg[t]), "col": deg[s], "row": deg[t]}[norm]
        factor = {"sym": np.sqrt(deg[s] / deg[t]), "col": deg[s] / deg[t], "row": np.ones(len(t))}[norm]
        gap = np.abs(np.asarray(got[both.row, both.col]).reshape(-1) - np.asarray(ref[both.row, both.col]).reshape(-1))
        assert bool((gap < eps * scale + TOL * factor).all())


STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")

INSTALL_SCRIPT = r'''
import os, shutil, sys, tempfile
ROOT, REF, STUB = sys.argv[1], sys.argv[2], sys.argv[3] == "stub"
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
os.chdir(scratch)                                              # pre_transform writes ./pprgo_saved
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import numpy as np, torch
if not hasattr(np, "int"):
    np.int = int
import cogdl_amd
from cogdl_amd import ppr_compat
cogdl_amd.install()
NAMES = ("ppr_topk", "topk_ppr_matrix", "build_topk_ppr_matrix_from_data")
orig = None
if STUB:
    import cogdl.utils.ppr_utils as pu
    orig = {n: getattr(pu, n) for n in NAMES}
    assert all(orig[n].__module__ == "cogdl.utils.ppr_utils" for n in NAMES)
else:
    # numba goes missing for the one module that has not been imported yet (cogdl.utils.sampling needs it at `import cogdl`,
    # so the package as a whole needs at least the stub): ppr_utils then cannot load, and the flag must still work
    import cogdl
    assert "cogdl.utils.ppr_utils" not in sys.modules
    sys.modules["numba"] = None
cogdl_amd.install(ppr=True)
import cogdl.utils.ppr_utils as pu
import cogdl.wrappers.data_wrapper.node_classification.pprgo_dw as dw
import cogdl.models.nn.mvgrl as mv
for n in NAMES:
    assert getattr(pu, n) is getattr(ppr_compat, n), n
assert dw.build_topk_ppr_matrix_from_data is ppr_compat.build_topk_ppr_matrix_from_data
assert mv.build_topk_ppr_matrix_from_data is ppr_compat.build_topk_ppr_matrix_from_data
if not STUB:
    assert pu is ppr_compat

from cogdl.data import Graph
from cogdl.datasets import NodeDataset
n = 2000
g = torch.Generator().manual_seed(0)
ei = torch.randint(0, n, (2, 12000), generator=g)
ei = torch.cat([ei, ei.flip(0)], 1)
data = Graph(edge_index=ei, x=torch.randn(n, 8, generator=g), y=torch.randint(0, 3, (n,), generator=g))
mask = torch.zeros(n, dtype=torch.bool); mask[:400] = True
data.train_mask, data.val_mask, data.test_mask = mask, mask.roll(400), mask.roll(800)
dataset = NodeDataset(data=data, scale_feat=False)
wrapper = dw.PPRGoDataWrapper(dataset, topk=32, alpha=0.5, norm="sym", eps=1e-4)
ppr_dataset = dw.pre_transform(dataset, 32, 0.5, 1e-4, "sym", mode="train")
assert isinstance(ppr_dataset, dw.PPRGoDataset)
assert ppr_dataset.matrix.shape == (400, n) and bool((np.diff(ppr_dataset.matrix.indptr) == 32).all())

cogdl_amd.uninstall()
if STUB:
    for n_ in NAMES:
        assert getattr(pu, n_) is orig[n_], n_
    assert dw.build_topk_ppr_matrix_from_data is orig["build_topk_ppr_matrix_from_data"]
    assert mv.build_topk_ppr_matrix_from_data is orig["build_topk_ppr_matrix_from_data"]
else:
    assert "cogdl.utils.ppr_utils" not in sys.modules
os.chdir(ROOT)
shutil.rmtree(scratch, ignore_errors=True)
print("PPR-INSTALL-OK")
'''


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
@pytest.mark.parametrize("numba", ["stub", "absent"])
def test_install_ppr_against_the_reference_package(numba):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    proc = subprocess.run([sys.executable, "-c", INSTALL_SCRIPT, ROOT, REF, numba], capture_output=True, text=True, timeout=600, env=env)
    assert proc.returncode == 0 and "PPR-INSTALL-OK" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]
