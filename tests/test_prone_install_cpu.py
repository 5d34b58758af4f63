"""install(prone=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present), in a fresh interpreter, on a CPU graph: ProNE.forward and propagate are
ours and return what the reference returns (numpy [N, dim] with unit-norm rows in the reference's node order, or the dict;
float64 numpy of the embedding's shape), the inputs that are not served reach the reference's own functions, and
uninstall() restores the function objects."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")

SCRIPT = r'''
import os, shutil, sys, tempfile
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import numpy as np
import scipy.sparse as sp
import torch
import cogdl_amd
from cogdl_amd import _rebind, prone_compat
cogdl_amd.install()
import cogdl
from cogdl.data import Graph
from cogdl.models.emb.prone import ProNE
import cogdl.utils.prone_utils as prone_utils
import cogdl.models.emb.pronepp as pronepp
original = ProNE.__dict__["forward"]
original_propagate = prone_utils.propagate
assert pronepp.propagate is original_propagate
cogdl_amd.install()
assert ProNE.__dict__["forward"] is original and prone_utils.propagate is original_propagate, "plain install() rebound ProNE"
cogdl_amd.install(prone=True)
assert ProNE.__dict__["forward"] is prone_compat.forward
assert prone_utils.propagate is prone_compat.propagate and pronepp.propagate is prone_compat.propagate
cogdl_amd.install(prone=True)                                  # idempotent: the originals are not lost
assert _rebind.original(ProNE, "forward") is original
assert _rebind.original(prone_utils, "propagate") is original_propagate

import _prone_cases as cases
rowptr, colind = cases.ragged()
row = torch.repeat_interleave(torch.arange(300), torch.from_numpy(np.diff(rowptr)).long())
col = torch.from_numpy(colind).long()
keep = row < col                                               # one direction only: the shim adds the reverse
graph = Graph(edge_index=torch.stack([row[keep], col[keep]]), num_nodes=300)
model = ProNE(8, 5, 0.2, 0.5)
torch.manual_seed(1)
emb = model.forward(graph)
assert isinstance(emb, np.ndarray) and emb.dtype == np.float64 and emb.shape == (300, 8) and np.isfinite(emb).all()
connected = np.diff(rowptr) > 0
assert np.allclose(np.linalg.norm(emb[connected], axis=1), 1.0, atol=1e-5)
assert not emb[~connected].any()                               # the reference's node order: row v belongs to node v
torch.manual_seed(1)
again = model.forward(graph)
assert np.array_equal(emb, again), "not equal from run to run for a seed"
torch.manual_seed(1)
as_dict = model.forward(graph, return_dict=True)
assert isinstance(as_dict, dict) and sorted(as_dict) == list(range(300))
assert all(np.array_equal(as_dict[v], emb[v]) for v in range(300))

# propagate: float64 numpy of the embedding's shape, close to the recorded reference, with and without a parameter dict
mx = cases.scipy_of(rowptr, colind)
gold = cases.load("filters_ragged")
for kind in cases.KINDS:
    out = prone_utils.propagate(mx, gold["a"], kind)
    assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == gold["a"].shape
    assert np.abs(out - gold[kind]).max() <= 1e-4 * np.abs(gold[kind]).max(), kind
for kind, space in (("heat", {"t": 0.3}), ("ppr", {"alpha": 0.3}), ("gaussian", {"mu": 0.3, "theta": 0.7})):
    out = pronepp.propagate(mx, gold["a"], kind, space)
    want = original_propagate(mx, gold["a"].copy(), kind, space)
    assert out.dtype == np.float64 and np.abs(out - want).max() <= 1e-4 * np.abs(want).max(), kind

# what is not served reaches the reference's own functions
calls = []
real_original = _rebind.original
def spy(owner, name):
    assert real_original(owner, name) in (original, original_propagate)
    def reference(*args, **kwargs):
        calls.append((name, args, kwargs))
        return "reference"
    return reference
_rebind.original = spy
try:
    ei = torch.stack(tuple(graph.edge_index))
    weight = torch.ones(ei.shape[1])
    weight[3] = 2.0
    weighted = Graph(edge_index=ei, edge_weight=weight, num_nodes=300)
    assert model.forward(weighted, return_dict=True) == "reference" and len(calls) == 1 and calls[0][0] == "forward"
    equal = Graph(edge_index=ei, edge_weight=torch.full_like(weight, 0.5), num_nodes=300)
    torch.manual_seed(1)
    assert isinstance(model.forward(equal), np.ndarray) and len(calls) == 1      # all weights equal: served
    empty = Graph(edge_index=torch.zeros(2, 0, dtype=torch.long), num_nodes=5)
    assert model.forward(empty) == "reference" and len(calls) == 2
    assert ProNE(8, 1, 0.2, 0.5).forward(graph) == "reference" and len(calls) == 3   # step == 1
    looped = Graph(edge_index=torch.cat([ei, torch.tensor([[4], [4]])], 1), num_nodes=300)
    assert model.forward(looped) == "reference" and len(calls) == 4
    assert prone_utils.propagate(mx, gold["a"], "sc") == "reference" and calls[-1][0] == "propagate"
    assert prone_utils.propagate(mx, gold["a"], "nothing") == "reference"
    assert prone_utils.propagate(mx, gold["a"], "prone", {"mu": 0.1}) == "reference"
    assert prone_utils.propagate(mx * 2.0, gold["a"], "heat") == "reference"      # weighted
    assert prone_utils.propagate(mx + sp.eye(300), gold["a"], "heat") == "reference"  # a diagonal
    assert len(calls) == 9
finally:
    _rebind.original = real_original

_rebind.undo("prone")
assert ProNE.__dict__["forward"] is original
assert prone_utils.propagate is original_propagate and pronepp.propagate is original_propagate
cogdl_amd.install(prone=True)
assert ProNE.__dict__["forward"] is prone_compat.forward
cogdl_amd.uninstall()
assert ProNE.__dict__["forward"] is original, "uninstall() did not restore ProNE.forward"
assert prone_utils.propagate is original_propagate and pronepp.propagate is original_propagate
print("ok")
'''


def test_install_flag_rebinds_prone_and_uninstall_restores_it():
    if not REF or not os.path.isdir(os.path.join(REF, "cogdl")):
        pytest.skip("the reference package is not staged (oracle/_ref/pkg) and COGDL_REFERENCE is not set")
    out = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")
