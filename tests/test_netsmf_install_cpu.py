"""install(netsmf=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present), in a fresh interpreter, on the CPU: NetSMF.forward is ours and returns
what the reference returns (float64 numpy [N, dim] with unit-norm rows, or the dict), a weighted graph reaches the
reference's own forward, uninstall() restores the function object, and the other flags' rebinds are left alone."""
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
import torch
import cogdl_amd
from cogdl_amd import _rebind, netsmf_compat
cogdl_amd.install()
import cogdl
from cogdl.data import Graph
import cogdl.utils.sampling
from cogdl.models.emb.netsmf import NetSMF
original = NetSMF.__dict__["forward"]
cogdl_amd.install()
assert NetSMF.__dict__["forward"] is original, "plain install() rebound NetSMF.forward"
cogdl_amd.install(random_walk=True)
walker = cogdl.utils.sampling.RandomWalker
assert walker.__module__ == "cogdl_amd.random_walk_compat"
cogdl_amd.install(netsmf=True)
assert NetSMF.__dict__["forward"] is netsmf_compat.forward
cogdl_amd.install(netsmf=True)                                 # idempotent: the original is not lost
assert _rebind.original(NetSMF, "forward") is original
assert cogdl.utils.sampling.RandomWalker is walker

import _netsmf_cases as cases
indptr, indices, block = cases.sbm_graph()
row = torch.repeat_interleave(torch.arange(128), indptr[1:] - indptr[:-1])
keep = row < indices                                           # one direction only: the shim adds the reverse
graph = Graph(edge_index=torch.stack([row[keep], indices[keep]]), num_nodes=128)
model = NetSMF(8, 5, 1, 100, 1)
torch.manual_seed(1)
emb = model.forward(graph)
assert isinstance(emb, np.ndarray) and emb.dtype == np.float64 and emb.shape == (128, 8)
assert np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-5)
assert cases.purity(emb, block) >= 0.9
torch.manual_seed(1)
as_dict = model.forward(graph, return_dict=True)
assert isinstance(as_dict, dict) and sorted(as_dict) == list(range(128))
assert all(np.array_equal(as_dict[v], emb[v]) for v in range(128))
sym_ip, sym_ix = netsmf_compat.symmetric_csr(graph.edge_index, 128)
assert torch.equal(sym_ip, indptr) and torch.equal(sym_ix, indices)
ei = torch.stack(tuple(graph.edge_index))
doubled = torch.cat([ei, ei, ei.flip(0)], 1)                   # duplicates and reverses: the same graph
assert all(torch.equal(a, b) for a, b in zip(netsmf_compat.symmetric_csr(doubled, 128), (indptr, indices)))

# a weighted graph (and a graph without edges) reaches the reference's forward
calls = []
real_original = _rebind.original
def spy(owner, name):
    assert owner is NetSMF and name == "forward" and real_original(owner, name) is original
    def reference_forward(self, graph, return_dict=False):
        calls.append((graph, return_dict))
        return "reference"
    return reference_forward
_rebind.original = spy
try:
    weight = torch.ones(ei.shape[1])
    weight[3] = 2.0
    weighted = Graph(edge_index=ei, edge_weight=weight, num_nodes=128)
    assert model.forward(weighted, return_dict=True) == "reference" and calls == [(weighted, True)]
    equal = Graph(edge_index=ei, edge_weight=torch.full_like(weight, 0.5), num_nodes=128)
    assert isinstance(model.forward(equal), np.ndarray) and len(calls) == 1      # all weights equal: served
    empty = Graph(edge_index=torch.zeros(2, 0, dtype=torch.long), num_nodes=5)
    assert model.forward(empty) == "reference" and len(calls) == 2
finally:
    _rebind.original = real_original

_rebind.undo("netsmf")                                         # the feature alone: the other rebinds stay
assert NetSMF.__dict__["forward"] is original
assert cogdl.utils.sampling.RandomWalker is walker
cogdl_amd.install(netsmf=True)
assert NetSMF.__dict__["forward"] is netsmf_compat.forward
cogdl_amd.uninstall()
assert NetSMF.__dict__["forward"] is original, "uninstall() did not restore NetSMF.forward"
assert cogdl.utils.sampling.RandomWalker is not walker
print("ok")
'''


def test_install_flag_rebinds_netsmf_and_uninstall_restores_it():
    if not REF or not os.path.isdir(os.path.join(REF, "cogdl")):
        pytest.skip("the reference package is not staged (oracle/_ref/pkg) and COGDL_REFERENCE is not set")
    out = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")
