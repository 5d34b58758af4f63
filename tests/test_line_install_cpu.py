"""install(line=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or $COGDL_REFERENCE;
skipped where neither is present), in a fresh interpreter, on the CPU: LINE.forward is ours and returns what the reference
returns (float64 numpy [N, width] with unit-norm rows, or the dict) without halving model.dimension, the four cases the shim
does not serve reach the reference's own forward, uninstall() restores the function object, and a plain install() leaves
LINE.forward alone.  Without the reference: a CPU graph is served by the host twin and libcogdl_hip.so is not loaded."""
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
from cogdl_amd import _rebind, line_compat
cogdl_amd.install()
import cogdl
from cogdl.data import Graph
import cogdl.utils.sampling
from cogdl.models.emb.line import LINE
original = LINE.__dict__["forward"]
cogdl_amd.install()
assert LINE.__dict__["forward"] is original, "plain install() rebound LINE.forward"
cogdl_amd.install(random_walk=True)
walker = cogdl.utils.sampling.RandomWalker
cogdl_amd.install(line=True)
assert LINE.__dict__["forward"] is line_compat.forward
cogdl_amd.install(line=True)                                   # idempotent: the original is not lost
assert _rebind.original(LINE, "forward") is original
assert [e[0] for e in _rebind._journal if e[1] is LINE] == ["line"]
assert cogdl.utils.sampling.RandomWalker is walker

import _netsmf_cases as cases
indptr, indices, block = cases.sbm_graph()
row = torch.repeat_interleave(torch.arange(128), indptr[1:] - indptr[:-1])
keep = row < indices                                           # one direction only: the edge table is undirected
ei = torch.stack([row[keep], indices[keep]])
graph = Graph(edge_index=ei, num_nodes=128)
for order, width in ((3, 16), (1, 17), (2, 17)):
    model = LINE(16 if order == 3 else 17, 80, 20, 5, 1000, 0.025, order)
    dimension = model.dimension
    torch.manual_seed(1)
    emb = model.forward(graph)
    assert isinstance(emb, np.ndarray) and emb.dtype == np.float64 and emb.shape == (128, width), (emb.dtype, emb.shape)
    halves = (emb[:, :8], emb[:, 8:]) if order == 3 else (emb,)
    assert all(np.allclose(np.linalg.norm(h, axis=1), 1.0, atol=1e-5) for h in halves)
    purity = cases.purity(emb, block)
    print("order %d: purity %.4f" % (order, purity))
    assert purity >= 0.9
    as_dict = model.forward(graph, return_dict=True)
    assert isinstance(as_dict, dict) and sorted(as_dict) == list(range(128)) and as_dict[5].shape == (width,)
    assert model.dimension == dimension, "the shim mutated model.dimension"
# both directions, duplicates and a repeated pair with another weight: one entry per pair, the last weight wins
both = torch.cat([ei, ei.flip(0)], 1)
weight = torch.ones(both.shape[1])
weight[ei.shape[1]] = 4.0                                      # the reverse of pair 0 comes later in edge_index: it wins
from cogdl_amd.embedding import undirected_edges
edges, w = undirected_edges(both[0], both[1], 128, weight)
assert edges.shape[0] == ei.shape[1] and float(w.sum()) == ei.shape[1] + 3.0
first = (edges[:, 0] == min(int(ei[0, 0]), int(ei[1, 0]))) & (edges[:, 1] == max(int(ei[0, 0]), int(ei[1, 0])))
assert int(first.sum()) == 1 and float(w[first]) == 4.0

# what the shim does not serve reaches the reference's forward
calls = []
real_original = _rebind.original
def spy(owner, name):
    assert owner is LINE and name == "forward" and real_original(owner, name) is original
    def reference_forward(self, graph, return_dict=False):
        calls.append((graph, return_dict))
        return "reference"
    return reference_forward
_rebind.original = spy
try:
    model = LINE(16, 2, 2, 5, 1000, 0.025, 3)
    for k, bad in enumerate((0.0, -1.0, float("nan"), float("inf"))):   # weights that are not all finite and positive
        weight = torch.ones(ei.shape[1])
        weight[3] = bad
        weighted = Graph(edge_index=ei, edge_weight=weight, num_nodes=128)
        assert model.forward(weighted, return_dict=True) == "reference" and calls[-1] == (weighted, True) and len(calls) == k + 1
    weight = torch.ones(ei.shape[1])
    weight[3] = 2.5
    served = Graph(edge_index=ei, edge_weight=weight, num_nodes=128)
    assert isinstance(model.forward(served), np.ndarray) and len(calls) == 4           # positive weights: served
    empty = Graph(edge_index=torch.zeros(2, 0, dtype=torch.long), num_nodes=5)
    assert model.forward(empty) == "reference" and len(calls) == 5
    assert LINE(16, 2, 2, 5, 1000, 0.025, 4).forward(graph) == "reference" and len(calls) == 6
    assert LINE(16, 2, 2, 5, 1000, 0.025, 0).forward(graph) == "reference" and len(calls) == 7
    assert LINE(1, 2, 2, 5, 1000, 0.025, 3).forward(graph) == "reference" and len(calls) == 8
    assert isinstance(LINE(1, 2, 2, 5, 1000, 0.025, 2).forward(graph), np.ndarray) and len(calls) == 8
finally:
    _rebind.original = real_original

_rebind.undo("line")                                           # the feature alone: the other rebinds stay
assert LINE.__dict__["forward"] is original
assert cogdl.utils.sampling.RandomWalker is walker
cogdl_amd.install(line=True)
assert LINE.__dict__["forward"] is line_compat.forward
cogdl_amd.uninstall()
assert LINE.__dict__["forward"] is original, "uninstall() did not restore LINE.forward"
print("ok")
'''


def test_install_flag_rebinds_line_and_uninstall_restores_it():
    if not REF or not os.path.isdir(os.path.join(REF, "cogdl")):
        pytest.skip("the reference package is not staged (oracle/_ref/pkg) and COGDL_REFERENCE is not set")
    out = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")


HOST_ROUTE = r'''
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import torch
import _netsmf_cases as cases
from cogdl_amd import _lib, embedding
from cogdl_amd.operators import line_train
indptr, indices, block = cases.sbm_graph()
emb = embedding.line((indptr, indices), dim=16, walk_length=80, walk_num=20, order=3, seed=1)
assert emb.device.type == "cpu" and emb.dtype == torch.float32 and tuple(emb.shape) == (128, 16)
assert cases.purity(emb.numpy(), block) >= 0.9
assert _lib._hip is None and _lib._host is not None, "a CPU graph loaded libcogdl_hip.so"
print("ok")
'''


def test_a_cpu_graph_is_served_by_the_host_twin_without_the_hip_library():
    out = subprocess.run([sys.executable, "-c", HOST_ROUTE, ROOT], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")


def test_install_signature_ends_with_the_line_flag():
    import inspect

    from cogdl_amd.install import install

    params = list(inspect.signature(install).parameters.values())
    assert params[-1].name == "line" and params[-1].default is False
