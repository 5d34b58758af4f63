"""install(graph2vec=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present), in a fresh interpreter, on the CPU: Graph2Vec.forward is ours and returns
what the reference returns (a float array with one row per graph), for the CLI argument order (dm = 1e-4) and for dm = 0; dm = 1
reaches the reference's forward and, through it, NotImplementedError from the shimmed Doc2Vec; uninstall() restores the function
object and sys.modules."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")

SCRIPT = r'''
import argparse, os, shutil, sys, tempfile
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import numpy as np
import torch
import cogdl_amd
from cogdl_amd import _rebind, graph2vec_compat
for name in [n for n in sys.modules if n == "gensim" or n.startswith("gensim.")]:
    del sys.modules[name]
sys.modules["gensim"] = None                                   # from here on the package is absent, whatever the image holds
cogdl_amd.install()
import cogdl
from cogdl.data import Graph
cogdl_amd.install(graph2vec=True)                              # imports the model (and serves gensim where it is absent)
import gensim.models.doc2vec
assert gensim.__name__ == "cogdl_amd.gensim_compat"
from cogdl.models.emb.graph2vec import Graph2Vec
assert Graph2Vec.__dict__["forward"] is graph2vec_compat.forward
original = _rebind.original(Graph2Vec, "forward")
assert original is not None and original.__module__ == "cogdl.models.emb.graph2vec"
cogdl_amd.install(graph2vec=True)                              # idempotent: the original is not lost
assert _rebind.original(Graph2Vec, "forward") is original

from test_graph2vec_cpu import two_families
pairs, family = two_families(count=12)
graphs = [Graph(edge_index=ei) for ei, _ in pairs]
graphs[3].x = torch.ones(int(pairs[3][0].max()) + 1, 2)      # one graph carries features

# the CLI path: build_model_from_args passes `sampling` into dm and `dm` into sampling_rate
args = argparse.Namespace(hidden_size=16, min_count=1, window_size=0, sampling=0.0001, dm=0, iteration=2, epochs=3, lr=0.025)
model = Graph2Vec.build_model_from_args(args)
assert model.dm == 0.0001 and model.sampling_rate == 0
torch.manual_seed(1)
emb = model(graphs)
assert isinstance(emb, np.ndarray) and emb.shape == (12, 16) and emb.dtype == np.float32 and np.isfinite(emb).all()
assert model.doc_collections is None                           # the interpreted extractor did not run

# dm = 0, positional as in __init__(dimension, min_count, window_size, dm, sampling_rate, rounds, epochs, lr)
direct = Graph2Vec(16, 1, 0, 0, 0.0, 2, 3, 0.025)
emb0 = direct.forward(graphs)
assert emb0.shape == (12, 16) and np.isfinite(emb0).all()

# dm = 1 selects PV-DM: the reference's own forward runs (its extractor fills doc_collections) and its Doc2Vec call refuses
pvdm = Graph2Vec(16, 1, 0, 1, 0.0, 2, 3, 0.025, worker=1)
try:
    pvdm.forward(graphs)
except NotImplementedError as e:
    assert "PV-DM" in str(e)
else:
    raise AssertionError("dm = 1 did not raise NotImplementedError")
assert pvdm.doc_collections is not None and len(pvdm.doc_collections) == 12

# an empty list and an x that is not a tensor reach the reference's forward
calls = []
real_original = _rebind.original
def spy(owner, name):
    assert owner is Graph2Vec and name == "forward"
    def reference_forward(self, graphs, **kw):
        calls.append(len(graphs))
        return "reference"
    return reference_forward
_rebind.original = spy
try:
    assert direct.forward([]) == "reference" and calls == [0]
    odd = Graph(edge_index=pairs[0][0])
    odd.x = [[1.0, 2.0]] * 20
    assert direct.forward([odd]) == "reference" and calls == [0, 1]
    star = Graph(edge_index=torch.stack([torch.zeros(32769, dtype=torch.long), torch.arange(1, 32770)]))
    assert direct.forward([star]) == "reference" and calls == [0, 1, 1]   # a row over the degree cap
    assert isinstance(direct.forward(graphs), np.ndarray) and len(calls) == 3   # served again
finally:
    _rebind.original = real_original

cogdl_amd.uninstall()
assert Graph2Vec.__dict__["forward"] is original, "uninstall() did not restore Graph2Vec.forward"
assert sys.modules.get("gensim", None) is None and "gensim.models.doc2vec" not in sys.modules and "gensim.models" not in sys.modules
print("ok")
'''


def test_install_flag_rebinds_graph2vec_and_uninstall_restores_it():
    if not REF or not os.path.isdir(os.path.join(REF, "cogdl")):
        pytest.skip("the reference package is not staged (oracle/_ref/pkg) and COGDL_REFERENCE is not set")
    out = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True,
                         env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")
