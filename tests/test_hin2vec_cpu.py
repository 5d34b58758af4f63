"""hin_pairs on the CPU (the OpenMP host twin of csrc/hin2vec.hip) against the Python loop and the law's negative-row
properties, and install(hin2vec=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present) in a fresh interpreter."""
import os
import subprocess
import sys

import pytest
import torch

import _hin2vec_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")


@pytest.mark.parametrize("W,L,hop,negative,T", cases.PAIR_CASES)
def test_host_twin_rows_follow_the_law(W, L, hop, negative, T):
    from cogdl_amd.operators.hin2vec import hin_pairs

    walks, node_type = cases.pair_inputs(W, L, hop, T)
    x, y, key, label = hin_pairs(walks, node_type, hop, negative, seed=11)
    per = 1 + negative
    assert list(zip(x[::per].tolist(), y[::per].tolist(), key[::per].tolist())) == cases.loop_positives(walks, node_type, hop)
    assert bool((label.view(-1, per)[:, 0] == 1).all()) and bool((label.view(-1, per)[:, 1:] == 0).all())
    if negative:
        px, py = (t.view(-1, per)[:, :1] for t in (x, y))
        nx, ny, nkey = (t.view(-1, per)[:, 1:] for t in (x, y, key))
        assert bool((nkey == key.view(-1, per)[:, :1]).all())
        assert bool(((nx != px) ^ (ny != py)).all()), "a negative must differ from its positive in exactly one of x / y"
        assert bool((node_type[nx] == node_type[px]).all()) and bool((node_type[ny] == node_type[py]).all())
        if nx.numel() >= 2000:
            assert bool((nx != px).any()) and bool((ny != py).any()), "only one side is ever replaced"


def test_a_type_with_a_single_node_is_refused_and_bad_walks_are_flagged():
    from cogdl_amd import _lib
    from cogdl_amd.operators.hin2vec import hin_pairs

    walks = torch.tensor([[0, 1, 2, 0]])
    with pytest.raises(_lib.BackendError, match="single node"):
        hin_pairs(walks, torch.tensor([0, 0, 1]), 1, 2, seed=1)
    assert hin_pairs(walks, torch.tensor([0, 0, 1]), 1, 0, seed=1)[0].tolist() == [0, 1, 2]  # nothing is replaced: served
    for bad in ([[0, 3, 1, 0]], [[0, -1, 1, 0]], [[0, -2, 1, 0]]):
        with pytest.raises(_lib.BackendError):
            hin_pairs(torch.tensor(bad), torch.tensor([0, 0, 0]), 1, 1, seed=1)


SCRIPT = r'''
import os, shutil, sys, tempfile
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import numpy as np
import torch
import cogdl_amd
from cogdl_amd import _rebind, hin2vec_compat
cogdl_amd.install()
from cogdl.data import Graph
from cogdl.models.emb.hin2vec import Hin2vec
original = Hin2vec.__dict__["forward"]
cogdl_amd.install()
assert Hin2vec.__dict__["forward"] is original, "plain install() rebound Hin2vec.forward"
cogdl_amd.install(hin2vec=True)
cogdl_amd.install(hin2vec=True)                                # idempotent: the original is not lost
assert Hin2vec.__dict__["forward"] is hin2vec_compat.forward and _rebind.original(Hin2vec, "forward") is original
assert [e[0] for e in _rebind._journal if e[1] is Hin2vec] == ["hin2vec"]

n = 30
src = torch.arange(n)
ei = torch.stack([torch.cat([src, src]), torch.cat([(src + 1) % n, (src + 4) % n])])
graph = Graph(edge_index=ei, pos=src % 3)
model = Hin2vec(8, 6, 2, 50, 2, 3, 1, 0.025, True)
emb = model.forward(graph)
assert isinstance(emb, np.ndarray) and emb.dtype == np.float32 and emb.shape == (n, 8) and np.isfinite(emb).all()

calls = []
real_original = _rebind.original
def spy(owner, name):
    assert owner is Hin2vec and name == "forward" and real_original(owner, name) is original
    return lambda self, data: calls.append(data) or "reference"
_rebind.original = spy
try:
    assert Hin2vec(8, 6, 2, 50, 9, 3, 1, 0.025, True).forward(graph) == "reference" and len(calls) == 1     # hop > 8
    gap = Graph(edge_index=ei + 1, pos=torch.arange(n + 1) % 3)                                             # node 0 in no edge
    assert model.forward(gap) == "reference" and len(calls) == 2
finally:
    _rebind.original = real_original
cogdl_amd.uninstall()
assert Hin2vec.__dict__["forward"] is original, "uninstall() did not restore Hin2vec.forward"
print("ok")
'''


def test_install_flag_rebinds_hin2vec_and_uninstall_restores_it():
    if not REF or not os.path.isdir(os.path.join(REF, "cogdl")):
        pytest.skip("the reference package is not staged (oracle/_ref/pkg) and COGDL_REFERENCE is not set")
    out = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")
