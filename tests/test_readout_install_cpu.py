"""install(readout=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present), in a fresh interpreter: every module that holds a pooling function by
name gets ours, the rebound GIN.forward / SortPool.forward return what the originals return, max readout runs on the CPU,
an unsorted batch reaches the original, and uninstall() restores every name and both methods."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")

SCRIPT = r'''
import importlib, os, shutil, sys, tempfile
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import torch
import cogdl_amd
from cogdl_amd import readout_compat
cogdl_amd.install()
import cogdl
from cogdl.data import Graph
from cogdl.models.nn.gin import GIN
from cogdl.models.nn.sortpool import SortPool
HOLDERS = ("cogdl.utils.utils", "cogdl.utils", "cogdl.models.nn.gcc_model", "cogdl.models.nn.infograph",
           "cogdl.layers.deepergcn_layer", "cogdl.layers.set2set")
NAMES = ("batch_sum_pooling", "batch_mean_pooling", "batch_max_pooling")
before = {(m, n): getattr(importlib.import_module(m), n) for m in HOLDERS for n in NAMES
          if hasattr(importlib.import_module(m), n)}
assert len(before) >= 9 and all((m, n) in before for m in HOLDERS[:2] for n in NAMES), sorted(before)
gin_fwd, sp_fwd = GIN.__dict__["forward"], SortPool.__dict__["forward"]

# a synthetic batch of 6 graphs: ring + random chords inside each graph, float32 features, sorted batch vector
torch.manual_seed(0)
sizes = [7, 12, 5, 31, 9, 18]
rows, cols, off = [], [], 0
for n in sizes:
    a = torch.arange(n)
    r = torch.cat([a, torch.randint(0, n, (2 * n,))]); c = torch.cat([(a + 1) % n, torch.randint(0, n, (2 * n,))])
    rows += [r + off, c + off]; cols += [c + off, r + off]; off += n
batch_vec = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
x = torch.randn(off, 16) * 3
x[:, -1] = torch.randperm(off).float() / 7                   # distinct values keep SortPool's keys distinct
def make_batch():
    g = Graph(x=x.clone(), edge_index=(torch.cat(rows), torch.cat(cols)))
    g.batch = batch_vec
    return g

gin = GIN(num_layers=3, in_feats=16, out_feats=4, hidden_dim=32, num_mlp_layers=2).eval()
sortpool = SortPool(16, 24, 3, 2, 8, 5, k=10).eval()
with torch.no_grad():
    want_gin, want_sp = gin(make_batch()), sortpool(make_batch())
xs = torch.randn(off, 5)
from cogdl.utils.utils import batch_sum_pooling as ref_sum, batch_mean_pooling as ref_mean, batch_max_pooling as ref_max
want_sum, want_mean = ref_sum(xs, batch_vec), ref_mean(xs, batch_vec)
try:
    ref_max(xs, batch_vec)
    raise SystemExit("the reference's CPU max readout was expected to need torch_scatter")
except ImportError:
    pass

cogdl_amd.install(readout=True)
for (m, n), fn in before.items():
    assert getattr(sys.modules[m], n) is getattr(readout_compat, n), (m, n)
assert GIN.__dict__["forward"] is readout_compat.gin_forward and SortPool.__dict__["forward"] is readout_compat.sortpool_forward
with torch.no_grad():
    got_gin, got_sp = gin(make_batch()), sortpool(make_batch())
assert torch.equal(got_gin, want_gin), (got_gin - want_gin).abs().max()
assert torch.equal(got_sp, want_sp), (got_sp - want_sp).abs().max()
import cogdl.utils as cu
assert torch.equal(cu.batch_sum_pooling(xs, batch_vec), want_sum) and torch.equal(cu.batch_mean_pooling(xs, batch_vec), want_mean)
mx = cu.batch_max_pooling(xs, batch_vec)
want_max = torch.stack([xs[batch_vec == g].max(0)[0] for g in range(len(sizes))])
assert torch.equal(mx, want_max)
# what the operators do not cover reaches the original: an unsorted batch, float64, a mean over absent ids
perm = torch.randperm(off)
assert torch.allclose(cu.batch_sum_pooling(xs[perm], batch_vec[perm]), want_sum, rtol=1e-5, atol=1e-5)
orig = cogdl_amd._rebind.original(sys.modules["cogdl.utils.utils"], "batch_sum_pooling")
assert orig is before[("cogdl.utils.utils", "batch_sum_pooling")]
try:
    cu.batch_sum_pooling(xs.double(), batch_vec)             # the reference's float32 zeros refuse a float64 src
    raise SystemExit("float64 was expected to reach the reference's function, which raises")
except RuntimeError as e:
    assert not isinstance(e, cogdl_amd._lib.BackendError), e
gaps = torch.tensor([0, 0, 2, 2, 2])
assert cu.batch_sum_pooling(xs[:5], gaps).shape == (3, 5) and not cu.batch_sum_pooling(xs[:5], gaps)[1].any()
try:
    shape = tuple(ref_mean(xs[:5], gaps).shape)
except Exception as e:
    shape = type(e)
try:
    ours = tuple(cu.batch_mean_pooling(xs[:5], gaps).shape)
except Exception as e:
    ours = type(e)
assert ours == shape, (ours, shape)                          # delegated: whatever the reference does there
gb = make_batch(); gb.batch = batch_vec[perm]; gb.x = x[perm]
with torch.no_grad():
    assert gin(gb).shape == want_gin.shape                  # the original forward, through the journal

cogdl_amd.uninstall()
for (m, n), fn in before.items():
    assert getattr(sys.modules[m], n) is fn, (m, n)
assert GIN.__dict__["forward"] is gin_fwd and SortPool.__dict__["forward"] is sp_fwd
shutil.rmtree(scratch, ignore_errors=True)
print("READOUT-INSTALL-OK")
'''


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_readout_install_serves_the_reference_models():
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "READOUT-INSTALL-OK" in proc.stdout, proc.stdout[-2000:] + proc.stderr[-4000:]
