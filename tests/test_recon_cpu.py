"""inner_product_bce without a GPU: the blocked torch composition on CPU tensors against the dense float64 formula
(tests/_recon_cases.py), what it refuses, and install(recon=True) against the REAL reference package (the copy build() stages
under oracle/_ref/pkg, or $COGDL_REFERENCE) in a fresh interpreter."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

import _recon_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")
EPS32 = 2.0 ** -24


@pytest.mark.parametrize("case", [(1, 3, "dup", None), (65, 3, "dup", None), (130, 33, "w32", None), (130, 256, "none", None),
                                  (65, 32, "dup", 200.0)], ids=str)
def test_blocked_composition_against_the_float64_formula(case):
    """Bounds from a forward error analysis of a float32 evaluation, with A_ij = SUM_c |z_ic z_jc|: a dot product of d terms is
    off by at most d eps A_ij, softplus and sigmoid do not amplify that, and a sum of n terms in any order by at most n eps
    times the sum of their magnitudes -- n <= N + 32 covers torch's blocked sums of N^2 terms and the block and edge sums.  So
    |loss err| <= (N + d + 32) eps (SUM_ij softplus(A_ij) + SUM_e w_e A_e), and row i of the gradient by the same factor times
    2 SUM_j (1 + A_ij) |z_j|_inf + SUM_{edges at i} w_e |z_other|_inf."""
    from cogdl_amd.operators.recon import inner_product_bce

    got = R.run(lambda z, row, col, w: inner_product_bce(z, row, col, w, route="torch", block=16), *case)
    want = R.reference(*case)
    z, row, col, weight = R.inputs(*case)
    z, row, col = z.double(), row.long(), col.long()
    w = torch.ones(row.numel(), dtype=torch.float64) if weight is None else weight.double()
    n, d = z.shape
    factor, A, zmax = (n + d + 32) * EPS32, z.abs() @ z.abs().t(), z.abs().amax(1)
    assert abs(float(got[0] - want[0])) <= factor * float(torch.nn.functional.softplus(A, threshold=1e4).sum()
                                                                  + (w * A[row, col]).sum())
    size = 2 * ((1 + A) * zmax).sum(1)
    size = size.index_add(0, row, w * zmax[col]).index_add(0, col, w * zmax[row])
    assert bool(((got[1].double() - want[1]).abs().amax(1) <= factor * size).all())


def test_empty_inputs_and_refusals():
    from cogdl_amd import _lib
    from cogdl_amd.operators.recon import inner_product_bce

    none = torch.zeros(0, dtype=torch.int64)
    assert float(inner_product_bce(torch.zeros(0, 4), none, none)) == 0.0
    assert float(inner_product_bce(torch.zeros(2, 4), none, none)) == pytest.approx(4 * 0.6931471805599453, rel=1e-6)
    z, one = torch.randn(5, 4), torch.ones(1, dtype=torch.int64)
    for bad in ((z[0], one, one), (z, 5 * one, one), (z, one, -one), (z, one, none), (z, one.float(), one), (z.long(), one, one),
                (z, one, one, torch.ones(2))):
        with pytest.raises(_lib.BackendError):
            inner_product_bce(*bad)
    for route in ("hip", "rocm"):  # the kernels do not serve CPU tensors; an unknown route
        with pytest.raises(_lib.BackendError):
            inner_product_bce(z, one, one, route=route)


def test_install_flag_is_off_by_default():
    import cogdl_amd

    assert inspect.signature(cogdl_amd.install).parameters["recon"].default is False


SCRIPT = r'''
import os, shutil, sys, tempfile, types
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import torch
import cogdl_amd
from cogdl_amd import recon_compat
cogdl_amd.install()
from cogdl.data import Graph
from cogdl.models.nn.gae import GAE, VGAE
from cogdl.models.nn.daegc import DAEGC
from cogdl.wrappers.model_wrapper.clustering.gae_mw import GAEModelWrapper
places = ((VGAE, "make_loss"), (DAEGC, "recon_loss"), (GAEModelWrapper, "pre_stage"))
originals = [owner.__dict__[name] for owner, name in places]

N, F, H = 20, 6, 4
gen = torch.Generator().manual_seed(3)
x = torch.randn(N, F, generator=gen)
src = torch.randint(0, N, (40,), generator=gen)
dst = (src + 1 + torch.randint(0, N - 1, (40,), generator=gen)) % N                  # no self loops
pairs = torch.unique(torch.cat([torch.stack([src, dst]), torch.stack([dst, src])], 1), dim=1)   # symmetric, no duplicates
graph = lambda: Graph(x=x.clone(), edge_index=(pairs[0].clone(), pairs[1].clone()))
adj = torch.sparse_coo_tensor(pairs, torch.ones(pairs.shape[1]), (N, N)).to_dense()
torch.manual_seed(0)
model = VGAE(F, H)

def step(fn, *args):
    model.zero_grad()
    torch.manual_seed(7)                                                              # the noise of reparameterize
    loss = fn(model, *args)
    loss.backward()
    return loss.detach().double(), [p.grad.clone().double() for p in model.parameters()]

ref_loss, ref_grads = step(originals[0], graph(), adj)
cogdl_amd.install(recon=True)
cogdl_amd.install(recon=True)                                                         # idempotent
for (owner, name), fn, before in zip(places, (recon_compat.make_loss, recon_compat.recon_loss, recon_compat.pre_stage), originals):
    assert owner.__dict__[name] is fn and cogdl_amd._rebind.original(owner, name) is before, name

# the reference's own error: 1 - sigmoid(s) is rounded to half an ulp of 1 and its log amplifies that by 1 / (1 - sigmoid(s))
# = 1 + e^s; so each of the N^2 terms is off by at most eps (e^smax + 8), and the gradients in proportion
torch.manual_seed(7)
with torch.no_grad():
    z = model(graph())
smax = float((z @ z.t()).abs().max())
assert smax < 10, smax
tol = N * N * 2.0 ** -24 * (torch.e ** smax + 8)
for adj_arg in (adj, None):                                                           # `adj` is ignored
    loss, grads = step(VGAE.make_loss, graph(), adj_arg)
    assert abs(float(loss - ref_loss)) <= tol, (float(loss), float(ref_loss), tol)
    for g, r in zip(grads, ref_grads):
        assert float((g - r).abs().max()) <= tol / float(ref_loss) * max(1.0, float(r.abs().max())), (g, r)

daegc = DAEGC(F, 8, H, 1, 0.0, 3)
zz = 0.5 * torch.randn(N, H, generator=gen)
ours = daegc.recon_loss(zz, edge_index=(pairs[0], pairs[1]))
dense = daegc.recon_loss(zz, adj)                                                     # a dense adj: the reference's method
assert torch.equal(dense, originals[1](daegc, zz, adj))
assert abs(float(ours) - float(dense)) <= N * N * 2.0 ** -24 * (torch.e ** float((zz @ zz.t()).abs().max()) + 8)

for net, dense_adj in ((model, False), (GAE(F, H, 2, 0.0), True)):
    g = graph()
    data_w = types.SimpleNamespace(get_dataset=lambda: types.SimpleNamespace(data=g))
    GAEModelWrapper(net, {"lr": 0.01, "weight_decay": 0.0}, 3).pre_stage(0, data_w)
    if dense_adj:
        assert torch.equal(g.adj_mx, adj) and getattr(g, "recon_index", None) is None
    else:
        assert g.adj_mx is None and torch.equal(g.recon_index, torch.stack(g.edge_index))

cogdl_amd.uninstall()
assert [owner.__dict__[name] for owner, name in places] == originals
shutil.rmtree(scratch, ignore_errors=True)
print("RECON-INSTALL-OK")
'''


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_recon_install_serves_the_reference_auto_encoders():
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "RECON-INSTALL-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
