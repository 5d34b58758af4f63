"""install(actnn=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or $COGDL_REFERENCE;
skipped where neither is present), in a fresh interpreter, on the CPU: `import actnn` gives cogdl_amd.actnn_compat with its
submodules, the reference's act* modules import, uninstall() removes every actnn* module, ActGCN computes GCN's forward and its
weight gradients lie within the bound derived from the quantiser's step, the optimisation levels and the group size behave as
documented, and the reference's own operators/linear.py with its random projection runs on the shim's quantize_activation."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")

SCRIPT = r'''
import os, shutil, sys, tempfile, warnings
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import numpy as np
if not hasattr(np, "int"):
    np.int = int
import torch
import cogdl_amd
from cogdl_amd import _rebind, actnn_compat
from cogdl_amd.operators import actq

cogdl_amd.install()
assert "actnn" not in sys.modules, "plain install() registered actnn"
cogdl_amd.install(actnn=True)
import actnn
assert actnn is actnn_compat
from actnn.ops import quantize_activation, dequantize_activation
from actnn.conf import config
from actnn.qscheme import QScheme
from actnn.layers import QLinear, QReLU, QDropout, QBatchNorm1d
from actnn.utils import empty_cache
assert config is actnn_compat.config and config.activation_compression_bits == [2] and config.group_size == 256
cogdl_amd.install(actnn=True)                                  # idempotent
assert sorted(e[2] for e in _rebind._journal if e[0] == "actnn" and e[1] is sys.modules) == [
    "actnn", "actnn.conf", "actnn.layers", "actnn.ops", "actnn.qscheme", "actnn.utils"]

import cogdl
cogdl_amd.install(actnn=True)
import cogdl.models.nn.actgcn, cogdl.layers.actsage_layer, cogdl.layers.actgcnii_layer, cogdl.layers.actmlp_layer
from cogdl.models.nn.actgcn import ActGCN
from cogdl.models.nn.gcn import GCN
from cogdl.data import Graph
import cogdl.operators.linear as ref_linear
assert ref_linear.quantize_activation is actnn_compat.quantize_activation

# ---- ActGCN against GCN on a 200-node graph, dropout 0 ------------------------------------------------------------------
gen = torch.Generator().manual_seed(0)
N, F, H, C = 200, 48, 64, 7
ei = torch.randint(0, N, (2, 900), generator=gen)
ei = torch.unique(torch.cat([ei, ei.flip(0)], 1), dim=1)
graph = Graph(x=torch.randn(N, F, generator=gen), edge_index=ei)
target = torch.randn(N, C, generator=gen)
torch.manual_seed(3)
gcn = GCN(F, H, C, 3, 0.0)
act = ActGCN(F, H, C, 3, 0.0)
act.load_state_dict(gcn.state_dict())
gcn.train(), act.train()

captured = {}
def keep_grad(i):
    def hook(module, inputs, output):
        captured[i] = (inputs[0].detach(), output)
        output.retain_grad()
    return hook
for i, layer in enumerate(gcn.layers):
    layer.linear.register_forward_hook(keep_grad(i))
out_ref = gcn(graph)
((out_ref - target) ** 2).sum().backward()
exact = [l.linear.weight.grad.clone() for l in gcn.layers]

for bits in (8, 2):
    config.activation_compression_bits = [bits]
    act.zero_grad()
    torch.manual_seed(40 + bits)
    actq.reset_draws()
    out = act(graph)
    assert float((out - out_ref).abs().max()) <= 1e-6 * max(1.0, float(out_ref.abs().max())), "forward differs"
    ((out - target) ** 2).sum().backward()
    for i, layer in enumerate(act.layers):
        x_in, support = captured[i]
        g = support.grad.double().abs()                            # [N, out]: the exact gradient of the layer's product
        q = actq.quantize(x_in, bits, config.group_size, seed=40 + bits, call=i)
        step = q.meta[:, 1].double()[torch.arange(x_in.numel()) // q.group].view_as(x_in)
        bound = g.t().mm(step)                                     # sum_n |g[n, o]| * step[n, i]
        diff = (layer.linear.weight.grad.double() - exact[i].double()).abs()
        assert bool((diff <= bound).all()), (bits, i, float((diff / bound).max()))
        assert float(diff.max()) > 0
        print("bits %d layer %d: max diff / bound = %.3f" % (bits, i, float((diff / bound).max())))
    for a, b in zip(act.layers, gcn.layers):                       # the bias gradient does not see the quantiser
        assert torch.allclose(a.linear.bias.grad, b.linear.bias.grad, rtol=1e-5, atol=1e-5)
config.activation_compression_bits = [2]

# eval mode / no grad: nothing is quantised
calls = []
real_quantize = actq.quantize
actq.quantize = lambda *a, **k: calls.append(1) or real_quantize(*a, **k)
lin, relu, drop, bn = QLinear(8, 8), QReLU(), QDropout(0.5), QBatchNorm1d(8)
x = torch.randn(16, 8)
for m in (lin, relu, drop, bn):
    m.eval()
    m(x)
    m.train()
    with torch.no_grad():
        m(x)
assert not calls
y = bn(lin(x.requires_grad_()))
assert len(calls) == 2
drop(relu(y)).sum().backward()
assert lin.weight.grad is not None and bn.weight.grad is not None and x.grad is not None
actq.quantize = real_quantize

# QBatchNorm1d against nn.BatchNorm1d: same output and running statistics; the backward is native_batch_norm_backward on
# the dequantised input
torch.manual_seed(1)
ref_bn, q_bn = torch.nn.BatchNorm1d(8), QBatchNorm1d(8)
xa = torch.randn(64, 8).requires_grad_()
xb = xa.detach().clone().requires_grad_()
actq.reset_draws()
ya, yb = ref_bn(xa), q_bn(xb)
assert torch.equal(ya, yb) and torch.equal(ref_bn.running_var, q_bn.running_var) and torch.equal(ref_bn.running_mean, q_bn.running_mean)
assert int(q_bn.num_batches_tracked) == 1
w = torch.randn(64, 8)
(yb * w).sum().backward()
x_hat = actq.dequantize(actq.quantize(xb.detach(), 2, 256, seed=1, call=0), xb.shape)
_, save_mean, save_invstd = torch.native_batch_norm(xb.detach(), q_bn.weight, q_bn.bias, None, None, True, 0.1, q_bn.eps)
gi, gw, gb = torch.ops.aten.native_batch_norm_backward(w, x_hat, q_bn.weight, q_bn.running_mean, q_bn.running_var, save_mean,
                                                       save_invstd, True, q_bn.eps, [True, True, True])
assert torch.equal(xb.grad, gi) and torch.equal(q_bn.weight.grad, gw) and torch.equal(q_bn.bias.grad, gb)

# ---- optimisation levels and group size ---------------------------------------------------------------------------------
with warnings.catch_warnings(record=True) as seen:
    warnings.simplefilter("always")
    actnn.set_optimization_level("L3")                             # what Trainer(actnn=True) calls
    actnn.set_optimization_level("L3")
    actnn.set_optimization_level("L4")
assert len(seen) == 1 and "L2" in str(seen[0].message), [str(w.message) for w in seen]
assert config.activation_compression_bits == [2] and config.compress_activation
actnn.set_optimization_level("L1")
assert config.activation_compression_bits == [4]
actnn.set_optimization_level("L0")
assert not config.compress_activation
q = quantize_activation(x.detach(), None)
assert dequantize_activation(q, x.shape) is q.codes                # compression off: the tensor itself
actnn.set_optimization_level("L2")
assert config.activation_compression_bits == [2] and config.compress_activation
config.group_size = 64
assert config.group_size == 64 and quantize_activation(torch.randn(4, 64), None).group == 64
try:
    config.group_size = 100
    raise SystemExit("group_size = 100 was accepted")
except ValueError:
    pass
assert config.group_size == 64

# ---- the reference's own linear with its random projection (rp_ratio = 2, group 64 as Trainer sets it) ------------------
from cogdl.layers.actlinear_layer import QLinear as RefQLinear
torch.manual_seed(5)
layer = RefQLinear(32, 16, rp_ratio=2)
assert layer.scheme is not None and isinstance(layer.scheme, QScheme)
xin = torch.randn(128, 32, requires_grad=True)
out = layer(xin)
assert torch.allclose(out, torch.nn.functional.linear(xin, layer.weight, layer.bias))
out.sum().backward()
assert layer.weight.grad.shape == (16, 32) and bool(torch.isfinite(layer.weight.grad).all()) and xin.grad is not None
config.group_size = 256

# ---- uninstall ------------------------------------------------------------------------------------------------------------
cogdl_amd.uninstall()
left = [m for m in sys.modules if m == "actnn" or m.startswith("actnn.")]
assert not left, left
print("ok")
'''


def test_install_flag_serves_actnn_and_uninstall_removes_it():
    if not REF or not os.path.isdir(os.path.join(REF, "cogdl")):
        pytest.skip("the reference package is not staged (oracle/_ref/pkg) and COGDL_REFERENCE is not set")
    out = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")


def test_the_shim_needs_no_reference_package():
    script = r'''
import sys
sys.path.insert(0, sys.argv[1])
import torch
import cogdl_amd
cogdl_amd.install(actnn=True)
import actnn
from actnn.layers import QLinear, QReLU, QDropout
from cogdl_amd import _lib, actnn_compat
assert actnn is actnn_compat
net = torch.nn.Sequential(QLinear(16, 16), QReLU(), QDropout(0.5), QLinear(16, 4))
net(torch.randn(300, 16)).sum().backward()
assert all(p.grad is not None for p in net.parameters())
cogdl_amd.uninstall()
assert not [m for m in sys.modules if m == "actnn" or m.startswith("actnn.")]
print("ok")
'''
    out = subprocess.run([sys.executable, "-c", script, ROOT], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")


def test_install_signature_has_the_actnn_flag_before_line():
    import inspect

    from cogdl_amd.install import install

    params = list(inspect.signature(install).parameters.values())
    assert params[-1].name == "line" and params[-2].name == "actnn" and params[-2].default is False
