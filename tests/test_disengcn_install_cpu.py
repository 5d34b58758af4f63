"""install(disengcn=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present), in a fresh interpreter, on the CPU: DisenGCNLayer.forward is ours and
uninstall() restores the function object; the rebound layer agrees with the un-rebound one under the rule of tests/_gen_cases.py

    err_new <= 4 * err_ref + 8 * eps32 * max|oracle|

for the output and the gradients of x, weight and bias.  The oracle is the reference's own layer in float64, err_ref the
un-rebound reference layer in float32 against it, err_new the rebound layer in float32.  The reference runs on its dispatcher's
torch route (see torch_route in the script), and err_ref is asserted to be of rounding size, so the rule cannot pass a wrong
gradient.  A graph without a CSR and a graph whose CSR does not describe its edge_index reach the reference's forward."""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import numpy as np
import torch
import cogdl_amd
from cogdl_amd import disengcn_compat
cogdl_amd.install()
import cogdl
from cogdl.data import Graph
from cogdl.layers.disengcn_layer import DisenGCNLayer
from cogdl.utils import spmm_utils
original = DisenGCNLayer.__dict__["forward"]

def torch_route():
    """The dispatcher's torch route (spmm_scatter) for the reference's CPU softmax: with an spmm_cpu in place the dispatcher
    calls it outside autograd for the softmax's denominator and drops that gradient (tests/test_genconv_install_cpu.py).
    install() resets the dispatcher, so this follows every install()."""
    spmm_utils.CONFIGS["spmm_cpu_flag"], spmm_utils.CONFIGS["fast_spmm_cpu"] = True, None

torch_route()
EPS32 = float(np.finfo(np.float32).eps)

torch.manual_seed(0)
N, E, IN = 60, 420, 10
row, col = torch.randint(0, N - 6, (E,)), torch.randint(0, N, (E,))     # (the last 6 nodes receive nothing)
x0 = torch.randn(N, IN)

def make_graph(dtype, csr=True):
    g = Graph(x=x0.to(dtype), edge_index=torch.stack([row, col]))
    if csr:
        g.row_indptr                                           # the graph holds a CSR (edges re-sorted) before the layer runs
        assert g._adj.row_ptr is not None
    return g

def run(width, K, iterations, tau, dtype, state=None):
    """forward + backward of a fresh layer holding `state` -> ({name: float64 tensor}, state)"""
    torch.set_default_dtype(dtype)
    try:
        layer = DisenGCNLayer(IN, width, K, iterations, tau=tau).train()
        if state is None:
            with torch.no_grad():
                layer.bias.copy_(torch.randn(width) * 0.1)
            state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
        layer.load_state_dict({k: v.to(dtype) for k, v in state.items()})
        graph = make_graph(dtype)
        x = graph.x.clone().requires_grad_()
        out = layer(graph, x)
        i, j = torch.arange(N).unsqueeze(1), torch.arange(width).unsqueeze(0)
        (out * (((i * 7 + j * 13) % 11 - 5).to(dtype) / 4)).sum().backward()
        got = {"out": out, "grad_x": x.grad, "grad_weight": layer.weight.grad, "grad_bias": layer.bias.grad}
        return {k: v.detach().double() for k, v in got.items()}, state
    finally:
        torch.set_default_dtype(torch.float32)

CASES = [(24, 3, 3, 1.0), (64, 16, 7, 1.0), (30, 2, 2, 0.5)]      # (d = 8, 4 and 15: the CPU route takes any d)
assert DisenGCNLayer.__dict__["forward"] is original              # the default install() leaves the layer alone
refs = {}
for case in CASES:
    ref32, state = run(*case, torch.float32)
    ref64, _ = run(*case, torch.float64, state)                   # the oracle: the reference's own layer in float64
    refs[case] = (ref32, ref64, state)

cogdl_amd.install(disengcn=True)
assert DisenGCNLayer.__dict__["forward"] is disengcn_compat.forward
assert cogdl_amd._rebind.original(DisenGCNLayer, "forward") is original
cogdl_amd.install(disengcn=True)                                  # idempotent: the journal keeps the first original
assert cogdl_amd._rebind.original(DisenGCNLayer, "forward") is original
torch_route()
calls = []
real = disengcn_compat.neighbor_routing
disengcn_compat.neighbor_routing = lambda *a, **k: (calls.append(a[3:]), real(*a, **k))[1]
for case, (ref32, ref64, state) in refs.items():
    before = len(calls)
    ours, _ = run(*case, torch.float32, state)
    assert len(calls) == before + 1 and calls[-1] == (case[1], case[2], case[3]), calls[-1]
    ours64, _ = run(*case, torch.float64, state)
    assert ours.keys() == ref64.keys() == ref32.keys()
    for name in sorted(ref64):
        err_ref = float((ref32[name] - ref64[name]).abs().max())
        err_new = float((ours[name] - ref64[name]).abs().max())
        top64 = float(ref64[name].abs().max())
        bound = 4 * err_ref + 8 * EPS32 * top64
        # err_ref is of float32 rounding size (amplified by up to 7 normalisations), so the rule is not vacuous: a wrong term
        # in a gradient is O(1e-2) and more.  In float64 the two layers compute the same function to rounding.
        assert err_ref <= 1e-3 * max(1.0, top64), (case, name, err_ref, top64)
        assert float((ours64[name] - ref64[name]).abs().max()) <= 1e-11 * max(1.0, top64), (case, name)
        print("%-18s %-12s err_new %.3e  err_ref %.3e  bound %.3e" % (case, name, err_new, err_ref, bound))
        assert err_new <= bound, (case, name, err_new, err_ref, bound)

# what the operator does not serve reaches the reference's forward: the operator is not called, the result is the original's
before = len(calls)
torch.manual_seed(1)
layer = DisenGCNLayer(IN, 24, 3, 3)
a = layer(make_graph(torch.float32, csr=False), x0).detach()     # no CSR on entry
b = original(layer, make_graph(torch.float32, csr=False), x0).detach()
assert torch.equal(a, b)
g = make_graph(torch.float32)
g.edge_index = (row, col)                                        # same length: the stale row pointer stays (data.py:628-639)
assert g._adj.row_ptr is not None
h = make_graph(torch.float32)
h.edge_index = (row, col)
assert torch.equal(layer(g, x0).detach(), original(layer, h, x0).detach())
assert len(calls) == before, "an unserved case reached neighbor_routing"
layer(make_graph(torch.float32), x0)
assert len(calls) == before + 1
disengcn_compat.neighbor_routing = real

cogdl_amd.uninstall()
assert DisenGCNLayer.__dict__["forward"] is original
shutil.rmtree(scratch, ignore_errors=True)
print("DISENGCN-INSTALL-OK")
'''


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_disengcn_install_serves_the_reference_layer():
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "DISENGCN-INSTALL-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
