"""install(genconv=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present), in a fresh interpreter, on the CPU: GENConv.forward is ours and uninstall()
restores the method object; layers with `softmax_sg` and a learnable beta, `softmax`, `mean` and the plain sum, with and without
the edge encoder, agree with the un-rebound layer under the rule of tests/_gen_cases.py

    err_new <= 4 * err_ref + 8 * eps32 * max|oracle|

for the output and every gradient.  The oracle is the layer on the torch composition in float64 (the reference's own CPU
softmax cannot run in float64: its spmm takes float32 only), err_ref the un-rebound reference layer in float32 against it,
err_new the rebound layer in float32.  The reference runs on its dispatcher's torch route (see torch_route in the script), and
err_ref is asserted to be of rounding size (<= 1e-5 max(1, max|oracle|)), so the rule cannot pass a wrong gradient.  The inputs keep beta * m <= 10, so the halving loop of the reference's CPU softmax (spmm_utils.py:157-160) stays out,
and the script asserts that; `powermean`, `max` and a graph without a CSR reach the reference's forward."""
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
from cogdl_amd import genconv_compat
cogdl_amd.install()
import cogdl
from cogdl.data import Graph
from cogdl.layers.deepergcn_layer import GENConv
from cogdl.utils import spmm_utils
original = GENConv.__dict__["forward"]

def torch_route():
    """The dispatcher's torch route (spmm_scatter) for the reference's CPU softmax.  With an spmm_cpu in place -- the reference's
    own extension, or the one install() serves -- the dispatcher calls it as a raw function for the softmax's denominator
    (spmm_utils.py:110-116), outside autograd: the reference's backward then drops the gradient through the denominator and
    is O(1) away from the softmax's gradient.  install() resets the dispatcher, so this follows every install()."""
    spmm_utils.CONFIGS["spmm_cpu_flag"], spmm_utils.CONFIGS["fast_spmm_cpu"] = True, None

torch_route()
EPS32 = float(np.finfo(np.float32).eps)

torch.manual_seed(0)
N, E, F, A = 60, 420, 12, 5
row, col = torch.randint(0, N - 6, (E,)), torch.randint(0, N, (E,))     # (the last 6 nodes receive nothing)
x0, attr0, G0 = torch.randn(N, F) * 0.8, torch.randn(E, A) * 0.5, torch.randn(N, F)
BETA = 1.5

def make_graph(dtype, attr, csr=True):
    g = Graph(x=x0.to(dtype), edge_index=torch.stack([row, col]), edge_attr=attr0.to(dtype) if attr else None)
    if csr:
        g.row_indptr                                           # the graph holds a CSR (edges re-sorted) before the layer runs
        assert g._adj.row_ptr is not None
    return g

def run(aggr, attr, dtype, state=None, **kw):
    """forward + backward of a fresh layer holding `state` -> ({name: float64 tensor}, state, max beta * m)"""
    torch.set_default_dtype(dtype)
    try:
        layer = GENConv(F, F, aggr=aggr, beta=BETA, learn_beta=True, use_msg_norm=True, learn_msg_scale=True, residual=True,
                        edge_attr_size=[A] if attr else None, **kw).train()
        if state is None:
            state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
        layer.load_state_dict({k: v.to(dtype) for k, v in state.items()})
        graph = make_graph(dtype, attr)
        x = graph.x.clone().requires_grad_()
        out = layer(graph, x)
        (out * G0.to(dtype)).sum().backward()
        got = {"out": out, "grad_x": x.grad}
        got.update({"grad_" + k: p.grad for k, p in layer.named_parameters() if p.grad is not None})
        with torch.no_grad():
            m = x[graph.edge_index[1]]
            if attr:
                m = m + layer.edge_encoder(graph.edge_attr)
            top = float((torch.relu(m) + layer.eps).max()) * (BETA if aggr == "softmax_sg" else 1.0)
        return {k: v.detach().double() for k, v in got.items()}, state, top
    finally:
        torch.set_default_dtype(torch.float32)

CASES = [(aggr, attr) for aggr in ("softmax_sg", "softmax", "mean", "sum") for attr in (False, True)]
assert GENConv.__dict__["forward"] is original                 # the default install() leaves the layer alone
refs = {}
for case in CASES:
    ref32, state, top = run(*case, torch.float32)
    assert top <= 10, (case, top)                                # the reference's halving loop stays out
    assert ("grad_beta" in ref32) == (case[0] == "softmax_sg") and ("grad_edge_encoder.nn.weight" in ref32) == case[1], sorted(ref32)
    refs[case] = (ref32, state)

cogdl_amd.install(genconv=True)
assert GENConv.__dict__["forward"] is genconv_compat.forward
assert cogdl_amd._rebind.original(GENConv, "forward") is original
cogdl_amd.install(genconv=True)                                  # idempotent: the journal keeps the first original
assert cogdl_amd._rebind.original(GENConv, "forward") is original
torch_route()
calls = []
real = genconv_compat.gen_aggregate
genconv_compat.gen_aggregate = lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1]
for case, (ref32, state) in refs.items():
    ref64, _, _ = run(*case, torch.float64, state)               # the oracle: the torch composition in float64
    before = len(calls)
    ours, _, _ = run(*case, torch.float32, state)
    assert len(calls) == before + 1 and calls[-1] == {"softmax_sg": "softmax", "softmax": "softmax", "mean": "mean", "sum": "sum"}[case[0]]
    assert ours.keys() == ref64.keys() == ref32.keys()
    for name in sorted(ref64):
        err_ref = float((ref32[name] - ref64[name]).abs().max())
        err_new = float((ours[name] - ref64[name]).abs().max())
        top64 = float(ref64[name].abs().max())
        bound = 4 * err_ref + 8 * EPS32 * top64
        # err_ref is of float32 rounding size, so the rule is not vacuous.  Inputs, parameters and the upstream gradient are O(1);
        # a summed gradient (grad_beta) may cancel to well below 1 while its rounding error stays that of its O(1) summands, hence
        # the floor of 1 on the scale.  The backward without the denominator's gradient is O(1) off: five orders above this.
        assert err_ref <= 1e-5 * max(1.0, top64), (case, name, err_ref, top64)
        print("%-10s attr=%d %-30s err_new %.3e  err_ref %.3e  bound %.3e" % (case[0], case[1], name, err_new, err_ref, bound))
        assert err_new <= bound, (case, name, err_new, err_ref, bound)

# what the operator does not serve reaches the reference's forward: the operator is not called, the result is the original's
def outcome(fn):
    try:
        return ("ok", fn().detach())
    except Exception as e:                                      # (e.g. max pooling without torch_scatter: the same error either way)
        return (type(e).__name__, None)

before = len(calls)
for aggr in ("powermean", "max"):
    torch.manual_seed(1)
    layer = GENConv(F, F, aggr=aggr)
    xpos = x0.abs() + 0.1
    a = outcome(lambda: layer(make_graph(torch.float32, False), xpos))
    b = outcome(lambda: original(layer, make_graph(torch.float32, False), xpos))
    assert a[0] == b[0] and (a[1] is None or torch.equal(a[1], b[1])), (aggr, a[0], b[0])
layer = GENConv(F, F, aggr="mean")
a = outcome(lambda: layer(make_graph(torch.float32, False, csr=False), x0))
b = outcome(lambda: original(layer, make_graph(torch.float32, False, csr=False), x0))
assert a[0] == b[0] == "ok" and torch.equal(a[1], b[1])
g = make_graph(torch.float32, False)
g.edge_index = (row, col)                                        # same length: the stale row pointer stays (data.py:628-639)
assert g._adj.row_ptr is not None
h = make_graph(torch.float32, False)
h.edge_index = (row, col)
a, b = outcome(lambda: layer(g, x0)), outcome(lambda: original(layer, h, x0))
assert a[0] == b[0] == "ok" and torch.equal(a[1], b[1])
assert len(calls) == before, "an unserved case reached gen_aggregate"
# a graph built from its CSR whose edge_index was never read is served: the layer expands the row pointer first
g, h = make_graph(torch.float32, False), make_graph(torch.float32, False)
g._adj.row = None
a, b = outcome(lambda: layer(g, x0)), outcome(lambda: layer(h, x0))
assert len(calls) == before + 2 and a[0] == b[0] == "ok" and torch.equal(a[1], b[1])
genconv_compat.gen_aggregate = real

cogdl_amd.uninstall()
assert GENConv.__dict__["forward"] is original
shutil.rmtree(scratch, ignore_errors=True)
print("GENCONV-INSTALL-OK")
'''


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_genconv_install_serves_the_reference_layer():
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "GENCONV-INSTALL-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
