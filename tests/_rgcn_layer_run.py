"""Run by tests/test_rgcn_cpu.py and tests/test_rgcn_layer_gpu.py in a fresh interpreter: `_rgcn_layer_run.py ROOT REF DEVICE`.
The reference's unchanged RGCNLayer under install(rgcn=True), both regularisers, in = out = 20, R = 7, on the graph of
tests/_rgcn_cases.py: output and every gradient against the layer's law composed here in float64,

    h[v] = sum_e n_e x[col_e] @ W[t_e],  n_e = 1 / (edges of row[e]);   out = layer_norm(h) + bias + x @ weight_self_loop

within 4 x the error of the same composition in float32 on the CPU; uninstall() restores the two method objects."""
import os
import shutil
import sys
import tempfile

ROOT, REF, DEV = sys.argv[1:4]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")  # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import torch
import torch.nn.functional as F

import _rgcn_cases as C
import cogdl_amd
from cogdl_amd import rgcn_compat

cogdl_amd.install()
from cogdl.data import Graph
from cogdl.layers.rgcn_layer import RGCNLayer

originals = {name: RGCNLayer.__dict__[name] for name in ("basis_forward", "bdd_forward")}
cogdl_amd.install(rgcn=True)
cogdl_amd.install(rgcn=True)  # idempotent
for name, fn in originals.items():
    assert RGCNLayer.__dict__[name] is getattr(rgcn_compat, name) and cogdl_amd._rebind.original(RGCNLayer, name) is fn

row, col, etype = C.coo()
norm = torch.bincount(row, minlength=C.N).double().reciprocal()[row]
torch.manual_seed(0)
x0, G = torch.randn(C.N, 20), torch.randn(C.N, 20)


def law(layer, params, dtype):
    p = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in params.items()}
    x = x0.clone().to(dtype).requires_grad_()
    if layer.regularizer == "basis":
        W = (p["alpha"] @ p["weight"].view(layer.num_bases, -1)).view(C.R, 20, 20)
    else:
        W = torch.stack([torch.block_diag(*blocks) for blocks in p["weight"].view(C.R, layer.num_bases, 5, 5)])
    msg = torch.einsum("ei,eio->eo", x[col], W[etype]) * norm.to(dtype).unsqueeze(-1)
    h = torch.zeros(C.N, 20, dtype=dtype).index_add_(0, row, msg)
    out = F.layer_norm(h, (20,), p["layer_norm.weight"], p["layer_norm.bias"]) + p["bias"] + x @ p["weight_self_loop"]
    out.backward(G.to(dtype))
    got = {"out": out.detach(), "grad_x": x.grad}
    got.update({"grad_" + k: v.grad for k, v in p.items()})
    return {k: v.double() for k, v in got.items()}


for regularizer, num_bases in (("basis", 3), ("bdd", 4)):
    layer = RGCNLayer.__new__(RGCNLayer)
    try:
        layer.__init__(20, 20, C.R, regularizer=regularizer, num_bases=num_bases)
    except AttributeError:  # the reference's reset_parameters reads self.alpha, which its bdd branch never defines
        assert regularizer == "bdd"
        layer.register_buffer("alpha", None)
        layer.reset_parameters()
    with torch.no_grad():
        layer.bias.normal_()
        layer.layer_norm.weight.normal_()
    params = dict(layer.named_parameters())
    ref64, ref32 = law(layer, params, torch.float64), law(layer, params, torch.float32)
    layer = layer.to(DEV)
    graph = Graph(edge_index=torch.stack([row, col]), edge_attr=etype, num_nodes=C.N).to(DEV)
    x = x0.clone().to(DEV).requires_grad_()
    out = layer(graph, x)
    out.backward(G.to(DEV))
    ours = {"out": out.detach(), "grad_x": x.grad}
    ours.update({"grad_" + k: v.grad for k, v in layer.named_parameters()})
    assert ours.keys() == ref64.keys(), sorted(ours)
    for name in sorted(ref64):
        err_ref = float((ref32[name] - ref64[name]).abs().max())
        err_ours = float((ours[name].double().cpu() - ref64[name]).abs().max())
        print("%-5s %-24s ours %.3e  float32 composition %.3e" % (regularizer, name, err_ours, err_ref))
        assert err_ref > 0 and err_ours <= 4 * err_ref, (regularizer, name, err_ours, err_ref)

cogdl_amd.uninstall()
for name, fn in originals.items():
    assert RGCNLayer.__dict__[name] is fn
shutil.rmtree(scratch, ignore_errors=True)
print("RGCN-LAYER-OK")
