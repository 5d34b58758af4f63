"""Run by tests/test_diffpool_install_cpu.py and tests/test_diffpool_layer_gpu.py in a fresh interpreter:
`_diffpool_layer_run.py ROOT REF DEVICE`.  The reference's unchanged BatchedDiffPoolLayer under install(diffpool=True) on a batch
of 4 graphs of 1, 5, 33 and 70 nodes, K = 3 and 33, link loss on: adj_new, h, both losses and the gradients of x and of the two
SAGE layers against the reference's own forward in float64 on the CPU.  Per tensor, in max-norm relative to the float64 tensor's:
the reference's float32 CPU run is the yardstick, the served layer on DEVICE stays within 4 times it.  Then what the served
forward does not take reaches the reference's, and uninstall() restores the method object."""
import copy
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

import cogdl_amd
from cogdl_amd import diffpool_compat

cogdl_amd.install()
from cogdl.data import Graph
from cogdl.models.nn.diffpool import BatchedDiffPoolLayer as Layer

original = Layer.__dict__["forward"]
SIZES, F_IN, F_OUT = (1, 5, 33, 70), 8, 6
N, B = sum(SIZES), len(SIZES)
gen = torch.Generator().manual_seed(7)
rows, cols, start = [torch.tensor([N - 1, N - 2])], [torch.tensor([N - 2, N - 1])], 1
for n in SIZES[1:]:  # 3 n random edges inside every graph but the first, whose one node stays isolated
    rows.insert(-1, start + torch.randint(0, n, (3 * n,), generator=gen))
    cols.insert(-1, start + torch.randint(0, n, (3 * n,), generator=gen))
    start += n
row, col = torch.cat(rows), torch.cat(cols)
batch0 = torch.repeat_interleave(torch.arange(B), torch.tensor(SIZES))
x0 = torch.randn(N, F_IN, generator=gen)


def make_graph(dtype, device):
    g = Graph(x=x0.to(dtype), edge_index=torch.stack([row, col])).to(device)
    g.row_indptr  # the graph holds a CSR before the layer runs (on the GPU the SAGE layers' spmm builds it anyway)
    return g


def run(layer, k, dtype, device, g_adj, g_h):
    torch.set_default_dtype(dtype)  # (the reference's row normalisation starts from torch.ones of the default dtype)
    try:
        layer = copy.deepcopy(layer).to(dtype).to(device)
        layer.loss_dict = dict()
        x = x0.clone().to(dtype).to(device).requires_grad_()
        adj_new, h = layer(make_graph(dtype, device), x, batch0.to(device))
        assert tuple(adj_new.shape) == (B * k, B * k) and tuple(h.shape) == (B * k, F_OUT)
        ((adj_new * g_adj.to(dtype).to(device)).sum() + (h * g_h.to(dtype).to(device)).sum() + layer.get_loss()).backward()
        got = {"adj_new": adj_new, "h": h, "grad_x": x.grad, **layer.loss_dict}
        got.update({"grad_" + name: p.grad for name, p in layer.named_parameters()})
        return {name: t.detach().double().cpu() for name, t in got.items()}
    finally:
        torch.set_default_dtype(torch.float32)


cogdl_amd.install(diffpool=True)
cogdl_amd.install(diffpool=True)  # idempotent: the journal keeps the first original
assert Layer.__dict__["forward"] is diffpool_compat.forward and cogdl_amd._rebind.original(Layer, "forward") is original
calls = []
real = diffpool_compat.diffpool_coarsen
diffpool_compat.diffpool_coarsen = lambda *a: (calls.append(a[3].shape), real(*a))[1]

for k in (3, 33):
    # (the seed: one for which the reference's float32 error of either scalar loss is not a small fraction of half an ulp, as
    # it is by chance for many -- a yardstick that no independent float32 evaluation of a scalar could stay within 4 x of)
    torch.manual_seed(10 + k)
    layer = Layer(F_IN, F_OUT, B * k, B, link_pred_loss=True)
    g_adj, g_h = torch.randn(B * k, B * k, generator=gen), torch.randn(B * k, F_OUT, generator=gen)
    Layer.forward = original
    ref64, ref32 = run(layer, k, torch.float64, "cpu", g_adj, g_h), run(layer, k, torch.float32, "cpu", g_adj, g_h)
    Layer.forward = diffpool_compat.forward
    ours = run(layer, k, torch.float32, DEV, g_adj, g_h)
    assert calls[-1] == (N, k) and ours.keys() == ref64.keys() and len(ours) == 9 and "adj_loss" in ours, sorted(ours)
    for name in sorted(ref64):
        top = float(ref64[name].abs().max())
        err_ref, err_ours = (float((t[name] - ref64[name]).abs().max()) / top for t in (ref32, ours))
        print("K=%-2d %-22s ours %.3e  reference in float32 %.3e  (x%.2f)" % (k, name, err_ours, err_ref, err_ours / err_ref))
        assert err_ref > 0 and err_ours <= 4 * err_ref, (k, name, err_ours, err_ref)


# what the served forward does not take reaches the reference's: same outcome, the operator is not called
def outcome(fn, *args):
    try:
        return ("ok",) + tuple(t.detach().cpu() for t in fn(*args))
    except Exception as e:
        return (type(e).__name__,)


def unserved(what):
    torch.manual_seed(0)
    layer = Layer(F_IN, F_OUT, B * 3 + (what == "width"), B, link_pred_loss=True).to(DEV)
    graph, x, batch = make_graph(torch.float32, DEV), x0.to(DEV), batch0.to(DEV)
    if what == "unsorted":
        batch = batch.flip(0)
    elif what == "weight grad":
        graph.edge_weight = torch.rand(row.numel(), device=DEV).requires_grad_()
    elif what == "float64":
        x, layer = x.double(), layer.double()
    elif what == "stale csr":
        graph.edge_index = (row.to(DEV), col.to(DEV))  # same length: the old row pointer stays (data.py:628-639)
    return layer, graph, x, batch


before = len(calls)
for what in ("width", "unsorted", "weight grad", "float64", "stale csr"):
    a, b = outcome(*unserved(what)), outcome(original, *unserved(what))
    print("%-12s -> %s" % (what, a[0]))
    assert a[0] == b[0] and all(torch.equal(s, t) for s, t in zip(a[1:], b[1:])), (what, a[0], b[0])
assert len(calls) == before, "an unserved case reached diffpool_coarsen"

cogdl_amd.uninstall()
assert Layer.__dict__["forward"] is original
shutil.rmtree(scratch, ignore_errors=True)
print("DIFFPOOL-LAYER-OK")
