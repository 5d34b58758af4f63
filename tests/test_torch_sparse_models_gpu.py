"""The reference models that import torch_sparse (srgcn, graph_unet, gtn) on cuda:0 through the unchanged reference code:
once under install(torch_sparse=True) -- spspmm on the HIP SpGEMM, spmm on the COO message operator -- and once with a
pure torch.sparse.mm stand-in registered as `torch_sparse`.  Each leg runs in a fresh interpreter (the models bind
`from torch_sparse import spspmm` at import time).  Follows tests/test_reference_zoo_gpu.py: tools/refpkg, the same
skip condition, the same synthetic node dataset, 2 epochs through cogdl.experiment().

  srgcn  nhop=2 with attention_type ppr and heat (adjacency powers and the PPR chain through spspmm, the node attention's
         learnable diagonal through spspmm with coalesced=True on an unsorted index), normalization row_uniform (spmm);
  unet   aug_adj=True (A . A through spspmm: graph_unet.py moves the index to the CPU, where the shim takes torch.sparse.mm).
         Trained on the CPU: on a GPU the reference's own pooling fails before any spspmm call (Graph.subgraph calls
         .numpy() on the device tensor, cogdl/data/data.py:893), with the real torch_sparse as well;
  gtn    GTLayer on synthetic multi-relation soft adjacencies (experiment() has no offline multi-relation dataset): two
         stacked layers, a loss over the products, gradients into both GTConv weights.
First-epoch losses agree to 1e-4 relative between the legs; the HIP leg really reached the new entry points."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import refpkg  # noqa: E402

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import collections, json, sys, types
import numpy as np
if not hasattr(np, "int"):
    np.int = int  # (the reference still spells the alias numpy 1.24 removed)
ROOT, LEG = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
from tools import refpkg
refpkg.setup(install=True)
import torch
import cogdl_amd
from cogdl_amd import _lib

if LEG == "hip":
    cogdl_amd.install(torch_sparse=True)
    import torch_sparse
    assert torch_sparse.__name__ == "cogdl_amd.torch_sparse_compat"
else:  # a pure torch.sparse.mm stand-in with torch_sparse's contract
    ts = types.ModuleType("torch_sparse")

    def spspmm(indexA, valueA, indexB, valueB, m, k, n, coalesced=False):
        A = torch.sparse_coo_tensor(indexA, valueA, (m, k)).coalesce()
        B = torch.sparse_coo_tensor(indexB, valueB, (k, n)).coalesce()
        C = torch.sparse.mm(A, B).coalesce()
        return C.indices(), C.values()

    def spmm(index, value, m, n, matrix):
        vec = matrix.dim() == 1
        x = matrix.view(-1, 1) if vec else matrix
        out = torch.zeros(m, x.shape[1], dtype=x.dtype, device=x.device).index_add(0, index[0], value.view(-1, 1) * x[index[1]])
        return out.view(-1) if vec else out

    ts.spspmm, ts.spmm = spspmm, spmm
    sys.modules["torch_sparse"] = ts

lib = _lib.hip()
COUNTS = collections.Counter()
def _counting(name, fn):
    def call(*a):
        COUNTS[name] += 1
        return fn(*a)
    return call
for _name in ("cogdl_hip_spgemm_count", "cogdl_hip_spgemm_fill", "cogdl_hip_coo_dupsum", "cogdl_hip_spgemm_grad_a",
              "cogdl_hip_spgemm_grad_b", "cogdl_hip_gspmm"):
    setattr(lib, _name, _counting(_name, getattr(lib, _name)))

report = {}
for label, kw in json.loads(sys.argv[3]):
    COUNTS.clear()
    ds = refpkg.node_dataset(2000, 10000, 32, 5, seed=1)
    cpu = kw.pop("cpu", False)
    res, _ = refpkg.run_experiment(ds, epochs=2, cpu=cpu, seed=0, **kw)
    report[label] = {"losses": [float(l) for l in res["train_losses"]], "counts": dict(COUNTS)}

# gtn: two GTLayers on synthetic soft adjacencies of 3 relations
from cogdl.models.nn.gtn import GTLayer
COUNTS.clear()
torch.manual_seed(0)
dev = torch.device("cuda:0")
N = 600
A = []
g = torch.Generator().manual_seed(3)
for r in range(3):
    e = 3000
    idx = torch.stack([torch.randint(0, N, (e,), generator=g), torch.randint(0, N, (e,), generator=g)])
    idx = torch.unique(idx, dim=1)
    A.append((idx.to(dev), torch.rand(idx.shape[1], generator=g).to(dev)))
l1 = GTLayer(3, 2, N, first=True).to(dev)
l2 = GTLayer(3, 2, N, first=False).to(dev)
H, _ = l1(A)
H, _ = l2(A, H)
w = torch.randn(N, generator=torch.Generator().manual_seed(4)).to(dev)
loss = sum((val * w[idx[0]] * w[idx[1]]).sum() for idx, val in H)
loss.backward()
report["gtn_layers"] = {"losses": [float(loss)], "nnz": [int(v.numel()) for _, v in H], "counts": dict(COUNTS),
                        "grad_norms": [float(l1.conv1.weight.grad.norm()), float(l1.conv2.weight.grad.norm()),
                                       float(l2.conv1.weight.grad.norm())]}
print("RESULT " + json.dumps(report))
'''

MODELS = [("srgcn_ppr", {"model": "srgcn", "nhop": 2, "attention_type": "ppr", "normalization": "row_uniform"}),
          ("srgcn_heat", {"model": "srgcn", "nhop": 2, "attention_type": "heat", "normalization": "row_uniform"}),
          ("unet_aug_adj", {"model": "unet", "aug_adj": True, "cpu": True})]

needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(refpkg.STAGED, "cogdl")),
                               reason="staged reference package absent (make -C oracle ref in the build container)")


def _leg(leg):
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, leg, json.dumps(MODELS)], capture_output=True, text=True,
                          timeout=1200)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")]
    assert proc.returncode == 0 and lines, proc.stdout[-3000:] + proc.stderr[-5000:]
    return json.loads(lines[-1][7:])


@needs_ref
def test_torch_sparse_models_train_on_the_hip_spgemm_like_on_torch_sparse_mm():
    hip, ref = _leg("hip"), _leg("torch")
    for label in [m[0] for m in MODELS] + ["gtn_layers"]:
        h, r = hip[label], ref[label]
        assert len(h["losses"]) == len(r["losses"]) >= 1 and all(x == x for x in h["losses"] + r["losses"]), (label, h, r)
        assert abs(h["losses"][0] - r["losses"][0]) <= 1e-4 * max(1.0, abs(r["losses"][0])), (label, h["losses"], r["losses"])
        assert not r["counts"].get("cogdl_hip_spgemm_count"), (label, r["counts"])
    for label in ("srgcn_ppr", "srgcn_heat", "gtn_layers"):
        c = hip[label]["counts"]
        assert c.get("cogdl_hip_spgemm_count", 0) >= 1 and c.get("cogdl_hip_spgemm_fill", 0) >= 1, (label, c)
        # (srgcn's products are taken on values that carry no gradient; gtn's below carry it into both operands)
    for label in ("srgcn_ppr", "srgcn_heat"):
        assert hip[label]["counts"].get("cogdl_hip_gspmm", 0) >= 1, (label, hip[label]["counts"])  # row_uniform: spmm
    c = hip["gtn_layers"]["counts"]
    assert c.get("cogdl_hip_spgemm_grad_a", 0) >= 1 and c.get("cogdl_hip_spgemm_grad_b", 0) >= 1, c
    assert hip["gtn_layers"]["nnz"] == ref["gtn_layers"]["nnz"]
    assert all(gn > 0 for gn in hip["gtn_layers"]["grad_norms"]), hip["gtn_layers"]
    for a, b in zip(hip["gtn_layers"]["grad_norms"], ref["gtn_layers"]["grad_norms"]):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (hip["gtn_layers"], ref["gtn_layers"])
