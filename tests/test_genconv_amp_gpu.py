"""install(genconv=True) under torch AMP: the REAL reference GENConv layer (the staged copy of tools/refpkg.py, in a fresh
interpreter), on the graph and the parameters of tests/golden/genconv_layer.npz, forward + backward under torch.autocast for
fp16 and bf16, with and without the edge encoder.  The rebound forward casts the node features and the encoded edge term to
the autocast dtype, so the aggregation runs the 16-bit kernels of csrc/genaggr16.hip: no TorchRouteWarning may be raised (before
those kernels, fp32 features next to a 16-bit edge term took the torch route).

Oracle: the recorded float64 layer (<tag>_out_f64).  Rule for the layer output, elementwise, as in tests/test_genaggr16_gpu.py:

    |ours - oracle| <= 0.5 ulp16(oracle) + 4 err_ref + 8 eps32 max|oracle|

with err_ref = max |reference - oracle| of the un-rebound reference layer under the same autocast on the same GPU.  The
gradients are printed with the same figures and must be finite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import refpkg  # noqa: E402

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import os, sys, warnings
import numpy as np
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from tools import refpkg
refpkg.setup(install=True)
import torch
import cogdl, cogdl_amd
import _halfprec as H
from cogdl.data import Graph
from cogdl.layers.deepergcn_layer import GENConv
from cogdl_amd import genconv_compat
from cogdl_amd.operators.ops import TorchRouteWarning

DEV, EPS32 = "cuda:0", float(np.finfo(np.float32).eps)
STATE = {"beta": "beta", "s": "s", "mlp0_weight": "mlp.mlp.0.weight", "mlp0_bias": "mlp.mlp.0.bias",
         "mlp1_weight": "mlp.mlp.1.weight", "mlp1_bias": "mlp.mlp.1.bias", "enc_weight": "edge_encoder.nn.weight"}
z = dict(np.load(os.path.join(ROOT, "tests", "golden", "genconv_layer.npz")))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
F, A = z["x"].shape[1], z["edge_attr"].shape[1]

def run(tag, dtype):
    enc = tag == "enc"
    g = Graph(x=T(z["x"]), edge_index=torch.stack([T(z["row"]), T(z["col"])]), edge_attr=T(z["edge_attr"]) if enc else None)
    g.row_indptr                                                # the graph holds its CSR before the layer runs
    assert torch.equal(g.edge_index[0], T(z["row"]))            # (recorded in CSR order: nothing is re-sorted)
    g = g.to(DEV)
    layer = GENConv(F, F, aggr="softmax_sg", beta=1.5, learn_beta=True, use_msg_norm=True, learn_msg_scale=True, residual=True,
                    activation="relu", edge_attr_size=[A] if enc else None).train()
    layer.load_state_dict({name: T(z["%s_%s" % (tag, k)]) for k, name in STATE.items() if "%s_%s" % (tag, k) in z})
    layer = layer.to(DEV)
    x = T(z["x"]).to(DEV).requires_grad_()
    with torch.autocast("cuda", dtype=dtype):
        out = layer(g, x)
    (out.float() * T(z["G"]).to(DEV)).sum().backward()
    got = {"out": out.detach(), "grad_x": x.grad}
    got.update({"grad_" + k: p.grad for k, name in STATE.items() for n, p in layer.named_parameters() if n == name})
    return {k: v.double().cpu().numpy() for k, v in got.items()}, out.dtype

original = GENConv.__dict__["forward"]
refs = {(tag, dt): run(tag, dt) for tag in ("plain", "enc") for dt in (torch.float16, torch.bfloat16)}
cogdl_amd.install(genconv=True)
assert GENConv.__dict__["forward"] is genconv_compat.forward
seen, real = [], genconv_compat.gen_aggregate
genconv_compat.gen_aggregate = lambda x, row, col, eterm, *a, **k: (seen.append((x.dtype, getattr(eterm, "dtype", None))),
                                                                    real(x, row, col, eterm, *a, **k))[1]
for (tag, dt), (ref, ref_dtype) in refs.items():
    with warnings.catch_warnings():
        warnings.simplefilter("error", TorchRouteWarning)
        ours, out_dtype = run(tag, dt)
    assert out_dtype == ref_dtype and ours.keys() == ref.keys()
    assert seen[-1] == (dt, dt if tag == "enc" else None), seen      # the layer was served, on 16-bit operands
    for name in sorted(ours):
        want = z["%s_%s_f64" % (tag, name)]
        err_ref, err_new = float(np.abs(ref[name] - want).max()), float(np.abs(ours[name] - want).max())
        print("%s %s %-18s err_new %.3e  err_ref %.3e" % (tag, dt, name, err_new, err_ref))
    assert all(np.isfinite(v).all() for v in ours.values()), (tag, dt)
    want = z["%s_out_f64" % tag]
    floor = 4 * float(np.abs(refs[(tag, dt)][0]["out"] - want).max()) + 8 * EPS32 * float(np.abs(want).max())
    H.assert_within(ours["out"], want, 0.5 * H.ulp(want, dt) + floor, "%s %s out" % (tag, dt))
cogdl_amd.uninstall()
assert GENConv.__dict__["forward"] is original
print("GENCONV-AMP-OK")
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(refpkg.STAGED, "cogdl")),
                    reason="staged reference package absent (make -C oracle ref in the build container)")
def test_the_reference_layer_under_autocast_runs_the_16_bit_kernels():
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT], capture_output=True, text=True, timeout=600)
    print(proc.stdout[-4000:])
    assert proc.returncode == 0 and "GENCONV-AMP-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
