"""install(relational=True) against the REAL reference package (the copy build() stages under oracle/_ref/pkg, or
$COGDL_REFERENCE; skipped where neither is present), in a fresh interpreter: CompGCNLayer.message_passing is ours, a two-layer
CompGCN forward + backward matches the un-rebound model within 4 x the reference's own float32 error (measured against a
float64 run of the same model), an unsupported `opn` reaches the original method, and uninstall() restores the method object."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")

SCRIPT = r'''
import os, shutil, sys, tempfile, types
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import torch
import cogdl_amd
from cogdl_amd import relational_compat
cogdl_amd.install()
import cogdl
from cogdl.models.nn.compgcn import CompGCN, CompGCNLayer
original = CompGCNLayer.__dict__["message_passing"]

# a small typed graph: 120 entities, 4 relations plus their reverses, 700 edges per direction, 10 -> 16 -> 8
torch.manual_seed(0)
N, R, E = 120, 4, 700
src, dst, typ = torch.randint(0, N, (E,)), torch.randint(0, N - 10, (E,)), torch.randint(0, R, (E,))
graph = types.SimpleNamespace(edge_index=(torch.cat([dst, src]), torch.cat([src, dst])), edge_attr=torch.cat([typ, typ + R]))
x0, g_node, g_rel = torch.randn(N, 10), torch.randn(N, 8), torch.randn(2 * R, 8)

def run(opn, dtype, state=None):
    """forward + backward of a fresh two-layer model holding `state` -> ({name: tensor}, state)"""
    torch.set_default_dtype(dtype)                            # (the layer allocates its zeros and ones in the default dtype)
    try:
        model = CompGCN(N, R, 0, 10, 16, 8, 2, 0.0, torch.tanh, opn).train()
        if state is None:
            state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state)
        x = x0.clone().to(dtype).requires_grad_()
        node, rel = model(graph, x)
        ((node * g_node.to(dtype)).sum() + (rel * g_rel.to(dtype)).sum()).backward()
        got = {"node": node, "rel": rel, "grad_x": x.grad}
        got.update({"grad_" + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
        return {k: v.detach().double() for k, v in got.items()}, state
    finally:
        torch.set_default_dtype(torch.float32)

refs = {}
for opn in ("sub", "mult"):
    ref32, state = run(opn, torch.float32)
    ref64, _ = run(opn, torch.float64, state)
    refs[opn] = (ref32, ref64, state)
    assert len(ref32) >= 12 and ref32.keys() == ref64.keys(), sorted(ref32)

cogdl_amd.install(relational=True)
assert CompGCNLayer.__dict__["message_passing"] is relational_compat.message_passing
assert cogdl_amd._rebind.original(CompGCNLayer, "message_passing") is original
cogdl_amd.install(relational=True)                           # idempotent: the journal keeps the first original
assert cogdl_amd._rebind.original(CompGCNLayer, "message_passing") is original
for opn, (ref32, ref64, state) in refs.items():
    ours, _ = run(opn, torch.float32, state)
    assert ours.keys() == ref64.keys()
    for name in sorted(ref64):
        err_ref = float((ref32[name] - ref64[name]).abs().max())
        err_ours = float((ours[name] - ref64[name]).abs().max())
        print("%-5s %-28s ours %.3e  reference %.3e" % (opn, name, err_ours, err_ref))
        assert err_ref > 0 and err_ours <= 4 * err_ref, (opn, name, err_ours, err_ref)

# an unsupported composition reaches the original method, which refuses it as before
layer = CompGCNLayer(10, 16, R, opn="corr")
try:
    layer.message_passing(x0, torch.randn(2 * R + 1, 10), graph.edge_index, graph.edge_attr, "in")
    raise SystemExit("opn='corr' was expected to reach the reference's method, which raises NotImplementedError")
except NotImplementedError as e:
    assert "corr" in str(e)

cogdl_amd.uninstall()
assert CompGCNLayer.__dict__["message_passing"] is original
shutil.rmtree(scratch, ignore_errors=True)
print("RELATIONAL-INSTALL-OK")
'''


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_relational_install_serves_the_reference_model():
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "RELATIONAL-INSTALL-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
