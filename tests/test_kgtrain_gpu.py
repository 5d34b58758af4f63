"""Knowledge-graph embedding training on the GPU: three AdamW steps of TransE, DistMult, ComplEx and RotatE on a synthetic
200-entity graph (hidden 64, B = 32, K = 16, head-batch and tail-batch in turn) with the scores from the HIP kernels.  The loss
trajectory matches the torch route's on the same device within tests/_kgtrain_cases.py::trajectory_tolerances (measured
against the float64 run, as written there); two runs of the served route end with bit-identical parameters -- the property
the reference's atomic scatter cannot give.  The first test scores through cogdl_amd.kgtrain.score_triples against the gather
composition; the second, where build() has staged the reference package (oracle/_ref/pkg, or $COGDL_REFERENCE), runs the
reference's own models through the forward that install(kg_train=True) rebinds, against the uninstalled reference."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

import _kgtrain_cases as C
from cogdl_amd.kgrank import prepare_query
from cogdl_amd.kgtrain import score_triples
from cogdl_amd.operators.kgscore import gather_composition

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")


def torch_route(model, ent, rel, rng):
    """The reference's arithmetic on torch's kernels: the same query, then the [B, K, D] gather composition."""
    def forward(sample, mode):
        if mode == "single":
            pos, idx, fixed, qmode = sample, sample[:, 2:3], sample[:, 0], "tail-batch"
        else:
            pos, idx = sample
            fixed, qmode = (pos[:, 2] if mode == "head-batch" else pos[:, 0]), mode
        q, kind, gamma = prepare_query(model, qmode, ent[fixed], rel[pos[:, 1]], rng, C.GAMMA)
        return gather_composition(q, ent, idx, kind, gamma)
    return forward


@pytest.mark.parametrize("model", C.MODELS)
def test_three_adamw_steps_match_the_torch_route_and_repeat_bit_for_bit(model):
    ent0, rel0, rng = C.synthetic_tables(model)
    batches = C.synthetic_batches()

    def run(route, dtype):
        ent = ent0.clone().to(device=DEV, dtype=dtype).requires_grad_()
        rel = rel0.clone().to(device=DEV, dtype=dtype).requires_grad_()
        if route == "served":
            fwd = lambda sample, mode: score_triples(model, ent, rel, sample, mode, rng, C.GAMMA)
        else:
            fwd = torch_route(model, ent, rel, rng)
        return C.adamw_run(ent, rel, fwd, batches, DEV)

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the served route stays on the kernels
        served = run("served", torch.float32)
        again = run("served", torch.float32)
    ref32, ref64 = run("torch", torch.float32), run("torch", torch.float64)
    e64, r64 = ent0.double().requires_grad_(), rel0.double().requires_grad_()
    tol = C.trajectory_tolerances(model, ent0, rel0, rng, batches, torch_route(model, e64, r64, rng), ref32[0], ref64[0])
    for t in range(len(batches)):
        print("%s step %d: served %.7f torch32 %.7f float64 %.7f  |served - float64| %.3e  tolerance %.3e"
              % (model, t, served[0][t], ref32[0][t], ref64[0][t], abs(served[0][t] - ref64[0][t]), tol[t]))
        assert abs(served[0][t] - ref64[0][t]) <= tol[t], (model, t)
    assert served[0] == again[0]
    assert torch.equal(served[1].view(torch.int32), again[1].view(torch.int32)), "entity table differs between two runs"
    assert torch.equal(served[2].view(torch.int32), again[2].view(torch.int32)), "relation table differs between two runs"
    assert not torch.equal(served[1], ent0)


SCRIPT = r'''
import os, shutil, sys, tempfile, warnings
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import torch
import cogdl_amd
import _kgtrain_cases as C
cogdl_amd.install()
from cogdl.models.emb.complex import ComplEx
from cogdl.models.emb.distmult import DistMult
from cogdl.models.emb.rotate import RotatE
from cogdl.models.emb.transe import TransE
classes = {"transe": TransE, "distmult": DistMult, "complex": ComplEx, "rotate": RotatE}
DEV = "cuda"
batches = C.synthetic_batches()

def run(name, dtype, device=DEV):
    ent0, rel0, rng = C.synthetic_tables(name)
    model = classes[name](200, 7, 64, C.GAMMA, C.DOUBLE_ENTITY[name], C.DOUBLE_RELATION[name])
    assert abs(model.embedding_range.item() - rng) == 0
    model = model.to(dtype)
    with torch.no_grad():
        model.entity_embedding.copy_(ent0)
        model.relation_embedding.copy_(rel0)
    model = model.to(device)
    return C.adamw_run(model.entity_embedding, model.relation_embedding, lambda sample, mode: model(sample, mode), batches, device)

reference = {name: (run(name, torch.float32), run(name, torch.float64)) for name in C.MODELS}
cogdl_amd.install(kg_train=True)
for name in C.MODELS:
    with warnings.catch_warnings():
        warnings.simplefilter("error")                         # the rebound forward stays on the kernels
        served, again = run(name, torch.float32), run(name, torch.float32)
    ref32, ref64 = reference[name]
    ent0, rel0, rng = C.synthetic_tables(name)
    cpu64 = classes[name](200, 7, 64, C.GAMMA, C.DOUBLE_ENTITY[name], C.DOUBLE_RELATION[name]).double()
    with torch.no_grad():
        cpu64.entity_embedding.copy_(ent0)
        cpu64.relation_embedding.copy_(rel0)
    tol = C.trajectory_tolerances(name, ent0, rel0, rng, batches, lambda s, m: cpu64(s, m), ref32[0], ref64[0])
    for t in range(len(batches)):
        print("%s step %d: served %.7f reference32 %.7f reference64 %.7f  |served - reference64| %.3e  tolerance %.3e"
              % (name, t, served[0][t], ref32[0][t], ref64[0][t], abs(served[0][t] - ref64[0][t]), tol[t]))
        assert abs(served[0][t] - ref64[0][t]) <= tol[t], (name, t)
    assert served[0] == again[0]
    assert torch.equal(served[1].view(torch.int32), again[1].view(torch.int32)), "entity table differs between two runs"
    assert torch.equal(served[2].view(torch.int32), again[2].view(torch.int32)), "relation table differs between two runs"
cogdl_amd.uninstall()
shutil.rmtree(scratch, ignore_errors=True)
print("KG-TRAIN-GPU-OK")
'''


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_rebound_forward_trains_the_reference_models():
    proc = subprocess.run([sys.executable, "-c", SCRIPT, ROOT, REF], capture_output=True, text=True, timeout=600)
    print(proc.stdout[-4000:])
    assert proc.returncode == 0 and "KG-TRAIN-GPU-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
