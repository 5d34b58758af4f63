"""The reference's `--actnn` family through cogdl.experiment() on the GPU, under install(actnn=True): the actgcn model, the
SAGE model of cogdl/models/nn/graphsage.py with actnn=True (ActSAGELayer; its registered name is `sage` -- the class registered
as `graphsage` is the sampling model, which never reads the flag: it is in the sweep to show that the flag does not break it)
and gcnii with actnn=True (ActGCNIILayer) each train 2 epochs through the unchanged Trainer -- which calls
actnn.set_optimization_level("L3") -- on the synthetic node dataset of the model-zoo sweep (tests/test_reference_zoo_gpu.py,
whose harness and call counters this reuses): finite losses, a falling loss for actgcn without dropout, and the quantiser's HIP
entry points really hit.  Runs in a fresh interpreter."""
import json

import pytest

import test_reference_zoo_gpu as zoo

pytestmark = pytest.mark.gpu

CASES = [("actgcn", "actgcn", {"dropout": 0.0}), ("actgcn_dropout", "actgcn", {}), ("sage", "sage", {}), ("gcnii", "gcnii", {}),
         ("graphsage", "graphsage", {})]
NO_QUANTISER = {"graphsage"}  # (cogdl.models.nn.graphsage.Graphsage takes no actnn argument)

SCRIPT = zoo.COMMON + r'''
import warnings
import cogdl_amd
cogdl_amd.install(actnn=True)
import actnn
from cogdl_amd import actnn_compat
assert actnn is actnn_compat
report = {}
for label, model, kw in json.loads(sys.argv[2]):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        losses, counts = run(model, False, epochs=2, actnn=True, **kw)
    report[label] = {"losses": losses, "counts": counts, "bits": actnn_compat.config.activation_compression_bits,
                     "warned": sum("L2" in str(w.message) for w in seen)}
print("RESULT " + json.dumps(report))
'''


@zoo.needs_ref
def test_the_actnn_models_train_on_the_hip_quantiser():
    rep = zoo._run(SCRIPT, json.dumps(CASES), timeout=600)
    assert sum(r["warned"] for r in rep.values()) == 1, {k: r["warned"] for k, r in rep.items()}  # L3 -> L2, said once
    for label, _, _ in CASES:
        r = rep[label]
        losses, counts = r["losses"], r["counts"]
        assert r["bits"] == [2]
        assert len(losses) == 2 and all(x == x and abs(x) < 1e4 for x in losses), (label, losses)
        if label in NO_QUANTISER:
            continue
        assert counts.get("cogdl_hip_actq_quantize", 0) >= 2 and counts.get("cogdl_hip_actq_dequantize", 0) >= 2, (label, counts)
        assert sum(counts.get(k, 0) for k in zoo.SPARSE_ENTRIES) >= 2, (label, counts)
        if label != "actgcn":
            assert counts.get("cogdl_hip_drop_apply", 0) >= 2, (label, counts)
        assert counts.get("cogdl_hip_relu_mask", 0) >= 1 and counts.get("cogdl_hip_mask_apply", 0) >= 1, (label, counts)
    assert rep["actgcn"]["losses"][1] < rep["actgcn"]["losses"][0], rep["actgcn"]["losses"]
