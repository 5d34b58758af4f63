"""grace_loss on the GPU against tests/golden/grace_loss.npz (the reference's own contrastive_loss and batched_loss, recorded
by tests/golden/make_golden_grace.py), full and batched, under the rule with the file's ref_err_*.  Reads only the committed
fixture.  (The operator runs torch's kernels on the GPU: cogdl_amd/operators/contrast.py.)"""
import pytest

import _grace_golden as GG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["full", "batched"])
@pytest.mark.filterwarnings("ignore::cogdl_amd.operators.ops.TorchRouteWarning")
def test_grace_loss_reproduces_the_reference_record(golden, tag):
    from cogdl_amd.operators.contrast import grace_loss

    rec = golden("grace_loss")
    loss = lambda a, b: grace_loss(a, b, GG.TAU)
    fn = loss if tag == "full" else (lambda a, b: GG.batched(loss, a, b, GG.BATCH))
    GG.check(tag, GG.run(fn, rec, device="cuda:0"), rec)
