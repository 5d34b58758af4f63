"""The CompGCN layer rebuilt on rel_gspmm (tests/_relational_layer.py) on the GPU against the reference layer recorded in
tests/golden/compgcn_layer.npz (tests/golden/make_golden_relational.py): for both outputs and each gradient

    err_ours = max |ours - ref64|  <=  4 * err_ref,     err_ref = max |ref32 - ref64|

where ref32 / ref64 are the reference layer in float32 / float64.  The tolerance is the reference's own float32 error, not a
chosen number; the factor 4 allows for the different association of the same sums (the weight behind the aggregation, the
kernels' summation order).  A wrong formula is off by about six orders of magnitude."""
import numpy as np
import pytest
import torch

import _relational_layer as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("opn", sorted(L.OPNS))
def test_rebuilt_layer_is_within_the_reference_float32_error(golden, opn):
    z = golden("compgcn_layer")
    got = L.rebuilt_layer(z, opn, DEV)
    report, bad = [], []
    for name in L.NAMES:
        ref32, ref64 = z["%s_%s_f32" % (opn, name)], z["%s_%s_f64" % (opn, name)]
        err_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
        assert err_ref == float(z["ref_err_%s_%s" % (opn, name)]) and err_ref > 0
        err_ours = float(np.abs(got[name].numpy().astype(np.float64) - ref64).max())
        report.append("%s %s: ours %.3e, reference %.3e" % (opn, name, err_ours, err_ref))
        if not err_ours <= 4 * err_ref:
            bad.append(report[-1])
    print("\n".join(report))
    assert not bad, bad
