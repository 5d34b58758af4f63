"""The DisenGCN layer rebuilt on neighbor_routing (tests/_disengcn_layer.py) on the GPU against the reference layers recorded in
tests/golden/disengcn_layer.npz (tests/golden/make_golden_disengcn.py): for the output and the gradients of x, weight and bias

    err_new = max |ours - oracle|  <=  4 * err_ref + 8 * eps32 * max|oracle|,     err_ref = max |ref32 - oracle|

where ref32 is the reference's own CPU layer in float32 and the oracle the same layer in float64 -- the rule of
tests/_gen_cases.py.  `small`: 3 channels of 8 columns, 3 iterations; `wide`: 16 channels of 4 columns, 7 iterations."""
import numpy as np
import pytest

import _disengcn_layer as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)


@pytest.mark.parametrize("tag", sorted(L.TAGS))
def test_rebuilt_layer_is_within_the_reference_float32_error(golden, tag):
    z = golden("disengcn_layer")
    got = L.rebuilt_layer(z, tag, DEV)
    report, bad = [], []
    for name in L.NAMES:
        ref32, oracle = z["%s_%s_f32" % (tag, name)], z["%s_%s_f64" % (tag, name)]
        assert ref32.dtype == np.float32 and oracle.dtype == np.float64
        err_ref = float(np.abs(ref32.astype(np.float64) - oracle).max())
        assert err_ref == float(z["ref_err_%s_%s" % (tag, name)])
        err_new = float(np.abs(got[name].numpy().astype(np.float64) - oracle).max())
        bound = 4 * err_ref + 8 * EPS32 * float(np.abs(oracle).max())
        report.append("%s %-12s err_new %.3e  err_ref %.3e  bound %.3e" % (tag, name, err_new, err_ref, bound))
        if not (np.isfinite(got[name].numpy()).all() and err_new <= bound):
            bad.append(report[-1])
    print("\n".join(report))
    assert not bad, bad
