"""inner_product_bce(route="hip"): the kernels of csrc/recon.hip against the dense float64 formula (tests/_recon_cases.py).

The rule, per case: the error of the route="torch" float32 composition against the float64 reference is the yardstick -- a
float32 evaluation of the same formula with another summation order -- and the kernels stay within 4 times it, for the loss
(|loss - loss64|) and for the gradient, whose error is taken per row in max-norm, |g_i - g64_i|_inf / |g64_i|_inf, the worst
row of the kernels against the worst row of the yardstick.  (Row by row the rule could not be met by any independent float32
evaluation: with 130 rows of one column some row of the yardstick is right to a small fraction of an ulp by chance.)  The 4
covers the tile order, the MFMA's accumulation order and the double fold; nothing is added to it.  Every case also runs twice and
returns equal bytes (no float atomics)."""
import pytest
import torch

import _offset
import _recon_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = ([(n, 3, "dup", None, None) for n in (1, 63, 64, 65, 130)]            # tile edges: diagonal only, first weight-2 tile, ragged
         + [(130, d, "w32", None, None) for d in (1, 32, 33, 256)]             # widths against the k-step of 2 and the widest tile
         + [(130, 33, "dup", None, split) for split in (1, 2, 3)]              # both folds, a ragged last slice
         + [(65, 32, "none", None, None), (65, 32, "dup", 200.0, None)])       # no edges; scores up to +-200


def _hip(split):
    from cogdl_amd.operators.recon import inner_product_bce

    return lambda z, row, col, w: inner_product_bce(z, row, col, w, route="hip", split=split)


def _check(name, got, case):
    from cogdl_amd.operators.recon import inner_product_bce

    want = R.reference(*case)
    yard = R.errors(R.run(lambda z, row, col, w: inner_product_bce(z, row, col, w, route="torch"), *case), want)
    err = R.errors(got, want)
    print("%s: loss %.3e vs %.3e (x%.2f), gradient %.3e vs %.3e (x%.2f)"
          % (name, err[0], yard[0], err[0] / max(yard[0], 1e-300), err[1], yard[1], err[1] / max(yard[1], 1e-300)))
    assert torch.isfinite(got[0]) and torch.isfinite(got[1]).all(), name
    assert err[0] <= 4 * yard[0] and err[1] <= 4 * yard[1], (name, err, yard)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-d%d-%s-scale%s-split%s" % c)
def test_kernels_against_the_float64_formula_and_equal_from_run_to_run(case):
    got = R.run(_hip(case[4]), *case[:4], device=DEV)
    again = R.run(_hip(case[4]), *case[:4], device=DEV)
    _check(str(case), got, case[:4])
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


def test_an_operand_that_starts_mid_allocation():
    case = (130, 32, "w32", None)
    z, row, col, weight = R.inputs(*case)
    view, _ = _offset.shifted(z, 1, device=DEV)  # 4-byte aligned only: the 16-byte loads of d % 4 == 0 do not apply
    view.requires_grad_()
    loss = _hip(None)(view, row.to(DEV), col.to(DEV), weight.to(DEV))
    loss.backward()
    _check("offset", (loss.detach().cpu(), view.grad.cpu()), case)


def test_refusals():
    from cogdl_amd import _lib

    row = torch.zeros(1, dtype=torch.int64, device=DEV)
    for z in (torch.randn(4, 257, device=DEV), torch.randn(4, 8, device=DEV, dtype=torch.float64)):
        with pytest.raises(_lib.BackendError):
            _hip(None)(z, row, row, None)
