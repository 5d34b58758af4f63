"""segment_matmul_tn / segment_matmul_nn (route="hip"): the kernels of csrc/segmm.hip against the float64 loop over the segments
(tests/_segmm_cases.py), forward and every gradient.  The rule is tests/test_recon_gpu.py's, per tensor: the error of the
route="torch" float32 composition against float64, in max-norm relative to the reference's max-norm, is the yardstick (nonzero
for these seeds, asserted), and the kernels stay within 4 times it.  The 4 covers the tile order, the MFMA's accumulation order
and the slice merge; nothing is added to it.  Every case runs twice and returns equal bytes."""
import pytest
import torch

import _offset
import _segmm_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators import segmm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TN_CASES = ([("ragged", k, (33,), False, None) for k in (1, 31, 32, 33, 65)]          # edges of the 32 / 64 tiles of S's columns
            + [("ragged", 33, (f,), False, None) for f in (1, 4, 64, 65)]             # .. and of a panel's columns
            + [("ragged", 33, (4, 65), False, None), ("ragged", 33, (64, 33), True, None),   # two and three panels, one tile group
               ("ragged", 65, (65, 130), True, None), ("front", 33, (33,), True, None)]      # 7 column tiles: two groups
            + [("ragged", 33, (33, 4), True, split) for split in (1, 2, 3)]           # the fold; 3 leaves ragged last slices
            + [("one", 32, (64,), True, 3)])                                          # B = 1
NN_CASES = [("ragged", 1, 65, False), ("ragged", 31, 1, False), ("ragged", 32, 33, True), ("ragged", 33, 32, False),
            ("ragged", 65, 4, True), ("ragged", 64, 130, False), ("front", 33, 33, True), ("one", 33, 33, False)]


def _within(name, got, want, yard):
    err, yard = C.errors(got, want), C.errors(yard, want)
    for k in sorted(want):
        print("%s %-8s kernels %.3e  torch route %.3e  (x%.2f)" % (name, k, err[k], yard[k], err[k] / max(yard[k], 1e-300)))
        assert torch.isfinite(got[k]).all() and yard[k] > 0 and err[k] <= 4 * yard[k], (name, k, err[k], yard[k])


def _tn(route, split=None):
    return lambda s, panels, ptr: segmm.segment_matmul_tn(s, panels, ptr, route=route, split=split)


@pytest.mark.parametrize("case", TN_CASES, ids=lambda c: "%s-K%d-F%s-s%d-split%s" % c)
def test_tn_against_the_float64_loop_and_equal_from_run_to_run(case):
    got, again = (C.run_tn(_tn("hip", case[4]), case, device=DEV) for _ in range(2))
    _within(str(case), got, C.reference_tn(case[:4]), C.run_tn(_tn("torch"), case))
    assert all(torch.equal(got[k], again[k]) for k in got)


@pytest.mark.parametrize("case", NN_CASES, ids=lambda c: "%s-P%d-Q%d-acc%d" % c)
def test_nn_against_the_float64_loop_and_equal_from_run_to_run(case):
    nn = lambda route: (lambda x, w, ptr: segmm.segment_matmul_nn(x, w, ptr, route=route))
    got, again = (C.run_nn(nn("hip"), case, device=DEV) for _ in range(2))
    want, yard = C.reference_nn(case[:3]), C.run_nn(nn("torch"), case)
    if case[3]:  # the launch that adds to what is there: base + x w against the same sum in float64 and in float32
        x, w, _, base = C.nn_inputs(*case[:3])
        for out in (got, again):
            out["acc"] = segmm._nn_raw(x.to(DEV), w.to(DEV), C.ptr_of(case[0]).to(DEV), out=base.to(DEV).clone()).cpu()
        want, yard = dict(want, acc=base.double() + want["out"]), dict(yard, acc=base + yard["out"])
    _within(str(case), got, want, yard)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_operands_that_start_mid_allocation():
    case = ("ragged", 32, (64,), True, None)  # widths that would allow 16-byte loads, 4 bytes into the allocation
    got = C.run_tn(_tn("hip"), case, device=DEV, shift=lambda t: _offset.shifted(t, 1, device=DEV)[0])
    _within("offset", got, C.reference_tn(case[:4]), C.run_tn(_tn("torch"), case))


def test_refusals():
    tn, nn = segmm.segment_matmul_tn, segmm.segment_matmul_nn
    s, x, ptr = torch.randn(6, 3, device=DEV), torch.randn(6, 5, device=DEV), torch.tensor([0, 2, 6], device=DEV)
    w = torch.randn(2, 3, 4, device=DEV)
    for call in (lambda: tn(s.double(), (x.double(),), ptr, route="hip"), lambda: nn(s.half(), w.half(), ptr, route="hip"),
                 lambda: tn(s, (x[:5],), ptr), lambda: tn(s, (x, x, x, x), ptr), lambda: tn(s, (x,), ptr.int()),
                 lambda: nn(s, w, ptr.int()), lambda: nn(s, w, ptr[:2]), lambda: tn(s.cpu(), (x.cpu(),), ptr.cpu(), route="hip")):
        with pytest.raises(_lib.BackendError):
            call()
