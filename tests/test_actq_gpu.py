"""Activation compression on the GPU (csrc/actq.hip) against its host twin: both follow csrc/actq_law.h, so codes, metadata,
dequantised values, mask words and dropout outputs are compared byte for byte -- for every case of tests/_actq_cases.py, for an
operand that starts one element into its allocation (the kernels' 4-byte lanes), and from run to run.  Then what the feature is
for: csrspmm(actnn=True) against actnn=False, and the memory a QLinear -> QReLU -> QDropout -> QLinear stack holds between its
forward and its backward pass."""
import pytest
import torch

import _actq_cases as cases
import _offset as O
from cogdl_amd.operators import actq

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _same_quantized(a, b):
    return torch.equal(a.codes.cpu(), b.codes.cpu()) and a.meta.cpu().numpy().tobytes() == b.meta.cpu().numpy().tobytes()


def _same_bytes(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("group", cases.GROUPS)
@pytest.mark.parametrize("bits", cases.BITS)
def test_quantize_and_dequantize_equal_the_host_twin_byte_for_byte(bits, group):
    for n in cases.SIZES:
        x = cases.tensor(n)
        want = actq.quantize(x, bits, group, seed=cases.SEED, call=cases.CALL)
        want_y = actq.dequantize(want, x.shape)
        got = actq.quantize(x.to(DEV), bits, group, seed=cases.SEED, call=cases.CALL)
        assert got.codes.is_cuda and _same_quantized(got, want), (n, bits, group)
        got_y = actq.dequantize(got, x.shape)
        assert _same_bytes(got_y, want_y), (n, bits, group)
        # an operand one element into its allocation: another instantiation, the same bytes, nothing written past the view
        view, _ = O.shifted(x, 1, device=DEV)
        assert view.data_ptr() % 16 == 4 and _same_quantized(actq.quantize(view, bits, group, seed=cases.SEED, call=cases.CALL), want)
        # two runs give equal bytes
        assert _same_quantized(actq.quantize(x.to(DEV), bits, group, seed=cases.SEED, call=cases.CALL), got)


def test_non_finite_groups_equal_the_host_twin():
    x = torch.randn(64 * 6, generator=torch.Generator().manual_seed(9))
    x[5], x[64 + 7], x[128 + 1], x[128 + 2], x[256 + 3] = float("nan"), float("inf"), 3e38, -3e38, 3e38
    x[192:256] = float("-inf")
    x[300:304] = torch.tensor([1e-40, 3e-40, 0.0, -0.0])
    for bits in cases.BITS:
        want = actq.quantize(x, bits, 64, seed=3, call=0)
        got = actq.quantize(x.to(DEV), bits, 64, seed=3, call=0)
        assert _same_quantized(got, want)
        assert _same_bytes(actq.dequantize(got, x.shape), actq.dequantize(want, x.shape))


@pytest.mark.parametrize("n", cases.SIZES)
def test_relu_mask_and_dropout_equal_the_host_twin(n):
    x = cases.tensor(n).clone()
    if n > 2:
        x[1] = float("nan")
    g = torch.randn(n, generator=torch.Generator().manual_seed(2))
    thresh, scale = actq.drop_params(0.3)
    want_y, want_mask = actq.relu_mask(x)
    want_g = actq.mask_apply(g, want_mask)
    want_d = actq.drop_apply(x, cases.SEED, cases.CALL, thresh, scale)
    for shift in (0, 1):
        if shift:
            (xd, _), (gd, _) = O.shifted(x, 1, device=DEV), O.shifted(g, 1, device=DEV)
        else:
            xd, gd = x.to(DEV), g.to(DEV)
        got_y, got_mask = actq.relu_mask(xd)
        assert _same_bytes(got_y, want_y) and torch.equal(got_mask.cpu(), want_mask)
        assert _same_bytes(actq.mask_apply(gd, got_mask), want_g)
        assert _same_bytes(actq.drop_apply(xd, cases.SEED, cases.CALL, thresh, scale), want_d)
    assert _same_bytes(actq.drop_apply(x.to(DEV), cases.SEED, cases.CALL, thresh, scale), want_d)  # two runs


def test_one_call_is_unbiased_on_the_gpu():
    """tests/test_actq_cpu.py's unbiasedness case (Hoeffding: 2 e^-32 per element) on the kernel."""
    row = torch.randn(256, generator=torch.Generator().manual_seed(5))
    x = row.repeat(4096, 1).to(DEV)
    q = actq.quantize(x, 2, 256, seed=cases.SEED, call=0)
    dev = (actq.dequantize(q, x.shape).double().mean(0).cpu() - row.double()).abs().max()
    assert float(dev) <= float(q.meta[0, 1]) / 16


def test_csrspmm_actnn_keeps_out_and_grad_feat_and_bounds_the_edge_gradient():
    from cogdl_amd import actnn_compat, synth
    from cogdl_amd.operators.spmm import csrspmm

    g = synth.scaled(300, 8, seed=3)
    rowptr, colind = g.rowptr.to(DEV), g.colind.to(DEV)
    feat = torch.randn(g.num_nodes, 40, generator=torch.Generator().manual_seed(0)).to(DEV)
    gout = torch.randn(g.num_nodes, 40, generator=torch.Generator().manual_seed(1)).to(DEV)
    res = {}
    for actnn in (False, True):
        x, w = feat.clone().requires_grad_(), g.weight.to(DEV).clone().requires_grad_()
        torch.manual_seed(21)
        actq.reset_draws()
        out = csrspmm(rowptr, colind, x, w, False, actnn=actnn)
        out.backward(gout)
        res[actnn] = (out.detach(), x.grad, w.grad)
    assert _same_bytes(res[True][0], res[False][0]) and _same_bytes(res[True][1], res[False][1])
    # |grad_w - exact| [e] <= sum_f |g[row(e), f]| * step(col[e], f): every dequantised element is within its group's step
    q = actq.quantize(feat, actnn_compat.config.bits, actnn_compat.config.group_size, seed=21, call=0)
    step = q.meta[:, 1].double()[cases.group_index(feat.numel(), q.group).to(DEV)].view_as(feat)
    row = torch.repeat_interleave(torch.arange(g.num_nodes, device=DEV), (rowptr[1:] - rowptr[:-1]).long())
    limit = (gout.double().abs()[row] * step[colind.long()]).sum(1)
    diff = (res[True][2].double() - res[False][2].double()).abs()
    assert bool((diff <= limit).all()), float((diff / limit).max())
    assert float(diff.max()) > 0  # the quantised operand was really used
    # nothing to save: exactly SPMMFunction
    x = feat.clone().requires_grad_()
    out = csrspmm(rowptr, colind, x, g.weight.to(DEV), False, actnn=True)
    assert _same_bytes(out.detach(), res[False][0]) and type(out.grad_fn).__name__.startswith("SPMMFunction")


def test_int64_rowptr_with_actnn_keeps_raising():
    from cogdl_amd import _lib
    from cogdl_amd.operators.spmm import csrspmm

    rowptr = torch.tensor([0, 1, 2], dtype=torch.int64, device=DEV)
    colind = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.BackendError, match="64-bit"):
        csrspmm(rowptr, colind, torch.ones(2, 4, device=DEV), torch.ones(2, device=DEV), False, actnn=True)


def _held_after_forward(stack, x):
    """Bytes the autograd graph of stack(x) holds: allocated after the forward, minus before, minus the output's own."""
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = stack(x)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before - out.numel() * out.element_size()
    out.sum().backward()
    return held


def test_a_compressed_stack_holds_an_eighth_of_what_the_nn_stack_holds():
    """QLinear(256, 256) -> QReLU -> QDropout(0.5) -> QLinear(256, 256) at N = 65536.  In units of 4 N F bytes the nn stack
    holds the first product, the ReLU output, a bool mask (1/4) and the dropout output: 3.25; the compressed stack holds two
    2-bit copies (1/16 each, plus 8 bytes per 256 elements) and a 1-bit mask (1/32): 0.17, a ratio of 0.053.  The cap of 1/8
    leaves room for the allocator's rounding.  Measured on the MI355X: 3.44 against 0.172 units."""
    from cogdl_amd import actnn_compat as A

    n, f = 65536, 256
    x = torch.randn(n, f, device=DEV)
    plain = torch.nn.Sequential(torch.nn.Linear(f, f), torch.nn.ReLU(), torch.nn.Dropout(0.5), torch.nn.Linear(f, f)).to(DEV)
    packed = torch.nn.Sequential(A.QLinear(f, f), A.QReLU(), A.QDropout(0.5), A.QLinear(f, f)).to(DEV)
    assert A.config.bits == 2 and A.config.compress_activation
    held_plain = _held_after_forward(plain, x)
    held_packed = _held_after_forward(packed, x)
    print("held after forward: nn %.2f, compressed %.3f units of 4 N F bytes" % (held_plain / (4 * n * f), held_packed / (4 * n * f)))
    assert held_plain > 0 and held_packed <= held_plain / 8, (held_packed, held_plain)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in packed.parameters())
