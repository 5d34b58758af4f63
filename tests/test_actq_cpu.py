"""Activation compression on the host twin (cogdl_host_actq_* / _relu_mask / _mask_apply / _drop_apply through
cogdl_amd/operators/actq.py) against the law of csrc/actq_law.h: the round-trip bound the header derives, exact constant
groups, what the minimum and the maximum dequantise to, zero padding bits, the sizes of codes and metadata, the seeds,
unbiasedness of one call, the packed ReLU, the regenerated dropout and the non-finite cases.  No GPU."""
import math

import pytest
import torch

import _actq_cases as cases
from cogdl_amd import _lib
from cogdl_amd.operators import actq


def _quant(n, bits, group, call=cases.CALL):
    x = cases.tensor(n)
    return x, actq.quantize(x, bits, group, seed=cases.SEED, call=call)


@pytest.mark.parametrize("group", cases.GROUPS)
@pytest.mark.parametrize("bits", cases.BITS)
def test_round_trip_sizes_bound_extremes_and_padding(bits, group):
    L = 2 ** bits - 1
    for n in cases.SIZES:
        x, q = _quant(n, bits, group)
        assert q.codes.dtype == torch.int32 and q.codes.numel() == (n * bits + 31) // 32
        assert q.meta.dtype == torch.float32 and q.meta.numel() == 2 * ((n + group - 1) // group)
        assert (q.bits, q.group, q.numel, q.dtype) == (bits, group, n, torch.float32)
        y = actq.dequantize(q, x.shape)
        gi = cases.group_index(n, group)
        mn, step = q.meta[:, 0], q.meta[:, 1]
        # the header's bound, elementwise
        err = (y.double() - x.double()).abs()
        bound = actq.error_bound(mn, step, bits)[gi]
        assert bool((err <= bound).all()), (n, float((err / bound).max()))
        codes = cases.unpack(q.codes, n, bits)
        assert int(codes.max()) <= L
        for g in range(q.meta.shape[0]):
            sel = gi == g
            xs, ys = x[sel], y[sel]
            assert float(mn[g]) == float(xs.min()) and float(step[g]) == float((xs.max() - xs.min()) / L)
            # the minimum returns mn and the maximum mn + L * step (float32: one product, one sum)
            assert bool((ys[xs == xs.min()] == mn[g]).all())
            assert bool((ys[xs == xs.max()] == mn[g] + torch.tensor(float(L)) * step[g]).all())
            if float(xs.max()) == float(xs.min()):  # a constant group is exact
                assert float(step[g]) == 0.0 and bool((ys == xs).all())
        # padding: the bits of the last word beyond element n are zero
        used = (n * bits) % 32
        if used:
            assert ((int(q.codes[-1]) & 0xFFFFFFFF) >> used) == 0


def test_a_constant_tensor_dequantises_exactly():
    for value in (0.0, -3.25, 1e-30, 7e37):
        x = torch.full((300,), value)
        q = actq.quantize(x, 2, 128, seed=1, call=0)
        assert bool((q.meta[:, 1] == 0).all()) and int(q.codes.abs().max()) == 0
        assert torch.equal(actq.dequantize(q, x.shape), x)


def test_equal_seeds_give_equal_bytes_and_calls_differ():
    x = cases.tensor(1000)
    a = actq.quantize(x, 2, 256, seed=11, call=3)
    b = actq.quantize(x, 2, 256, seed=11, call=3)
    c = actq.quantize(x, 2, 256, seed=11, call=4)
    d = actq.quantize(x, 2, 256, seed=12, call=3)
    assert torch.equal(a.codes, b.codes) and torch.equal(a.meta, b.meta)
    assert not torch.equal(a.codes, c.codes) and not torch.equal(a.codes, d.codes)
    assert torch.equal(a.meta, c.meta)  # the bounds do not depend on the draw


def test_default_seed_follows_torch_initial_seed_and_counts_calls():
    x = cases.tensor(1000)
    torch.manual_seed(123)
    actq.reset_draws()
    first, second = actq.quantize(x), actq.quantize(x)
    assert torch.equal(first.codes, actq.quantize(x, seed=123, call=0).codes)
    assert torch.equal(second.codes, actq.quantize(x, seed=123, call=1).codes)
    torch.manual_seed(124)  # a new seed restarts the counter
    assert torch.equal(actq.quantize(x).codes, actq.quantize(x, seed=124, call=0).codes)


def test_one_call_is_unbiased():
    """[4096, 256] with equal rows, b = 2, G = 256: the column mean of the dequantised rows is within step / 16 of the value.
    A code is the value's position plus a noise in an interval of length 1 (in steps), independent across rows: Hoeffding gives
    P(|mean - value| > step / 16) <= 2 exp(-2 * 4096 / 256) = 2 e^-32 per element, and the draws are fixed by the seed."""
    row = torch.randn(256, generator=torch.Generator().manual_seed(5))
    x = row.repeat(4096, 1)
    q = actq.quantize(x, 2, 256, seed=cases.SEED, call=0)
    assert bool((q.meta == q.meta[0]).all())
    y = actq.dequantize(q, x.shape)
    dev = (y.double().mean(0) - row.double()).abs().max()
    assert float(dev) <= float(q.meta[0, 1]) / 16, (float(dev), float(q.meta[0, 1]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_are_quantised_in_float32_and_come_back_in_their_dtype(dtype):
    x = cases.tensor(1000).to(dtype)
    q = actq.quantize(x, 4, 64, seed=1, call=0)
    ref = actq.quantize(x.float(), 4, 64, seed=1, call=0)
    assert q.dtype == dtype and torch.equal(q.codes, ref.codes) and torch.equal(q.meta, ref.meta)
    y = actq.dequantize(q, x.shape)
    assert y.dtype == dtype and torch.equal(y, actq.dequantize(ref, x.shape).to(dtype))


def test_bad_arguments_are_refused():
    x = cases.tensor(64)
    for bits, group in ((3, 256), (0, 256), (16, 256), (2, 100), (2, 32), (2, 512)):
        with pytest.raises(ValueError):
            actq.quantize(x, bits, group)
    with pytest.raises(_lib.BackendError):
        actq.quantize(x.long())
    with pytest.raises(ValueError):
        actq.dequantize(actq.quantize(x), (63,))
    empty = actq.quantize(x[:0])
    assert empty.codes.numel() == 0 and empty.meta.numel() == 0 and actq.dequantize(empty, (0, 4)).shape == (0, 4)


# ------------------------------------------------------------------------------------------------------------ non-finite
def test_non_finite_groups_follow_the_header():
    """A group with a NaN, an infinity or a range beyond FLT_MAX is stored as (NaN, NaN) with zero codes and dequantises to
    NaN; its neighbours are untouched; no code is above L."""
    for bits in cases.BITS:
        L = 2 ** bits - 1
        x = torch.randn(64 * 6, generator=torch.Generator().manual_seed(9))
        x[5] = float("nan")                     # group 0
        x[64 + 7] = float("inf")                # group 1
        x[128 + 1], x[128 + 2] = 3e38, -3e38    # group 2: finite bounds, the range overflows
        x[192:256] = float("-inf")              # group 3: all equal infinities (mx - mn is a NaN)
        x[256 + 3] = 3e38                       # group 4: large but representable
        q = actq.quantize(x, bits, 64, seed=3, call=0)
        y = actq.dequantize(q, x.shape)
        codes = cases.unpack(q.codes, x.numel(), bits)
        assert int(codes.max()) <= L
        for g in range(4):
            assert bool(torch.isnan(q.meta[g]).all()) and int(codes[64 * g:64 * g + 64].max()) == 0
            assert bool(torch.isnan(y[64 * g:64 * g + 64]).all())
        assert bool(torch.isfinite(q.meta[4:]).all()) and bool(torch.isfinite(y[256:]).all())
        clean = actq.quantize(x[256:].clone(), bits, 64, seed=3, call=0)
        assert torch.equal(clean.meta, q.meta[4:])
        err = (y[256:].double() - x[256:].double()).abs()
        assert bool((err <= actq.error_bound(q.meta[4:, 0], q.meta[4:, 1], bits)[cases.group_index(128, 64)]).all())


def test_a_tiny_range_stays_inside_its_bounds():
    x = torch.tensor([1e-40, 3e-40, 2e-40, 0.0] * 16)  # L / range overflows float32
    for bits in cases.BITS:
        q = actq.quantize(x, bits, 64, seed=3, call=0)
        y = actq.dequantize(q, x.shape)
        assert int(cases.unpack(q.codes, 64, bits).max()) <= 2 ** bits - 1
        assert float((y.double() - x.double()).abs().max()) <= float(actq.error_bound(q.meta[:, 0], q.meta[:, 1], bits)[0])


# ------------------------------------------------------------------------------------------------------------ ReLU mask
@pytest.mark.parametrize("n", cases.SIZES)
def test_relu_packed_is_torch_relu_with_autograd_gradient(n):
    x = cases.tensor(n).clone()
    if n > 2:
        x[1] = float("nan")
    y, mask = actq.relu_mask(x)
    want = torch.relu(x)
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and torch.equal(torch.nan_to_num(y), torch.nan_to_num(want))
    assert mask.dtype == torch.int64 and mask.numel() == (n + 63) // 64
    assert torch.equal(cases.mask_bits(mask, n), x > 0)
    if n % 64:
        assert ((int(mask[-1]) & (2 ** 64 - 1)) >> (n % 64)) == 0
    a = cases.tensor(n).clone().requires_grad_()
    b = cases.tensor(n).clone().requires_grad_()
    g = torch.randn(n, generator=torch.Generator().manual_seed(2))
    actq.relu_packed(a).backward(g)
    torch.relu(b).backward(g)
    assert torch.equal(a.grad, b.grad)


# -------------------------------------------------------------------------------------------------------------- dropout
def test_dropout_regen_identity_zeros_rate_and_backward():
    x = cases.tensor(256 * 64 + 5).clone().requires_grad_()
    assert torch.equal(actq.dropout_regen(x, 0.0), x)
    assert int(actq.dropout_regen(x, 1.0).count_nonzero()) == 0
    assert actq.dropout_regen(x, 0.5, training=False) is x
    # keep rate over 2^20 elements at p = 0.5: sigma = sqrt(0.25 / 2^20) = 0.049 %, the bound is ten of them
    big = torch.ones(2 ** 20)
    kept = actq.dropout_regen(big, 0.5, seed=cases.SEED, call=1)
    assert abs(float((kept != 0).float().mean()) - 0.5) <= 0.005
    assert bool(((kept == 0) | (kept == 2.0)).all())
    # the backward uses the forward's mask and scale
    y = actq.dropout_regen(x, 0.25, seed=cases.SEED, call=2)
    g = torch.randn(x.numel(), generator=torch.Generator().manual_seed(3))
    y.backward(g)
    keep = actq.dropout_regen(torch.ones(x.numel()), 0.25, seed=cases.SEED, call=2) != 0  # (x holds zeros: ask a tensor of ones)
    scale = 65536.0 / (65536 - 16384)
    assert math.isclose(float(keep.float().mean()), 0.75, abs_tol=0.02)
    assert torch.equal(y.detach(), torch.where(keep, x.detach() * scale, torch.zeros(())))
    assert torch.equal(x.grad, torch.where(keep, g * scale, torch.zeros(())))
    # two calls without a seed draw two masks
    torch.manual_seed(77)
    assert not torch.equal(actq.dropout_regen(big, 0.5), actq.dropout_regen(big, 0.5))


# ------------------------------------------------------------------------------------------------------------- linear_q
def test_linear_q_forward_is_exact_and_weight_gradient_is_within_the_bound():
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(200, 48, generator=gen)
    w = torch.randn(24, 48, generator=gen).requires_grad_()
    b = torch.randn(24, generator=gen).requires_grad_()
    xg = x.clone().requires_grad_()
    g = torch.randn(200, 24, generator=gen)
    torch.manual_seed(8)
    actq.reset_draws()
    out = actq.linear_q(xg, w, b, bits=2, group=64)
    assert torch.equal(out, torch.nn.functional.linear(x, w, b))
    out.backward(g)
    q = actq.quantize(x, 2, 64, seed=8, call=0)
    assert torch.equal(w.grad, g.t().mm(actq.dequantize(q, x.shape)))
    assert torch.equal(xg.grad, g.mm(w.detach())) and torch.allclose(b.grad, g.sum(0))
    # |grad_w - exact| [o, i] <= sum_n |g[n, o]| * bound[n, i]
    bound = actq.error_bound(q.meta[:, 0], q.meta[:, 1], 2)[cases.group_index(x.numel(), 64)].view(200, 48)
    exact = g.double().t().mm(x.double())
    # (+ 1e-4: the float32 accumulation of 200 products of magnitude ~1 in grad_w itself)
    assert bool(((w.grad.double() - exact).abs() <= g.double().abs().t().mm(bound) + 1e-4).all())
