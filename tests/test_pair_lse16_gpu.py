"""pair_lse(route="hip") on float16 / bfloat16 operands (csrc/contrast16.hip) against the float64 composition of
tests/_contrast_cases.py on the ROUNDED inputs (rounded to the dtype under test, then upcast: input rounding is not charged to the
kernel).  Derived, not measured, with u = 2^-p (p from tests/_halfprec.py), err_ref the error of the same composition in float32 on
those inputs and eps32 the project's fp32 rule (tests/_contrast_cases.py: check):

    lse             |got - want| <= 0.5 ulp(|want|) + 4 err_ref + 8 eps32 max|want|      exact products, fp32 sums, one store
                    rounding; -inf where the oracle has it
    grad_q, grad_k  |got - want| <= u scale + 0.5 ulp(|want| + u scale) + 4 err_ref + 8 eps32 max|want|     per element; scale =
                    the sum of the element's absolute terms in float64, (|g_i| / tau) SUM_j p_ij |k_jc| and (1 / tau) SUM_i |g_i|
                    p_ij |q_ic|: the ONE rounding of W to the operand type, then the one store rounding.

A truncating conversion of W, an output rounded twice or a W that underflowed fails the rule at the last case (20000 keys: p_ij
~ 5e-5 is below fp16's normal range; the upstream gradient is scaled by 2^-20).  One case per dtype is run twice: equal bits.
grace_loss under autocast: contrast_compat.contrastive_loss on float32 inputs reaches the 16-bit kernels, silently."""
import functools
import types
import warnings

import numpy as np
import pytest
import torch

import _contrast_cases as C
import _halfprec as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SLICED = (40, 2100, 128, "tile_edges", "unit")
TINY_W = (40, 20000, 16, "minus1", "unit", None)  # its G is scaled by 2^-20
CASES = [(1, 1, 1, "zero", "unit", None), (33, 31, 6, "minus1", "unit", None), (70, 150, 24, "arange", "unit", None),
         (70, 150, 24, "last_tile", "unit", None), (64, 96, 130, "arange", "unit", None), (96, 96, 256, "arange", "unit", None),
         SLICED + (None,), SLICED + (1,), SLICED + (5,), (129, 257, 64, "none", "hot", None), TINY_W]
DTYPES = (torch.float16, torch.bfloat16)


@functools.lru_cache(maxsize=None)
def reference(case, dtype):
    """The rounded inputs, G, the float64 oracle, the float32 composition and the float64 `scale` of both gradients."""
    q, k, skip, G = C.inputs(case)
    q, k = q.to(dtype).float(), k.to(dtype).float()
    G = G * 2.0 ** -20 if case == TINY_W else G
    tau = C.tau_of(case)
    fn = lambda qa, ka, sa: C.composition(qa, ka, tau, sa)
    oracle, ref32 = C.run(fn, q, k, skip, G, dtype=torch.float64), C.run(fn, q, k, skip, G)
    s = q.double() @ k.double().t() / tau
    if skip is not None:
        s = s.masked_fill(skip.unsqueeze(1) == torch.arange(k.shape[0]).unsqueeze(0), float("-inf"))
    live = torch.isfinite(oracle["lse"]).unsqueeze(1)
    p = torch.where(live, torch.exp(s - oracle["lse"].masked_fill(~live.squeeze(1), 0.0).unsqueeze(1)), torch.zeros_like(s))
    gp = G.double().abs().unsqueeze(1) * p / tau
    return q, k, skip, G, oracle, ref32, {"g_q": gp @ k.double().abs(), "g_k": gp.t() @ q.double().abs()}


def _run(case, dtype):
    from cogdl_amd.operators.contrast import pair_lse

    q, k, skip, G = reference(case[:5] + (None,), dtype)[:4]
    fn = lambda qa, ka, sa: pair_lse(qa, ka, C.tau_of(case), sa, route="hip", split=case[5])
    return C.run(fn, q, k, skip, G, device=DEV, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: str(t).split(".")[-1])
@pytest.mark.parametrize("case", CASES, ids=C.case_id)
def test_kernels_within_one_rounding_of_w_and_one_of_the_store(case, dtype):
    oracle, ref32, scale = reference(case[:5] + (None,), dtype)[4:]
    u = 2.0 ** -H.DTYPES[dtype][0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = _run(case, dtype)
    for name, want in oracle.items():
        assert got[name].dtype == dtype
        have, want = got[name].double().numpy(), want.numpy()
        finite = np.isfinite(want)
        assert (want[~finite] == -np.inf).all() and (have[~finite] == -np.inf).all(), name
        if not finite.any():
            continue
        fp32 = 4 * float(np.abs(ref32[name].double().numpy() - want)[finite].max()) + 8 * C.EPS32 * float(np.abs(want[finite]).max())
        first = u * scale[name].numpy() if name in scale else np.zeros_like(want)
        limit = first + 0.5 * H.ulp(np.abs(np.where(finite, want, 0.0)) + first, dtype) + fp32
        err = np.abs(have - want)[finite]
        print("%s %s %-4s worst err / bound %.3f" % (C.case_id(case), dtype, name, float((err / limit[finite]).max())))
        H.assert_within(have[finite], want[finite], limit[finite], "%s %s %s" % (C.case_id(case), dtype, name))
    if case == SLICED + (None,):  # no float atomics, every sum in a fixed order
        again = _run(case, dtype)
        for name in got:
            assert torch.equal(got[name], again[name]), name


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: str(t).split(".")[-1])
def test_contrastive_loss_under_autocast_runs_the_16_bit_kernels(dtype):
    from cogdl_amd import contrast_compat
    from cogdl_amd.operators.ops import TorchRouteWarning

    tau = 0.5
    gen = torch.Generator().manual_seed(70)
    z1 = torch.randn(70, 24, generator=gen).to(DEV).requires_grad_()
    z2 = torch.randn(70, 24, generator=gen).to(DEV).requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("error", TorchRouteWarning)
        with torch.autocast("cuda", dtype=dtype):
            loss = contrast_compat.contrastive_loss(types.SimpleNamespace(tau=tau), z1, z2)
        loss.backward()
    assert loss.dtype == torch.float32 and z1.grad.dtype == torch.float32 and z2.grad.dtype == torch.float32
    # the reference formula on the normalised-then-rounded rows (rounded where the call rounds them)
    a, b = (torch.nn.functional.normalize(z.detach(), p=2, dim=-1).to(dtype).cpu() for z in (z1, z2))
    formula = lambda a, b: torch.mean(C.composition(a, torch.cat([a, b]), tau, torch.arange(a.shape[0])) - (a * a).sum(1) / tau)
    want, ref32 = float(formula(a.double(), b.double())), float(formula(a.float(), b.float()))
    bound = 4 * abs(ref32 - want) + 8 * C.EPS32 * abs(want)
    print("loss %.9f want %.9f err %.3e bound %.3e" % (loss.item(), want, abs(loss.item() - want), bound))
    assert abs(loss.item() - want) <= bound
