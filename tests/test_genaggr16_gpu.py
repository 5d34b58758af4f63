"""gen_aggregate on fp16 / bf16 GPU tensors (cogdl_hip_gen_aggr16_fwd / _bwd, csrc/genaggr16.hip): fp32 arithmetic, one rounding
where the output and each gradient is stored.  Oracle: the torch composition (tests/_gen_cases.py: a true per-row softmax) in
float64 on the 16-bit inputs upcast.  Rule for out, grad_x and grad_eterm, elementwise:

    |new - oracle| <= 0.5 ulp16(oracle) + 4 err_ref + 8 eps32 max|oracle|

err_ref = max |ref32 - oracle| of the same composition in float32 (CPU, sequential edge order) on the same upcast inputs: the
rule of tests/_gen_cases.py plus the one store rounding (ulp16: tests/_halfprec.py).  grad_beta is fp32 and meets the fp32 rule.

Graph: 24 destinations, 40 sources (num_nodes != x.shape[0]), edges shuffled into a caller's order (the eid path).  Destinations
0 .. 5 have 0 .. 5 edges -- around the forward's unroll of 4 and the softmax backward's of 2 -- and destination 6 has one edge
more than the long-row threshold, so two pieces merge; source 7 sends more than the threshold (the backward's long row);
destinations 20 .. 23 receive nothing, sources 36 .. 39 send nothing.  Widths 1, 7, 8, 9, 64, 72, 136: vector widths 1, 4 and 2
on lane groups of 4 to 64, a ragged last lane group (72), two column tiles (136); tables that start 2, 4 and 8 bytes past a
16-byte boundary take widths 1, 2 and 4 (at 2 bytes: 136 columns in three tiles).  Every call runs with TorchRouteWarning as an
error: before the 16-bit kernels these tensors took the torch route."""
import functools
import warnings

import numpy as np
import pytest
import torch

import _gen_cases as C
import _halfprec as H
from cogdl_amd import _lib
from cogdl_amd.operators import genaggr as GA
from cogdl_amd.operators.ops import TorchRouteWarning

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_DST, N_SRC, LONG = 24, 40, 129
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def graph():
    rng = np.random.default_rng(3)
    row = np.concatenate([np.repeat(np.arange(6), np.arange(6)), np.full(LONG, 6), rng.integers(8, 20, 150)])
    col = rng.integers(0, 36, row.size)
    col[-140:] = 7
    order = rng.permutation(row.size)
    return torch.from_numpy(row[order]).long(), torch.from_numpy(col[order]).long()


@functools.lru_cache(maxsize=None)
def inputs(dtype, width, with_eterm, centre=0.0, spread=2.0):
    """x, eterm | None, G: 16-bit CPU tensors, |x| <= 8 around `centre`; G is signed, as in tests/_gen_cases.py."""
    gen = torch.Generator().manual_seed(100 * width + with_eterm)
    x = (centre + (torch.randn(N_SRC, width, generator=gen) * spread).clamp(-8, 8)).to(dtype)
    eterm = (torch.randn(graph()[0].numel(), width, generator=gen) * 0.25 * spread).to(dtype) if with_eterm else None
    return x, eterm, torch.randn(N_DST, width, generator=gen).to(dtype)


def run(fn, x, eterm, beta, G, device="cpu", dtype=None, offset=0):
    """fn(x, eterm, beta) -> out, then backward(G); beta: None, a float, or a float32 one-element tensor.  Its gradient is taken
    by a second backward with |G|: grad_beta = sum G (q - out^2) is then a sum of non-negative terms, and the fp32 rule's floor,
    which is relative to |oracle|, is relative to the summands too (with a signed G and |x| <= 8 the sum cancels: DESIGN.md).
    dtype: upcast the operands (the references).  offset: the operands start that many bytes into their storage."""
    def place(t):
        t = t.detach().clone().to(device=device, dtype=dtype or t.dtype)
        if offset:
            store = torch.zeros(t.numel() + 8, dtype=t.dtype, device=device)
            view = store[offset // 2:offset // 2 + t.numel()].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == offset
            t = view
        return t

    xa = place(x).requires_grad_()
    ta = None if eterm is None else place(eterm).requires_grad_()
    ba = beta.detach().clone().to(device=device, dtype=dtype or torch.float32).requires_grad_() if torch.is_tensor(beta) else beta
    out = fn(xa, ta, ba)
    out.backward(place(G), retain_graph=torch.is_tensor(beta))
    got = {"out": out.detach(), "g_x": xa.grad}
    if ta is not None:
        got["g_eterm"] = ta.grad
    if torch.is_tensor(beta):
        got["g_beta"] = torch.autograd.grad(out, ba, place(G).abs())[0]
    return {k: v.cpu() for k, v in got.items()}


def check(dtype, width, with_eterm, aggr, beta, offset=0, **kw):
    assert _lib.hip().cogdl_hip_exact_row_edges(graph()[0].numel()) == LONG - 1
    row, col = graph()
    x, eterm, G = inputs(dtype, width, with_eterm, **kw)
    ref = lambda xa, ta, ba: C.composition(xa, row, col, ta, aggr, ba, C.EPS, N_DST)  # noqa: E731
    with C.edge_order():
        oracle = run(ref, x, eterm, beta, G, dtype=torch.float64)
        ref32 = run(ref, x, eterm, beta, G, dtype=torch.float32)
    rd, cd = row.to(DEV), col.to(DEV)
    ours = lambda xa, ta, ba: GA.gen_aggregate(xa, rd, cd, ta, aggr, ba, C.EPS, num_nodes=N_DST)  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("error", TorchRouteWarning)
        got = run(ours, x, eterm, beta, G, device=DEV, offset=offset)
        again = run(ours, x, eterm, beta, G, device=DEV, offset=offset)
    assert got.keys() == oracle.keys()
    for name, want in oracle.items():
        err_ref = float((ref32[name].double() - want).abs().max())
        floor = 4 * err_ref + 8 * C.EPS32 * float(want.abs().max())
        assert got[name].dtype == (torch.float32 if name == "g_beta" else dtype), name
        limit = floor if name == "g_beta" else 0.5 * H.ulp(want.numpy(), dtype) + floor
        print("%s err %.3e  err_ref %.3e" % (name, float((got[name].double() - want).abs().max()), err_ref))
        H.assert_within(got[name].double().numpy(), want.numpy(), limit, name)
        assert torch.equal(got[name].view(torch.uint8), again[name].view(torch.uint8)), name  # no atomics: the same bits
    one = int((row == 1).nonzero()[0])
    m = torch.relu(x[col[one]].float() + (eterm[one].float() if with_eterm else 0)) + C.EPS
    assert torch.equal(got["out"][1], m.to(dtype))  # a one-edge row: its message, rounded once (mean: times 1 / 1)
    assert not got["out"][0].any() and not got["out"][20:].any() and not got["g_x"][36:].any()  # empty rows, idle sources
    return got


WIDTHS = (1, 7, 8, 9, 64, 72, 136)
CASES = [("softmax", True, "learn", w) for w in WIDTHS]
CASES += [("softmax", False, 0.5, 8), ("softmax", False, 0.5, 72), ("softmax", False, None, 64)]
CASES += [("sum", True, None, 9), ("sum", True, None, 136), ("sum", False, None, 64)]
CASES += [("mean", True, None, 7), ("mean", True, None, 72), ("mean", False, None, 8)]


@pytest.mark.parametrize("aggr,with_eterm,beta,width", CASES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_against_the_float64_oracle(dt, aggr, with_eterm, beta, width):
    check(DTYPES[dt], width, with_eterm, aggr, torch.tensor([0.75]) if beta == "learn" else beta)


@pytest.mark.parametrize("offset,width", [(2, 136), (4, 72), (8, 72)])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_tables_that_start_mid_allocation_are_served(dt, offset, width):
    for aggr, beta in (("softmax", torch.tensor([0.75])), ("mean", None)):
        check(DTYPES[dt], width, True, aggr, beta, offset=offset)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_large_logits_carry_the_maximum(dt):
    """beta * m near 3000: exp of it overflows fp32 from 88.7 on, so the row maximum has to be subtracted."""
    got = check(DTYPES[dt], 8, True, "softmax", 100.0, centre=30.0, spread=0.05)
    assert 25 < float(got["out"][6].float().min()) < 35


def test_an_fp16_output_beyond_the_range_is_inf():
    row, col = (t.to(DEV) for t in graph())
    x = torch.full((N_SRC, 8), 600.0, dtype=torch.float16, device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error", TorchRouteWarning)
        out = GA.gen_aggregate(x, row, col, None, "sum", None, C.EPS, num_nodes=N_DST)
    assert out.dtype == torch.float16 and bool(torch.isposinf(out[6]).all())  # 129 x 600 = 77400 > 65504: rounds to inf
    assert bool((out[5] == 3000).all()) and bool(torch.isfinite(out[:6]).all())
