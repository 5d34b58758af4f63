"""Seeded inputs and the float64 references (a plain loop over the segments) shared by tests/test_segmm_gpu.py and
tests/test_diffpool_install_cpu.py.  A tn case is (lens, K, widths, with_s, split): s [N, K], one panel [N, F] per width and,
with_s, s itself as the last panel; an nn case is (lens, P, Q, accumulate): x [N, P], w [B, P, Q] and a base [N, Q] the product
is added to.  `lens` names the segment lengths.  The gradients compared are those of SUM_p <out_p, G_p> for fixed random G_p."""
import functools
import zlib

import torch

LENS = {"ragged": (1, 31, 32, 33, 65, 0, 130, 0),  # tile edges of 16, 32 and 64 rows; an empty segment inside and at the end
        "front": (0, 70, 3),                       # an empty segment at the start
        "one": (130,)}                             # B = 1


def ptr_of(lens):
    return torch.tensor((0,) + LENS[lens]).cumsum(0)


@functools.lru_cache(maxsize=None)
def tn_inputs(lens, k, widths, with_s):
    """-> s, the panels, the upstream gradients"""
    gen = torch.Generator().manual_seed(zlib.crc32(repr((lens, k, widths, with_s)).encode()))
    n, b = sum(LENS[lens]), len(LENS[lens])
    return (torch.randn(n, k, generator=gen), [torch.randn(n, f, generator=gen) for f in widths],
            [torch.randn(b, k, f, generator=gen) for f in widths + ((k,) if with_s else ())])


@functools.lru_cache(maxsize=None)
def nn_inputs(lens, p, q):
    """-> x, w, the upstream gradient, the base of accumulate"""
    gen = torch.Generator().manual_seed(zlib.crc32(repr((lens, p, q)).encode()))
    n, b = sum(LENS[lens]), len(LENS[lens])
    return (torch.randn(n, p, generator=gen), torch.randn(b, p, q, generator=gen), torch.randn(n, q, generator=gen),
            torch.randn(n, q, generator=gen))


def run_tn(fn, case, dtype=torch.float32, device="cpu", shift=None):
    """fn(s, panels, ptr) -> outs; -> {name: CPU tensor} of the outputs and the gradients of s and every panel.  shift: a
    function that moves an operand inside its allocation (tests/_offset.py), applied to s and the first panel."""
    s, panels, grads = tn_inputs(*case[:4])
    move = lambda t, i: (shift(t.to(dtype)) if shift is not None and i < 2 else t.to(dtype).to(device).clone()).requires_grad_()
    s, panels = move(s, 0), [move(p, i + 1) for i, p in enumerate(panels)]
    outs = fn(s, tuple(panels) + ((s,) if case[3] else ()), ptr_of(case[0]).to(device))
    sum((o * g.to(dtype).to(device)).sum() for o, g in zip(outs, grads)).backward()
    got = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    got.update({"grad_s": s.grad}, **{"grad_x%d" % i: p.grad for i, p in enumerate(panels)})
    return {name: t.cpu() for name, t in got.items()}


def run_nn(fn, case, dtype=torch.float32, device="cpu"):
    x, w, g, _ = nn_inputs(*case[:3])
    x, w = (t.to(dtype).to(device).clone().requires_grad_() for t in (x, w))
    out = fn(x, w, ptr_of(case[0]).to(device))
    (out * g.to(dtype).to(device)).sum().backward()
    return {"out": out.detach().cpu(), "grad_x": x.grad.cpu(), "grad_w": w.grad.cpu()}


def loop_tn(s, panels, ptr):
    return tuple(torch.stack([s[a:b].t() @ x[a:b] for a, b in zip(ptr[:-1].tolist(), ptr[1:].tolist())]) for x in panels)


def loop_nn(x, w, ptr):
    return torch.cat([x[a:b] @ w[g] for g, (a, b) in enumerate(zip(ptr[:-1].tolist(), ptr[1:].tolist()))])


reference_tn = functools.lru_cache(maxsize=None)(lambda case: run_tn(loop_tn, case, torch.float64))
reference_nn = functools.lru_cache(maxsize=None)(lambda case: run_nn(loop_nn, case, torch.float64))


def errors(got, want):
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    return {k: float((got[k].double() - want[k]).abs().max() / want[k].abs().max().clamp_min(1e-300)) for k in want}
