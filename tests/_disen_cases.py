"""Shared cases of the disen_route tests (tests/test_disen_cpu.py, tests/test_disen_gpu.py): the graph of tests/_gen_cases.py
(destinations of 0, 1, 2, 63, 64, 65, 128, 129 and 1000 edges, a 400-edge hub source, self-loops, duplicates), the inputs per
(K, d), the float64 oracle and the acceptance rule.

Cases (K, d, tau) and what they reach in csrc/disen.hip:
    (3, 4, 1)      one 16-byte lane per channel, a partial tile (12 of 64 columns)
    (16, 4, 1)     one lane per channel, a full 16-lane group (the model's first layer)
    (8, 8, 0.5)    a 2-lane group per channel
    (5, 2, 1)      10 columns: 8-byte lanes (the row length is no multiple of 4), one lane per channel, a partial tile
    (16, 16, 1)    256 columns: a 4-lane group per channel, the whole wave
    (2, 64, 0.01)  a 16-lane group per channel; scores up to 100
    (6, 2, 1)      added here: 12 columns, two channels in one 16-byte lane

Inputs: c and z normalised per channel, as the layer hands them over, G the upstream gradient; seeded by 100 K + d.  Oracle: the
torch composition (gather, dot, per-row softmax with the row maximum subtracted, scale, scatter_add, add z, normalise) in
float64 on the float32 inputs, gradients from its autograd; ref32 the same composition in float32 under
_gen_cases.edge_order().  Rule, per compared tensor (out, g_c, g_z): _gen_cases.check,

    err_new <= 4 * err_ref + 8 * eps32 * max|oracle|

The normalisation divides by ||a||: `reference` asserts min ||a|| >= 0.05 in float64 for every case, so no case sits next to the
pole (100 K + d gives 0.069 .. 1.0)."""
import functools

import torch

import _gen_cases as G

N = G.N
ISSUE_CASES = ((3, 4, 1.0), (16, 4, 1.0), (8, 8, 0.5), (5, 2, 1.0), (16, 16, 1.0), (2, 64, 0.01))
CASES = ISSUE_CASES + ((6, 2, 1.0),)
MIN_NORM = 0.05
graph = G.graph


def unit(h, K):
    h3 = h.reshape(h.shape[0], K, -1)
    return (h3 / h3.pow(2).sum(-1).sqrt().unsqueeze(-1)).reshape(h.shape)


@functools.lru_cache(maxsize=None)
def inputs(K, d):
    """c, z [N, K d] with unit channels, G [N, K d]."""
    gen = torch.Generator().manual_seed(100 * K + d)
    c = unit(torch.randn(N, K * d, generator=gen), K)
    z = unit(torch.randn(N, K * d, generator=gen), K)
    return c, z, torch.randn(N, K * d, generator=gen)


def softmax_parts(c, z, row, col, K, tau):
    """(zj [E, K, d], s [E, K], p [E, K] the softmax over the edges of each destination)"""
    n = z.shape[0]
    zj = z.reshape(n, K, -1)[col]
    s = (c.reshape(n, K, -1)[row] * zj).sum(-1) / tau
    idx = row.unsqueeze(-1).expand(-1, K)
    top = torch.full((n, K), float("-inf"), dtype=z.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    p = torch.exp(s - top[row])
    return zj, s, p / torch.zeros((n, K), dtype=z.dtype).scatter_add(0, idx, p)[row]


def composition(c, z, row, col, K, tau, with_norm=False):
    n, f = z.shape
    zj, _, p = softmax_parts(c, z, row, col, K, tau)
    msg = (zj * p.unsqueeze(-1)).reshape(row.numel(), f)
    a = (z + torch.zeros_like(z).scatter_add(0, row.unsqueeze(-1).expand(-1, f), msg)).reshape(n, K, -1)
    nrm = a.pow(2).sum(-1).sqrt()
    out = (a / nrm.unsqueeze(-1)).reshape(n, f)
    return (out, nrm) if with_norm else out


def closed_form(c, z, row, col, K, tau, g):
    """(g_c, g_z) by the formulas the kernels implement (cogdl_amd/operators/disen.py), ga and dl from the package's own
    expression."""
    from cogdl_amd.operators.disen import _ga_dl

    n, f = z.shape
    out, nrm = composition(c, z, row, col, K, tau, with_norm=True)
    ga, dl = _ga_dl(g, out, nrm, z, K)
    zj, _, p = softmax_parts(c, z, row, col, K, tau)
    ga3, c3 = ga.reshape(n, K, -1), c.reshape(n, K, -1)
    t = (ga3[row] * zj).sum(-1)
    r = p * (t - dl[row]) / tau
    wide = lambda idx: idx.unsqueeze(-1).expand(-1, f)
    g_c = torch.zeros_like(z).scatter_add(0, wide(row), (r.unsqueeze(-1) * zj).reshape(-1, f))
    per_edge = p.unsqueeze(-1) * ga3[row] + r.unsqueeze(-1) * c3[row]
    g_z = ga + torch.zeros_like(z).scatter_add(0, wide(col), per_edge.reshape(-1, f))
    return g_c, g_z


def run(fn, c, z, Gr, device="cpu", dtype=torch.float32):
    """fn(c, z) -> out; {"out", "g_c", "g_z"} on the CPU."""
    ca = c.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    za = z.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    out = fn(ca, za)
    out.backward(Gr.to(device=device, dtype=dtype))
    return {"out": out.detach().cpu(), "g_c": ca.grad.cpu(), "g_z": za.grad.cpu()}


@functools.lru_cache(maxsize=None)
def reference(K, d, tau):
    """(oracle, ref32): the composition in float64 and in float32 (CPU, deterministic mode) on the same float32 inputs."""
    row, col = graph()
    c, z, Gr = inputs(K, d)
    _, nrm = composition(c.double(), z.double(), row, col, K, tau, with_norm=True)
    assert float(nrm.min()) >= MIN_NORM, (K, d, float(nrm.min()))
    fn = lambda ca, za: composition(ca, za, row, col, K, tau)
    with G.edge_order():
        oracle = run(fn, c, z, Gr, dtype=torch.float64)
        ref32 = run(fn, c, z, Gr)
    return oracle, ref32


check = G.check


def reference_loop(h, row, col, K, iterations, tau):
    """What the layer's loop computes (cogdl/layers/disengcn_layer.py:46-71), restated one channel at a time on [N, d] slices:
    normalise the slice, then per iteration score every edge against the current centres, softmax over the edges of each
    destination, add the weighted sources to the normalised slice and normalise again.  The first iteration's centres are
    the normalised features themselves; the sources stay fixed."""
    n, d = h.shape[0], h.shape[1] // K
    done = []
    for k in range(K):
        feat = h[:, k * d:(k + 1) * d]
        src = feat / feat.pow(2).sum(-1, keepdim=True).sqrt()
        centre = src
        for _ in range(iterations):
            score = (centre[row] * src[col]).sum(-1) / tau
            top = torch.full((n,), float("-inf"), dtype=h.dtype).scatter_reduce(0, row, score.detach(), "amax")
            w = torch.exp(score - top[row])
            w = w / torch.zeros(n, dtype=h.dtype).index_add(0, row, w)[row]
            agg = src + torch.zeros_like(src).index_add(0, row, src[col] * w.unsqueeze(-1))
            centre = agg / agg.pow(2).sum(-1, keepdim=True).sqrt()
        done.append(centre)
    return torch.cat(done, dim=1)
