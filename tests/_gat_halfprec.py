"""Cases, references and bounds of the 16-bit fused GAT tests (tests/test_halfprec_gat_gpu.py: the ordinary launches;
tests/test_halfprec_plan_gpu.py: the same operator over XCD plans): inputs rounded to the dtype, the float64 oracle's results for
them with the same dropout mask, computed once per case and never modified.

Bounds.  `out` and `grad_feat` are 16-bit, computed in fp32 and stored once:  0.5 * ulp(|want| + s) + s  with s = S_REL x scale --
2e-5 (4e-5 on graphs with hub rows), the tolerances tests/test_gat_dropout.py holds the SAME kernels to in fp32; 16-bit adds exactly
one store rounding (tests/_halfprec.py).  grad_attn_row / grad_attn_col are fp32 but the backward reads the rounded forward output:
4 * 2^-7 (bf16) / 4 * 2^-10 (f16) x scale, as tests/test_xcd_gpu.py."""
import functools

import numpy as np
import torch

import _halfprec as hp
from cogdl_amd import synth
from cogdl_amd.operators import fused_gat

DEV = "cuda:0"
ATTN_TOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
HUBS = ((3, 129), (4, 1000), (17, 5000), (18, 257), (40, 128))
S_REL = {"random": 2e-5, "hubs": 4e-5}
# kind -> builder of a square, unweighted CSR graph; register() adds the graphs of other files
GRAPHS = {"random": lambda: synth.random_csr(150, 120, 7, weighted=False),
          "hubs": lambda: synth.hub_csr(60, 60, hubs=HUBS, weighted=False)}


def register(kind, builder, s_rel):
    """Another graph for graph() / case() / check(): `builder()` -> CSRGraph; s_rel: S_REL of a graph of its nature."""
    GRAPHS.setdefault(kind, builder)
    S_REL.setdefault(kind, s_rel)


@functools.lru_cache(maxsize=None)
def graph(kind):
    return GRAPHS[kind]()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(kind, h, f, dtype, p):
    """Inputs (rounded to dtype) and the oracle's results for them, computed once and never modified."""
    from oracle import oracle

    g = graph(kind)
    v, n_src = g.num_nodes, g.n_cols
    seed = 1000 + 7 * h + f
    gen = torch.Generator().manual_seed(seed)
    a_row, a_col = torch.randn(v, h, generator=gen), torch.randn(n_src, h, generator=gen)
    feat = torch.randn(n_src, h, f, generator=gen).to(dtype)
    gout = torch.randn(v, h, f, generator=gen).to(dtype)
    drop = oracle.edge_dropout_mask(g.nnz, h, p, seed) if p > 0 else None
    fh, gh = feat.float(), gout.float()
    want = oracle.gat_fwd(g.rowptr, g.colind, a_row, a_col, fh, 0.2, drop=drop)
    scale = oracle.gat_fwd(g.rowptr, g.colind, a_row, a_col, fh.abs(), 0.2, drop=drop)
    grads = oracle.gat_bwd(g.rowptr, g.colind, a_row, a_col, fh, 0.2, gh, n_src=n_src, scales=True, drop=drop)
    return g, seed, a_row, a_col, feat, gout, _frozen(want, scale), _frozen(*grads)


def run(kind, h, f, dtype, p, pad):
    """One forward + backward of the operator -> {name: (got, want, scale)} as float64 arrays."""
    g, seed, a_row, a_col, feat, gout, (want, scale), (gf, gl, gr, sf, sl, sr) = case(kind, h, f, dtype, p)
    saved = fused_gat.PAD_FEATURES
    fused_gat.PAD_FEATURES = pad
    try:
        ar, ac, ft = (t.to(DEV).requires_grad_() for t in (a_row, a_col, feat))
        out = fused_gat.fused_gat_dropout_func(ar, ac, g.rowptr.to(DEV), g.colind.to(DEV), 0.2, ft, p, seed)
        out.backward(gout.to(DEV))
    finally:
        fused_gat.PAD_FEATURES = saved
    assert out.dtype == dtype and ft.grad.dtype == dtype and ar.grad.dtype == torch.float32 and ac.grad.dtype == torch.float32
    assert out.shape == want.shape and ft.grad.shape == gf.shape
    as64 = lambda t: t.detach().float().cpu().numpy().astype(np.float64)  # noqa: E731
    return {"out": (as64(out), want, scale), "grad_feat": (as64(ft.grad), gf, sf),
            "grad_attn_row": (as64(ar.grad), gl, sl), "grad_attn_col": (as64(ac.grad), gr, sr)}


def check(kind, h, f, dtype, p, pad):
    res = run(kind, h, f, dtype, p, pad)
    what = "%s (%d, %d) p=%s pad=%s " % (kind, h, f, p, pad)
    for name in ("out", "grad_feat"):
        got, want, scale = res[name]
        s = S_REL[kind] * np.asarray(scale, dtype=np.float64)
        hp.assert_within(got, want, 0.5 * hp.ulp(np.abs(want) + s, dtype) + s, what + name)
    for name in ("grad_attn_row", "grad_attn_col"):
        got, want, scale = res[name]
        hp.assert_within(got, want, 4 * ATTN_TOL[dtype] * np.asarray(scale, dtype=np.float64) + 1e-30, what + name)
