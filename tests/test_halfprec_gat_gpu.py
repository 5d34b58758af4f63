"""The fused GAT operator (fused_gat_dropout_func) in f16 / bf16 at its ORDINARY launches, forward and backward, against the
float64 oracle on the rounded inputs with the same dropout mask (oracle.gat_fwd / gat_bwd, as tests/test_gat_dropout.py).

Bounds.  `out` and `grad_feat` are 16-bit, computed in fp32 and stored once:  0.5 * ulp(|want| + s) + s  with
s = 2e-5 * scale (4e-5 on the hub graph) -- the tolerances tests/test_gat_dropout.py holds the SAME kernels to in fp32; 16-bit
adds exactly one store rounding (tests/_halfprec.py).  grad_attn_row / grad_attn_col are fp32 but the backward reads the
rounded forward output: 4 * 2^-7 (bf16) / 4 * 2^-10 (f16) x scale, as tests/test_xcd_gpu.py.

What the shapes reach for 2-byte elements at their own widths (PAD_FEATURES off; gat_fwd_geometry / gat_bwd_geometry,
csrc/gat_op.h; (vec, lanes per row, column tiles)):
    shape      forward        backward
    (8, 8)     (8, 8, 1)      one group (8, 8)
    (1, 41)    (1, 64, 1)     one group (1, 64)
    (3, 5)     (1, 16, 1)     tiled (1, 16, 1)
    (6, 12)    (4, 32, 1)     tiled (4, 64, 1)
    (2, 64)    (8, 16, 1)     one group (8, 16)
    (8, 64)    (8, 64, 1)     one group (8, 64)
    (4, 128)   (8, 64, 1)     one group (8, 64)
    (16, 64)   (8, 64, 2)     tiled (8, 64, 2)
    (3, 24)    (8, 16, 1)     tiled (8, 16, 1)
    (1, 300)   (4, 64, 2)     tiled (4, 64, 2)
    (3, 12)    (4, 16, 1)     tiled (4, 16, 1)
    (3, 6)     (2, 16, 1)     tiled (2, 16, 1)
    (6, 6)     (2, 32, 1)     tiled (2, 64, 1)
    (3, 7)     (1, 32, 1)     tiled (1, 64, 1)
    (4, 4)     (4, 8, 1)      one group (4, 8)
    (16, 2)    (2, 16, 1)     one group (2, 16)
    (32, 1)    (1, 32, 1)     one group (1, 32)
    (4, 64)    (8, 32, 1)     one group (8, 32)
With PAD_FEATURES on (the default) the operator pads F to whole 16-byte lanes first (fused_gat._padded_width): every width is
then a multiple of 8, forward and one-group backward at vec 8, (3, 24) and (16, 64) tiled at vec 8.
So every tiled backward instantiation for 2-byte elements (vec 1, 2, 4, 8 x 16 or 64 lanes) is launched, and every vector
width and every group size of the forward and of the one-group backward at least once.  NOT launched in 16-bit by this file:
forward (1, 8), (2, 8), (2, 64); one-group backward (1, 8), (1, 16), (2, 8), (2, 32), (2, 64), (4, 16), (4, 32), (4, 64)
(as (vec, lanes): these need F = 1, 2 or 4 with up to 64 heads, or one head whose width is no multiple of 8)."""
import functools

import numpy as np
import pytest
import torch

import _halfprec as hp
from cogdl_amd import _lib, synth, xcdplan
from cogdl_amd.operators import fused_gat

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATTN_TOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
SHAPES = [(8, 8), (1, 41), (3, 5), (6, 12), (2, 64), (8, 64), (4, 128), (16, 64), (3, 24), (1, 300),
          (3, 12), (3, 6), (6, 6), (3, 7), (4, 4), (16, 2), (32, 1), (4, 64)]  # (second line: the instantiations the first leaves out)
HUB_SHAPES = [(8, 8), (1, 41), (16, 64), (6, 12), (3, 12), (3, 6)]
HUBS = ((3, 129), (4, 1000), (17, 5000), (18, 257), (40, 128))
S_REL = {"random": 2e-5, "hubs": 4e-5}


@pytest.fixture(autouse=True)
def ordinary_launch(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")  # (the default: these graphs are far below any plan's size)


@pytest.fixture(params=[0, 1, 2], ids=["auto", "edgewise-softmax", "chunkwise-softmax"])
def gat_kernel(request):
    _lib.hip().cogdl_hip_set_tuning(5, request.param)
    yield request.param
    _lib.hip().cogdl_hip_set_tuning(5, 0)


@functools.lru_cache(maxsize=None)
def _graph(kind):
    if kind == "random":
        return synth.random_csr(150, 120, 7, weighted=False)
    return synth.hub_csr(60, 60, hubs=HUBS, weighted=False)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case(kind, h, f, dtype, p):
    """Inputs (rounded to dtype) and the oracle's results for them, computed once and never modified."""
    from oracle import oracle

    g = _graph(kind)
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
    g, seed, a_row, a_col, feat, gout, (want, scale), (gf, gl, gr, sf, sl, sr) = _case(kind, h, f, dtype, p)
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


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("pad", [True, False], ids=["padded-rows", "raw-width"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,f", SHAPES)
def test_fused_gat_16bit_within_half_an_ulp(gat_kernel, dtype, pad, p, h, f):
    check("random", h, f, dtype, p, pad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("pad", [True, False], ids=["padded-rows", "raw-width"])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,f", HUB_SHAPES)
def test_fused_gat_16bit_hub_rows_within_half_an_ulp(gat_kernel, dtype, pad, p, h, f):
    """Rows and columns of thousands of edges: the long-row path of the forward and of both backward passes."""
    check("hubs", h, f, dtype, p, pad)
