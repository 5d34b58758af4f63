"""Pins the 16-bit error bound of tests/_halfprec.py itself (no GPU), so that a later loosening is visible.

The kernels' arithmetic -- 16-bit weights and features, fp32 accumulation in CSR order, one store rounding -- is emulated in
numpy, once with a fused multiply-add per edge and once with a rounded multiply followed by a rounded add (the two paths of
SpmmOp::apply, csrc/spmm_op.h).  Stored with round-to-nearest-even every output is inside the bound; stored by TRUNCATION to
bf16 at least a quarter of the outputs are outside it (a condition, not a measurement: the emulation gives 45 %), while none
is outside the bound the suite used before (2^-7 relative), which is therefore blind to a wrong store rounding."""
import numpy as np
import pytest
import torch

import _halfprec as hp

M, N_COLS, K = 200, 150, 7


def _graph():
    rng = np.random.default_rng(20261019)
    deg = rng.integers(0, 18, size=M)  # 0 .. 17
    deg[:18] = np.arange(18)           # every degree is there
    deg[50], deg[51] = 3000, 1
    rowptr = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    colind = rng.integers(0, N_COLS, size=int(rowptr[-1]))
    return rowptr, colind, deg


def _inputs(dtype):
    gen = torch.Generator().manual_seed(7)
    rowptr, colind, deg = _graph()
    w = torch.randn(int(rowptr[-1]), generator=gen).to(dtype).float().numpy()
    x = torch.randn(N_COLS, K, generator=gen).to(dtype).float().numpy()
    return rowptr, colind, deg, w, x


def _emulate(rowptr, colind, w, x, fma):
    out = np.zeros((M, K), dtype=np.float32)
    for r in range(M):
        sl = slice(rowptr[r], rowptr[r + 1])
        if sl.start == sl.stop:
            continue
        if not fma:  # rounded fp32 products, summed left to right in fp32 (cumsum is sequential)
            out[r] = np.cumsum(w[sl, None] * x[colind[sl]], axis=0, dtype=np.float32)[-1]
            continue
        acc = np.zeros(K, dtype=np.float32)
        for e in range(sl.start, sl.stop):  # the product of two 16-bit numbers is exact in float64: one rounding, of the sum
            acc = (acc.astype(np.float64) + np.float64(w[e]) * x[colind[e]].astype(np.float64)).astype(np.float32)
        out[r] = acc
    return out


def _reference(rowptr, colind, w, x):
    want, scale = np.zeros((M, K)), np.zeros((M, K))
    for r in range(M):
        sl = slice(rowptr[r], rowptr[r + 1])
        terms = w[sl].astype(np.float64)[:, None] * x[colind[sl]].astype(np.float64)
        want[r], scale[r] = terms.sum(0), np.abs(terms).sum(0)
    return want, scale


def test_ulp_values():
    bf, f16 = torch.bfloat16, torch.float16
    assert hp.ulp(1.0, bf) == 2.0 ** -7 and hp.ulp(1.999, bf) == 2.0 ** -7 and hp.ulp(2.0, bf) == 2.0 ** -6
    assert hp.ulp(1.0, f16) == 2.0 ** -10 and hp.ulp(0.75, f16) == 2.0 ** -11
    assert hp.ulp(0.0, f16) == 2.0 ** -24 and hp.ulp(2.0 ** -20, f16) == 2.0 ** -24 and hp.ulp(2.0 ** -14, f16) == 2.0 ** -24
    assert hp.ulp(0.0, bf) == 2.0 ** -133 and hp.ulp(-3.0, bf) == 2.0 ** -6
    # the spacing torch's own types have
    for dt, v in ((bf, 1.0), (bf, 100.0), (f16, 1.0), (f16, 0.01), (f16, 3e-6)):
        t = torch.tensor(v).to(dt)
        nxt = torch.nextafter(t, torch.tensor(float("inf")).to(dt))
        assert float(nxt.double() - t.double()) == float(hp.ulp(float(t), dt)), (dt, v)
    a = np.array([[0.0, 1.0], [3.0, 2.0 ** -30]])
    assert hp.ulp(a, f16).shape == (2, 2) and hp.ulp(a, f16).dtype == np.float64


def test_bound_formula():
    want, scale = np.array([1.0, 0.0, -5.0]), np.array([2.0, 0.0, 8.0])
    s = (2 * 9 + 2) * 2.0 ** -24 * scale
    assert np.array_equal(hp.bound(want, scale, 9, torch.bfloat16), 0.5 * hp.ulp(np.abs(want) + s, torch.bfloat16) + s)
    # a sum just below a binade border gets the next binade's ulp
    b = hp.bound(np.array([2.0 - 1e-9]), np.array([2.0]), 1, torch.float16)
    assert b[0] == 0.5 * 2.0 ** -9 + 4 * 2.0 ** -24 * 2.0
    with pytest.raises(AssertionError, match="worst at flat index 1"):
        hp.assert_close(np.array([1.0, 1.01]), np.array([1.0, 1.0]), np.array([1.0, 1.0]), 1, torch.bfloat16, "x")
    with pytest.raises(AssertionError):  # a NaN where a number is wanted is outside every bound
        hp.assert_close(np.array([np.nan]), np.array([1.0]), np.array([1.0]), 1, torch.bfloat16, "x")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "mul-add"])
def test_round_to_nearest_store_is_inside_and_truncation_is_outside(dtype, fma):
    rowptr, colind, deg, w, x = _inputs(dtype)
    assert deg.min() == 0 and deg.max() == 3000 and set(range(18)) <= set(deg.tolist())
    acc = _emulate(rowptr, colind, w, x, fma)
    want, scale = _reference(rowptr, colind, w, x)
    limit = hp.bound(want, scale, deg[:, None], dtype)
    stored = torch.from_numpy(acc).to(dtype).double().numpy()
    hp.assert_within(stored, want, limit, "round to nearest even")
    worst = float((np.abs(stored - want) / limit).max())
    assert worst > 0.9, worst  # ... and tightly: the bound has no room for a second rounding
    if dtype != torch.bfloat16:
        return
    trunc = (acc.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    out = hp.outside(trunc, want, limit)
    assert out.mean() >= 0.25, out.mean()
    old = 2.0 ** -7 * np.abs(want) + 1e-5 * scale + 1e-6
    assert not hp.outside(trunc, want, old).any()
