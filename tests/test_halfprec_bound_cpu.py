"""Pins the 16-bit error bound of tests/_halfprec.py itself (no GPU), so that a later loosening is visible.

The kernels' arithmetic -- 16-bit weights and features, fp32 accumulation in CSR order, one store rounding -- is emulated in
numpy, once with a fused multiply-add per edge and once with a rounded multiply followed by a rounded add (the two paths of
SpmmOp::apply, csrc/spmm_op.h).  Stored with round-to-nearest-even every output is inside the bound; stored by TRUNCATION to
bf16 at least a quarter of the outputs are outside it (a condition, not a measurement: the emulation gives 45 %), while none
is outside the bound the suite used before (2^-7 relative), which is therefore blind to a wrong store rounding.

The same for the row softmax (second half of this file): an emulation of csr_edge_softmax's arithmetic against the bounds of
tests/test_halfprec_softmax_gpu.py -- round-to-nearest inside, forward and backward, f16 and bf16; a truncating store outside for
at least a quarter of ALL elements (conditions, not measurements: the emulation gives 38 - 44 % forward, 35 - 40 % backward) and
invisible to the old relative tolerances; exp(v - max) parked in 16 bits before the division outside for at least 10 % (bf16) /
3 % (f16) of them (the emulation: 17 % / 15 %).  And for the exact-equality helper: integer sums are order-independent in fp32,
and round-half-away differs from torch's cast on the ties of the K = 602 product."""
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


# ------------------------------------------------------------------------------------------------------------ row softmax
# The bound tests/test_halfprec_softmax_gpu.py holds csr_edge_softmax to (hp.row_softmax, hp.softmax_terms), pinned on an emulation
# of the kernels' arithmetic in numpy fp32: exp in float32, the row sum over 64 strided lanes (each lane sequential, the lanes
# added in order), 1 / sum, one multiplication; backward: the dot product <s, g> the same way, s * (g - dot).
# The graph: SM_ROWS rows of 0 .. 17 edges (every degree is there), a row of 3,000 edges and a row of 20,000; H = 3; values
# 3 * randn rounded to the dtype.  On the two hub rows the fp32 slack is of the order of half an ulp (of several, in f16), so a wrong
# store rounding CANNOT show there -- they are in the graph so that an honest kernel is seen to stay inside the bound on them --
# and the shares below are shares of ALL elements: the short rows are as many as it takes to carry them.
SM_ROWS, SM_H = 6000, 3
SM_OLD_RTOL = {torch.bfloat16: (2.0 ** -7, 1e-30, 1e-12), torch.float16: (2.0 ** -10, 1e-7, 6e-8)}  # (rtol, atol forward, floor backward)


def _sm_graph():
    rng = np.random.default_rng(20261020)
    deg = rng.integers(0, 18, size=SM_ROWS)
    deg[:18] = np.arange(18)
    deg[100], deg[101] = 3000, 20000
    rowptr = np.zeros(SM_ROWS + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    return rowptr, deg


def _lane_sum(terms):
    """fp32 sum of terms [n, H] over 64 strided lanes: lane l adds the elements l, l + 64, ... in order, then the lanes in order."""
    n, h = terms.shape
    padded = np.zeros(((n + 63) // 64 * 64, h), dtype=np.float32)
    padded[:n] = terms
    lanes = np.cumsum(padded.reshape(-1, 64, h), axis=0, dtype=np.float32)[-1]
    return np.cumsum(lanes, axis=0, dtype=np.float32)[-1]


def _store(x32, dtype, how):
    """fp32 -> dtype -> float64: "nearest" (ties to even) or "truncate" (toward zero)."""
    near = torch.from_numpy(np.ascontiguousarray(x32)).to(dtype)
    if how == "truncate":
        if dtype == torch.bfloat16:
            return (x32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
        n16 = near.numpy()
        over = np.abs(n16.astype(np.float32)) > np.abs(x32)
        return np.where(over, np.nextafter(n16, np.float16(0)), n16).astype(np.float64)
    return near.double().numpy()


def _sm_emulate(rowptr, v, g, dtype, how, parked=False):
    """-> (out, grad_in) as float64 arrays of values of `dtype`; the backward reads the STORED forward output."""
    v32, g32 = v.astype(np.float32), g.astype(np.float32)
    out32 = np.zeros_like(v32)
    for r in range(rowptr.shape[0] - 1):
        sl = slice(rowptr[r], rowptr[r + 1])
        if sl.start == sl.stop:
            continue
        e = np.exp(v32[sl] - v32[sl].max(0))  # float32
        inv = np.float32(1.0) / _lane_sum(e)
        if parked:  # exp(v - max) kept in the 16-bit type between the statistics and the division: a SECOND rounding
            e = _store(e, dtype, "nearest").astype(np.float32)
        out32[sl] = e * inv
    out = _store(out32, dtype, how)
    s32 = out.astype(np.float32)
    gin32 = np.zeros_like(v32)
    for r in range(rowptr.shape[0] - 1):
        sl = slice(rowptr[r], rowptr[r + 1])
        if sl.start == sl.stop:
            continue
        dot = _lane_sum(s32[sl] * g32[sl])
        gin32[sl] = s32[sl] * (g32[sl] - dot)
    return out, _store(gin32, dtype, how)


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def sm_case(request):
    dtype = request.param
    rowptr, deg = _sm_graph()
    gen = torch.Generator().manual_seed(11)
    e = int(rowptr[-1])
    v = (3.0 * torch.randn(e, SM_H, generator=gen)).to(dtype).double().numpy()
    g = torch.randn(e, SM_H, generator=gen).to(dtype).double().numpy()
    want, spread = hp.row_softmax(rowptr, v)
    assert spread.max() <= 40.0 and deg.max() == 20000 and set(range(18)) <= set(deg.tolist())
    terms_f, terms_b = hp.softmax_terms(rowptr, spread)
    return dtype, rowptr, v, g, want, hp.bound(want, want, terms_f, dtype), terms_b


def _sm_judge(case, out, gin):
    """-> (mask of forward elements outside the bound, the same for the backward, the two references and limits)."""
    dtype, rowptr, v, g, want, limit_f, terms_b = case
    _, _, want_g, scale_g = hp.row_softmax(rowptr, v, g, s=out)
    limit_b = hp.bound(want_g, scale_g, terms_b, dtype)
    return hp.outside(out, want, limit_f), hp.outside(gin, want_g, limit_b), (want, limit_f, want_g, limit_b, scale_g)


def test_row_softmax_reference():
    rowptr = np.array([0, 2, 2, 5])
    v = np.array([[0.0, 1.0], [np.log(3.0), 1.0], [5.0, -2.0], [5.0, -2.0], [5.0, 0.0]])
    g = np.arange(10.0).reshape(5, 2)
    want, spread, want_g, scale_g = hp.row_softmax(rowptr, v, g)
    e2 = np.exp(-2.0)
    assert np.allclose(want, [[0.25, 0.5], [0.75, 0.5], [1 / 3, e2 / (2 * e2 + 1)], [1 / 3, e2 / (2 * e2 + 1)], [1 / 3, 1 / (2 * e2 + 1)]])
    assert np.allclose(spread, [[np.log(3.0), 0.0], [0.0, 0.0], [0.0, 2.0]])
    dot0 = 0.25 * 0.0 + 0.75 * 2.0
    assert np.allclose(want_g[:2, 0], [0.25 * (0.0 - dot0), 0.75 * (2.0 - dot0)])
    assert np.allclose(scale_g[:2, 0], [0.25 * (0.0 + dot0), 0.75 * (2.0 + dot0)])
    terms_f, terms_b = hp.softmax_terms(rowptr, spread)
    assert terms_f.shape == (5, 2) and terms_b.shape == (5, 1)
    assert terms_f[0].tolist() == [2 + 2 + 16, 2 + 0 + 16] and terms_f[4].tolist() == [3 + 0 + 16, 3 + 2 + 16] and terms_b[4, 0] == 3 + 16
    # the saved output replaces the exact softmax in the backward
    _, _, wg2, _ = hp.row_softmax(rowptr, v, g, s=np.ones((5, 2)))
    assert np.allclose(wg2[:2, 0], [0.0 - 2.0, 2.0 - 2.0])


def test_softmax_round_to_nearest_store_is_inside(sm_case):
    dtype, rowptr, v, g = sm_case[:4]
    out, gin = _sm_emulate(rowptr, v, g, dtype, "nearest")
    bad_f, bad_b, (want, limit_f, want_g, limit_b, _) = _sm_judge(sm_case, out, gin)
    assert not bad_f.any() and not bad_b.any(), (int(bad_f.sum()), int(bad_b.sum()))
    for got, ref, limit in ((out, want, limit_f), (gin, want_g, limit_b)):
        worst = float((np.abs(got - ref) / limit).max())
        assert worst > 0.9, worst  # ... and tightly


def test_softmax_truncating_store_is_outside_and_the_old_tolerances_do_not_see_it(sm_case):
    dtype, rowptr, v, g = sm_case[:4]
    out, gin = _sm_emulate(rowptr, v, g, dtype, "truncate")
    bad_f, bad_b, (want, _, want_g, _, scale_g) = _sm_judge(sm_case, out, gin)
    assert bad_f.mean() >= 0.25 and bad_b.mean() >= 0.25, (bad_f.mean(), bad_b.mean())
    rtol, atol, floor = SM_OLD_RTOL[dtype]
    assert not hp.outside(out, want, rtol * np.abs(want) + atol).any()
    assert not hp.outside(gin, want_g, rtol * scale_g + floor).any()


def test_softmax_value_rounded_twice_is_outside(sm_case):
    dtype, rowptr, v, g = sm_case[:4]
    out, gin = _sm_emulate(rowptr, v, g, dtype, "nearest", parked=True)
    bad_f, _, _ = _sm_judge(sm_case, out, gin)
    assert bad_f.mean() >= (0.10 if dtype == torch.bfloat16 else 0.03), bad_f.mean()


# ------------------------------------------------------------------------------------------------------------ integer data
def _half_away(x64, dtype):
    """float64 -> the nearest value of dtype with ties AWAY from zero (what the exact-equality tests must catch), as float64."""
    u = hp.ulp(x64, dtype)
    return np.sign(x64) * np.floor(np.abs(x64) / u + 0.5) * u


def test_integer_sums_are_order_independent_and_ties_show_the_rounding_mode():
    """The inputs of the exact-equality tests (tests/test_halfprec_linear_gpu.py, K = 602): integer products accumulated in fp32
    in two different orders give the same bits, and rounding half away from zero differs from torch's cast."""
    gen = torch.Generator().manual_seed(602)
    x = torch.randint(-4, 5, (500, 602), generator=gen).float().numpy()
    w = torch.randint(-4, 5, (602, 64), generator=gen).float().numpy()
    fwd = np.zeros((500, 64), dtype=np.float32)
    for k in range(602):
        fwd += x[:, k:k + 1] * w[k]
    rev = np.zeros((500, 64), dtype=np.float32)
    for k in list(range(301, 602)) + list(range(300, -1, -1)):
        rev += x[:, k:k + 1] * w[k]
    exact = x.astype(np.float64) @ w.astype(np.float64)
    assert fwd.tobytes() == rev.tobytes() and np.array_equal(fwd.astype(np.float64), exact)
    scale = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64)
    for dtype in (torch.bfloat16, torch.float16):
        cast = torch.from_numpy(fwd).to(dtype)
        hp.assert_exact(cast, exact, scale, dtype, "torch's own cast")
    cast = torch.from_numpy(exact).to(torch.bfloat16).double().numpy()
    ties = np.abs(exact - cast) == 0.5 * hp.ulp(exact, torch.bfloat16)
    assert ties.mean() > 0.01, ties.mean()  # sums beyond 256 are odd half the time
    away = _half_away(exact, torch.bfloat16)
    assert (away != cast).any() and np.array_equal(away[~ties], cast[~ties])
    with pytest.raises(AssertionError, match="not the exact sum rounded once"):
        hp.assert_exact(torch.from_numpy(away).to(torch.bfloat16), exact, scale, torch.bfloat16, "half away")
    with pytest.raises(AssertionError, match="not exact in fp32"):
        hp.assert_exact(torch.zeros(2, dtype=torch.bfloat16), np.zeros(2), np.array([1.0, 2.0 ** 24]), torch.bfloat16, "x")
