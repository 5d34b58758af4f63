"""The error bound of a 16-bit result that was computed in fp32 and rounded ONCE, to nearest, on store (the promise of
include/cogdl_hip.h for f16 / bf16 csr_spmm, mhspmm and the fused GAT operator).  Nothing here is measured:

    slack = (2 * terms + 2) * 2^-24 * scale      fp32 summation of `terms` products in ANY order: at most two roundings per
                                                 term (multiply, add; one with an fma), each at most 2^-24 relative to a
                                                 partial sum that `scale` (the same sum over absolute values) bounds -- the
                                                 standard bound, first order, with a margin of two terms.  It therefore covers
                                                 the re-associated pieces of the long-row path and both arithmetic paths of
                                                 SpmmOp::apply.
    bound = 0.5 * ulp(|want| + slack) + slack    one round-to-nearest store of the fp32 sum; the ulp is taken at
                                                 |want| + slack so that a sum that crossed into the next binade is covered.

`want` is the float64 result on the ROUNDED inputs.  A store that truncates, or a value rounded twice, is outside this bound
for a large share of the outputs (tests/test_halfprec_bound_cpu.py pins that), while the old 2^-7 / 2^-10 relative bounds --
four units roundoff -- cannot see either.

Two more tools for the same promise:  assert_exact  -- with integer data every fp32 partial sum is exact, the slack is zero and
the result has to be the float64 result cast once, ties to even --  and  row_softmax / softmax_terms  -- the float64 reference
of csr_edge_softmax and the `terms` its bound takes (derived in tests/test_halfprec_softmax_gpu.py)."""
import numpy as np
import torch

# dtype -> (p = significand bits with the hidden one, emin = exponent of the smallest normal number)
DTYPES = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}


def ulp(a, dtype):
    """Spacing of `dtype` at magnitude a (elementwise, float64): 2^(max(floor(log2 a), emin) - (p - 1)); a = 0 and the
    subnormal range use emin."""
    p, emin = DTYPES[dtype]
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.full(a.shape, float(emin))
    pos = a > 0
    e[pos] = np.maximum(np.floor(np.log2(a[pos])), emin)
    return np.exp2(e - (p - 1))


def slack(scale, terms):
    return (2.0 * np.asarray(terms, dtype=np.float64) + 2.0) * 2.0 ** -24 * np.asarray(scale, dtype=np.float64)


def bound(want, scale, terms, dtype):
    """want, scale: float64 arrays of one shape; terms: the number of summands of every output element (a scalar or an array
    that broadcasts against `want`: the row's degree as [m, 1], or k for a dot product)."""
    s = slack(scale, terms)
    return 0.5 * ulp(np.abs(np.asarray(want, dtype=np.float64)) + s, dtype) + s


def outside(got, want, limit):
    """Boolean mask of the elements whose error exceeds `limit` (a non-finite `got` where `want` is finite counts)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    return ~(err <= limit)


def assert_within(got, want, limit, what):
    """Every element of `got` within `limit` of `want`; reports the worst one."""
    got, want, limit = (np.asarray(a, dtype=np.float64) for a in (got, want, limit))
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    limit = np.broadcast_to(limit, want.shape)
    bad = outside(got, want, limit)
    if bad.any():
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bad, np.nan_to_num(np.abs(got - want) / limit, nan=np.inf, posinf=np.inf), 0.0)
        worst = int(np.argmax(ratio))
        raise AssertionError("%s: %d of %d elements outside the bound; worst at flat index %d: got %.9e, want %.9e, err %.3e > "
                             "bound %.3e" % (what, int(bad.sum()), bad.size, worst, got.flat[worst], want.flat[worst],
                                             abs(got.flat[worst] - want.flat[worst]), limit.flat[worst]))


def assert_close(got, want, scale, terms, dtype, what):
    """got: the 16-bit result (a tensor or an array, any device); every element within bound(want, scale, terms, dtype)."""
    if torch.is_tensor(got):
        got = got.detach().float().cpu().numpy()
    assert_within(got, want, bound(want, scale, terms, dtype), what)


def assert_exact(got, want64, scale, dtype, what):
    """Exact arithmetic: the inputs are small integers (or multiples of a power of two), so every product and every fp32 partial
    sum -- in ANY order -- is exact as long as the sum of the absolute terms `scale` stays below 2^24 (asserted here).  The only
    rounding left is the store's, there is no slack, and ties occur (257 in bf16 is one): `got` (a tensor of `dtype`) has to
    be the float64 result cast ONCE by torch (round to nearest, ties to even; beyond the range: inf), bit for bit -- only the sign
    of a zero is left open (a sum of exact terms that cancel is +0 or -0 by the order they were added in)."""
    scale = np.asarray(scale, dtype=np.float64)
    assert scale.shape == np.shape(want64) and bool((scale < 2.0 ** 24).all()), "%s: the sums are not exact in fp32" % what
    want = torch.from_numpy(np.ascontiguousarray(want64, dtype=np.float64)).to(dtype)
    got = got.detach().cpu()
    assert got.dtype == dtype and got.shape == want.shape, "%s: %s %s, expected %s %s" % (what, got.dtype, tuple(got.shape), dtype,
                                                                                          tuple(want.shape))
    gb, wb = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    bad = (gb != wb) & ~((got == 0) & (want == 0))
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError("%s: %d of %d elements are not the exact sum rounded once; first at flat index %d: got %r, exact %r "
                             "-> %r" % (what, int(bad.sum()), bad.numel(), i, float(got.flatten()[i]),
                                        float(np.asarray(want64).flat[i]), float(want.flatten()[i])))


def row_softmax(rowptr, v, g=None, s=None):
    """Float64 softmax over the rows of a CSR structure, per head: rowptr [m + 1], v [E, H] (empty rows are fine).
    -> (want [E, H], A [m, H]) with A = max over the row of |v - max_row| (0 for an empty row); with an upstream gradient g [E, H]
    also the backward  want_g = s * (g - sum_row s * g)  and the sum of its absolute terms  scale_g = s * (|g| + sum_row |s * g|),
    both [E, H], for s = `s` if given (the forward output a kernel SAVED, so that the two passes are judged separately), else
    `want`.  v = None (with g and s): the backward alone -> (None, None, want_g, scale_g)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    m = rowptr.shape[0] - 1
    row = np.repeat(np.arange(m), np.diff(rowptr))
    if v is None:  # the backward alone, from a saved output
        g, s = np.asarray(g, dtype=np.float64), np.asarray(s, dtype=np.float64)
        dot, dot_abs = np.zeros((m, s.shape[1])), np.zeros((m, s.shape[1]))
        np.add.at(dot, row, s * g)
        np.add.at(dot_abs, row, np.abs(s * g))
        return None, None, s * (g - dot[row]), np.abs(s) * (np.abs(g) + dot_abs[row])
    v = np.asarray(v, dtype=np.float64)
    h = v.shape[1]
    mx = np.full((m, h), -np.inf)
    np.maximum.at(mx, row, v)
    d = v - mx[row]
    e = np.exp(d)
    tot = np.zeros((m, h))
    np.add.at(tot, row, e)
    want = e / tot[row]
    spread = np.zeros((m, h))
    np.maximum.at(spread, row, np.abs(d))
    if g is None:
        return want, spread
    g = np.asarray(g, dtype=np.float64)
    s = want if s is None else np.asarray(s, dtype=np.float64)
    dot, dot_abs = np.zeros((m, h)), np.zeros((m, h))
    np.add.at(dot, row, s * g)
    np.add.at(dot_abs, row, np.abs(s * g))
    return want, spread, s * (g - dot[row]), np.abs(s) * (np.abs(g) + dot_abs[row])


SOFTMAX_MARGIN = 16  # terms beyond the row's additions: the division, the difference v - max, the merge of piece records


def softmax_terms(rowptr, spread):
    """`terms` of bound() for every element of a row softmax (tests/test_halfprec_softmax_gpu.py derives them):
    forward  deg + ceil(A) + 16 per (row, head) -> [E, H];  backward  deg + 16 -> [E, 1]."""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    row = np.repeat(np.arange(deg.shape[0]), deg)
    return (deg[:, None] + np.ceil(spread) + SOFTMAX_MARGIN)[row], (deg + SOFTMAX_MARGIN)[row][:, None]
