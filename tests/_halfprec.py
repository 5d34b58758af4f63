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
four units roundoff -- cannot see either."""
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
