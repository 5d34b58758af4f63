"""The value gradients of spgemm against the closed forms of csrc/spgemm.hip evaluated in float64
(tests/_spgemm_cases.py: grad_ref, itself checked against float64 autograd of torch.sparse.mm on the CPU):

  gA[(i,k)] = sum_j G[i,j] B[k,j]        gB[(k,j)] = sum_i A[i,k] G[i,j]

Rules: on integer-valued A, B and G (values in {-4 .. 4}: every partial sum is an integer below 2^24) the gradients are
EQUAL; on random data |g - g64| <= gamma_(t+1) * sum |terms| per entry, t = the entry's number of terms, u = 2^-24 -- the
classical bound of t products and t - 1 additions in any order, fused or not.  An entry without terms must be exactly 0.

Reached here and not in tests/test_spgemm_gpu.py: rows of B and columns of A of 0, 1, 15, 16, 17, 33 (and 100) entries
around the 16-lane group; leading and trailing empty rows under row_of; duplicates and unsorted columns in A and B (every
duplicate receives its own gradient); a cancelled entry of C with an upstream gradient; one operand requiring a gradient;
more than 65,536 x 16 gradient entries for each of the two kernels (their grid stride); products without any entry.
"""
import numpy as np
import pytest
import torch

import _spgemm_cases as C
from cogdl_amd import torch_sparse_compat
from cogdl_amd.operators.spgemm import coalesce, spgemm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _backward(A, B, n, G, need=(True, True)):
    """-> (gA, gB) as numpy (None where not required) for the upstream gradient G (numpy float32, one per entry of C)."""
    (rA, cA, vA), (rB, cB, vB) = C.to_device(A, DEV), C.to_device(B, DEV)
    vA.requires_grad_(need[0])
    vB.requires_grad_(need[1])
    rC, cC, vC = spgemm(rA, cA, vA, rB, cB, vB, n)
    assert vC.numel() == len(G)
    (vC * torch.from_numpy(np.asarray(G, dtype=np.float32)).to(DEV)).sum().backward()
    return tuple(None if v.grad is None else v.grad.cpu().numpy() for v in (vA, vB))


def _within(got, want, bound, terms, what):
    err = np.abs(got.astype(np.float64) - want)
    lim = C.gamma(terms + 1) * bound
    assert (err <= lim).all(), "%s: %d entries beyond gamma_(t+1) sum|terms|, worst excess %.3g" % (
        what, int((err > lim).sum()), float((err - lim).max()))
    assert not got[terms == 0].any(), what


def _check(A, B, n, seed=0, need=(True, True), force=None):
    """Random data under the bound, then the same pattern in integers, exactly.  force: entries of C whose upstream gradient is
    set to 3 (never 0)."""
    rng = np.random.default_rng(seed + 100)
    nnz = len(C.ref32(A, B, n)[1])
    for X, Y, G in ((A, B, rng.standard_normal(nnz).astype(np.float32)),
                    (C.ints(A, seed + 1), C.ints(B, seed + 2), rng.integers(-4, 5, nnz).astype(np.float32))):
        if force is not None:
            G[force] = 3.0
        gA, gB, bA, bB, tA, tB = C.grad_ref(X, Y, n, G)
        got = _backward(X, Y, n, G, need)
        for g, want, bound, terms, what, needed in ((got[0], gA, bA, tA, "gA", need[0]), (got[1], gB, bB, tB, "gB", need[1])):
            if not needed:
                assert g is None
            elif X is A:
                _within(g, want, bound, terms, what)
            else:
                assert np.array_equal(g.astype(np.float64), want), what + " (integer data)"


def _coo_case(m, k, n, e, seed):
    g = torch.Generator().manual_seed(seed)
    ia = torch.stack([torch.randint(0, m, (e,), generator=g), torch.randint(0, k, (e,), generator=g)])
    ib = torch.stack([torch.randint(0, k, (e,), generator=g), torch.randint(0, n, (e,), generator=g)])
    return ia.numpy(), torch.randn(e, generator=g).numpy(), ib.numpy(), torch.randn(e, generator=g).numpy()


@pytest.mark.parametrize("m,k,n,e,seed", [(30, 40, 50, 300, 0), (120, 80, 60, 2000, 1), (8, 300, 9, 1500, 2)])
def test_gradients_through_coalesce(m, k, n, e, seed):
    """COO with duplicates -> coalesce -> spgemm, gradients into the ORIGINAL value vectors: the canonical entry's gradient
    for every duplicate.  The reference works on the float32 canonical values that coalesce returns (exact: see
    test_spgemm_exact_gpu), so the bound covers the product alone."""
    ia, va, ib, vb = _coo_case(m, k, n, e, seed)
    for integer in (False, True):
        if integer:
            rng = np.random.default_rng(seed)
            va, vb = rng.integers(-2, 3, e).astype(np.float32), rng.integers(-2, 3, e).astype(np.float32)
        ra, ca, xa, mapa = C.coalesce_ref(ia[0], ia[1], va, m, k)
        rb, cb, xb, mapb = C.coalesce_ref(ib[0], ib[1], vb, k, n)
        nnz = len(C.ref32((ra, ca, xa), (rb, cb, xb), n)[1])
        G = np.random.default_rng(seed + 7).integers(-4, 5, nnz).astype(np.float32) if integer else \
            np.random.default_rng(seed + 7).standard_normal(nnz).astype(np.float32)
        gA, gB, bA, bB, tA, tB = C.grad_ref((ra, ca, xa), (rb, cb, xb), n, G)
        a, b = torch.from_numpy(va).to(DEV).requires_grad_(), torch.from_numpy(vb).to(DEV).requires_grad_()
        rA, cA, vA = coalesce(torch.from_numpy(ia[0]).to(DEV), torch.from_numpy(ia[1]).to(DEV), a, m, k)
        rB, cB, vB = coalesce(torch.from_numpy(ib[0]).to(DEV), torch.from_numpy(ib[1]).to(DEV), b, k, n)
        vC = spgemm(rA, cA, vA, rB, cB, vB, n)[2]
        assert vC.numel() == nnz
        (vC * torch.from_numpy(G).to(DEV)).sum().backward()
        for got, want, bound, terms, mp in ((a.grad, gA, bA, tA, mapa), (b.grad, gB, bB, tB, mapb)):
            got = got.cpu().numpy()
            if integer:
                assert np.array_equal(got.astype(np.float64), want[mp])
            else:
                _within(got, want[mp], bound[mp], terms[mp], "through coalesce")


def test_gradient_through_the_global_path():
    a = C._random(20, 300, 0.1, 12)
    a[3] = torch.randn(300, generator=torch.Generator().manual_seed(3))
    A, B = C.csr_of_dense(a.numpy()), C.csr_of_dense(C._random(300, 400, 0.5, 13).numpy())
    assert C.bin_of(C.ub(A, B))[3] == 3
    _check(A, B, 400)


def test_group_tails():
    """Rows of B with 0, 1, 15, 16, 17, 33, 100 entries (gA) and columns of A with 0, 1, 15, 16, 17, 33 (gB)."""
    A, B, n = C.group_tail_case()
    assert set(np.diff(B[0])) == set(C.GROUP_LENGTHS_B) and set(np.bincount(A[1], minlength=42)) == set(C.GROUP_LENGTHS_A)
    _check(A, B, n)


def test_leading_and_trailing_empty_rows():
    A, B, n = C.empty_ends_case()
    for X in (A, B):
        assert np.diff(X[0])[:3].sum() == 0 and np.diff(X[0])[-3:].sum() == 0
    _check(A, B, n)


@pytest.mark.parametrize("which", ["A", "B", "AB"])
def test_noncanonical_operands(which):
    """Every duplicate entry receives its own gradient (the closed form is per entry, not per cell)."""
    A, B, n = C.noncanonical_case(which)
    assert list(C.bin_of(C.ub(A, B))) == [0, 1, -1, 2, 3]
    _check(A, B, n, seed=3)


def test_cancelled_entry_passes_its_gradient_on():
    """C[i, n-1] = x y - x y = 0 is an entry: with G = 3 there, y and the x of A receive 3 y and 3 x as anywhere else."""
    A, B, n = C.zero_case()
    rowptr, col, _ = C.ref32(A, B, n)
    assert (col[rowptr[1:] - 1] == n - 1).all()
    _check(A, B, n, seed=4, force=rowptr[1:] - 1)


@pytest.mark.parametrize("need", [(True, False), (False, True)])
def test_one_operand_requires_grad(need):
    A, B, n = C.rectangular(*C.RECTANGULAR[1])
    _check(A, B, n, seed=5, need=need)


def test_grad_a_beyond_one_launch_of_groups():
    """nnz(A) = 66,037 x 16 > 65,536 x 16: spgemm_grad_a_kernel strides.  Integer data; 53 patterns tiled, and so are G and
    the expected gA; gB sums every pattern's share times its number of copies."""
    A, B, n, m, _ = C.multirow_case(0)
    Ai, Bi = C.ints(A, 1), C.ints(B, 2)
    rowptr = C.ref32(Ai, Bi, n)[0]
    G = np.random.default_rng(6).integers(-4, 5, rowptr[-1]).astype(np.float32)
    At = C.tile(Ai, m)
    assert len(At[1]) == 16 * m > 65536 * 16
    gA, gB = C.grad_ref(Ai, Bi, n, G, row_weight=np.bincount(np.arange(m) % C.P_TILE))[:2]
    assert np.abs(gB).max() < 2 ** 24
    got = _backward(At, Bi, n, C.tile((rowptr, G, G), m)[1])
    assert np.array_equal(got[0].astype(np.float64), C.tile((Ai[0], gA, gA), m)[1])
    assert np.array_equal(got[1].astype(np.float64), gB)


def test_grad_b_beyond_one_launch_of_groups():
    """nnz(B) = 70,000 x 16 > 65,536 x 16: spgemm_grad_b_kernel strides.  Integer data."""
    A, B, n = C.stride_b_case()
    assert len(B[1]) > 65536 * 16
    nnz = len(C.ref32(A, B, n)[1])
    G = np.random.default_rng(8).integers(-4, 5, nnz).astype(np.float32)
    gA, gB, _, _, _, tB = C.grad_ref(A, B, n, G)
    assert tB[65536 * 16:].sum() > 0 and tB[-16:].sum() > 0  # entries past the first launch have terms
    got = _backward(A, B, n, G)
    assert np.array_equal(got[0].astype(np.float64), gA) and np.array_equal(got[1].astype(np.float64), gB)


# ---- products without an entry ---------------------------------------------------------------------------------------------
def _empty_product(kind):
    rng = np.random.default_rng(30)
    m, k, n = 6, 8, 5
    if kind == "A-meets-empty-rows":  # rows 0 .. 3 of B are empty and A has columns 0 .. 3 only
        A = C.csr_of_rows([(np.sort(rng.choice(4, size=2, replace=False)), rng.standard_normal(2)) for _ in range(m)])
        B = C.csr_of_rows([(np.zeros(0), np.zeros(0))] * 4 + [(np.arange(3), rng.standard_normal(3))] * 4)
    elif kind == "B-empty":
        A = C.csr_of_dense(rng.standard_normal((m, k)))
        B = C.csr_of_rows([(np.zeros(0), np.zeros(0))] * k)
    else:
        A = C.csr_of_rows([(np.zeros(0), np.zeros(0))] * m)
        B = C.csr_of_dense(rng.standard_normal((k, n)))
    return A, B, m, k, n


@pytest.mark.parametrize("kind", ["A-meets-empty-rows", "B-empty", "A-empty"])
def test_backward_through_an_empty_product(kind):
    """nnz(C) = 0: zero gradients of the operands' shapes, an empty operand an empty one -- no error from the backward."""
    A, B, m, k, n = _empty_product(kind)
    assert C.ub(A, B).sum() == 0
    (rA, cA, vA), (rB, cB, vB) = C.to_device(A, DEV), C.to_device(B, DEV)
    vA.requires_grad_()
    vB.requires_grad_()
    rC, cC, vC = spgemm(rA, cA, vA, rB, cB, vB, n)
    assert vC.numel() == 0 and cC.numel() == 0 and rC.tolist() == [0] * (m + 1)
    vC.sum().backward()
    assert vA.grad.shape == vA.shape and vB.grad.shape == vB.shape
    assert not vA.grad.any() and not vB.grad.any()


@pytest.mark.parametrize("kind", ["A-meets-empty-rows", "B-empty", "A-empty"])
def test_spspmm_backward_through_an_empty_product(kind):
    A, B, m, k, n = _empty_product(kind)

    def coo(X):
        rows = np.repeat(np.arange(len(X[0]) - 1), np.diff(X[0]))
        return torch.from_numpy(np.stack([rows, X[1]])).to(DEV), torch.from_numpy(X[2]).to(DEV).requires_grad_()

    (ia, va), (ib, vb) = coo(A), coo(B)
    index, val = torch_sparse_compat.spspmm(ia, va, ib, vb, m, k, n)
    assert index.shape == (2, 0) and val.numel() == 0
    val.sum().backward()
    assert va.grad.shape == va.shape and vb.grad.shape == vb.shape
    assert not va.grad.any() and not vb.grad.any()
