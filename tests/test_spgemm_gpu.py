"""cogdl_amd.operators.spgemm on the GPU: the structural pattern of C and its values against float64 torch.sparse.mm on
the CPU (|c - c64| <= 1e-5 * sum |a b| per entry), the LDS bins and the global-memory path for rows beyond them,
coalesce, determinism, the value gradients, and the strict refusals."""
import pytest
import torch

from cogdl_amd import _lib, synth
from cogdl_amd.operators.spgemm import coalesce, spgemm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _csr(dense_or_coo, shape=None):
    """CPU COO (indices, values) or dense -> int32 CSR on the GPU + the float64 CPU sparse tensor."""
    if isinstance(dense_or_coo, torch.Tensor):
        s = dense_or_coo.to_sparse().coalesce()
    else:
        idx, val = dense_or_coo
        s = torch.sparse_coo_tensor(idx, val, shape).coalesce()
    s64 = torch.sparse_coo_tensor(s.indices(), s.values().double(), s.shape).coalesce()
    rowptr = torch.zeros(s.shape[0] + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(s.indices()[0], minlength=s.shape[0]).cumsum(0)
    return (rowptr.int().to(DEV), s.indices()[1].int().to(DEV), s.values().float().to(DEV)), s64


def _random(m, n, density, seed):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(m, n, generator=g) < density
    return torch.where(mask, torch.randn(m, n, generator=g), torch.zeros(()))


def _check(a, b, sa=None, sb=None):
    (rA, cA, vA), A64 = _csr(a, sa)
    (rB, cB, vB), B64 = _csr(b, sb)
    n = B64.shape[1]
    rC, cC, vC = spgemm(rA, cA, vA, rB, cB, vB, n)
    want = torch.sparse.mm(A64, B64).coalesce()
    bound = torch.sparse.mm(torch.sparse_coo_tensor(A64.indices(), A64.values().abs(), A64.shape),
                            torch.sparse_coo_tensor(B64.indices(), B64.values().abs(), B64.shape)).coalesce()
    m = A64.shape[0]
    assert rC.numel() == m + 1
    rows = torch.repeat_interleave(torch.arange(m), (rC[1:] - rC[:-1]).long().cpu())
    got_idx = torch.stack([rows, cC.long().cpu()])
    assert torch.equal(got_idx, want.indices()), "pattern differs"
    err = (vC.cpu().double() - want.values()).abs()
    assert bool((err <= 1e-5 * bound.values() + 1e-30).all()), float((err - 1e-5 * bound.values()).max())
    return rC, cC, vC


def test_structural_zero_is_kept():
    a = torch.tensor([[1.0, -1.0], [0.0, 2.0]])
    b = torch.tensor([[1.0, 0.0], [1.0, 0.0]])
    rC, cC, vC = _check(a, b)
    assert rC.tolist() == [0, 1, 2] and cC.tolist() == [0, 0] and vC.tolist() == [0.0, 2.0]


@pytest.mark.parametrize("m,k,n,d,seed", [(37, 53, 29, 0.1, 0), (200, 150, 300, 0.05, 1), (64, 500, 7, 0.3, 2),
                                          (300, 40, 900, 0.2, 3), (1, 1, 1, 1.0, 4)])
def test_random_rectangular(m, k, n, d, seed):
    _check(_random(m, k, d, seed), _random(k, n, d, seed + 100))


def test_empty_operands_and_rows():
    _check(torch.zeros(5, 4), _random(4, 6, 0.5, 0))
    _check(_random(5, 4, 0.5, 1), torch.zeros(4, 6))
    a = _random(30, 20, 0.3, 2)
    a[::3] = 0  # empty rows
    b = _random(20, 25, 0.3, 3)
    b[1::2] = 0
    _check(a, b)
    _check(torch.zeros(0, 3), torch.zeros(3, 4))
    _check(torch.zeros(3, 0), torch.zeros(0, 4))


def test_every_bin_and_the_global_path():
    """Rows with ~1 .. 20 k products: the three LDS bins and the hub path in one product."""
    g = torch.Generator().manual_seed(5)
    k, n = 400, 3000
    b = _random(k, n, 0.02, 6)   # ~60 per row
    rows = []
    for nnz_row in (1, 3, 10, 40, 60, 150, 330):
        r = torch.zeros(k)
        r[torch.randperm(k, generator=g)[:nnz_row]] = torch.randn(nnz_row, generator=g)
        rows.append(r)
    _check(torch.stack(rows), b)


def test_hub_row_forces_the_global_path():
    """One A row that references every row of a dense-ish B: 300 x 2000 products, far beyond an LDS table."""
    a = _random(50, 300, 0.05, 7)
    a[17] = torch.randn(300)
    _check(a, _random(300, 2500, 0.8, 8))


def test_rmat_squared():
    src, dst = synth.rmat_pairs(20000, 120000, seed=3)
    idx = torch.stack([torch.as_tensor(src).long(), torch.as_tensor(dst).long()])
    val = torch.randn(idx.shape[1], generator=torch.Generator().manual_seed(9))
    _check((idx, val), (idx, val), (20000, 20000), (20000, 20000))


def test_bit_identical_across_calls():
    src, dst = synth.rmat_pairs(5000, 60000, seed=4)
    idx = torch.stack([torch.as_tensor(src).long(), torch.as_tensor(dst).long()])
    (rA, cA, vA), _ = _csr((idx, torch.randn(idx.shape[1])), (5000, 5000))
    first = spgemm(rA, cA, vA, rA, cA, vA, 5000)
    for _ in range(2):
        again = spgemm(rA, cA, vA, rA, cA, vA, 5000)
        for x, y in zip(first, again):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_coalesce_duplicates_and_unsorted():
    g = torch.Generator().manual_seed(11)
    m, n, e = 40, 70, 900
    row, col = torch.randint(0, m, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    val = torch.randn(e, generator=g)
    rowptr, colu, valu, mp = coalesce(row.to(DEV), col.to(DEV), val.to(DEV), m, n, return_map=True)
    want = torch.sparse_coo_tensor(torch.stack([row, col]), val.double(), (m, n)).coalesce()
    rows = torch.repeat_interleave(torch.arange(m), (rowptr[1:] - rowptr[:-1]).long().cpu())
    assert torch.equal(torch.stack([rows, colu.long().cpu()]), want.indices())
    torch.testing.assert_close(valu.cpu().double(), want.values(), rtol=1e-5, atol=1e-5)
    key = rows * n + colu.long().cpu()
    assert torch.equal(key[mp.long().cpu()], row * n + col)
    # gradient through coalesce: every input entry receives its canonical entry's gradient
    v = val.to(DEV).requires_grad_()
    _, _, vu = coalesce(row.to(DEV), col.to(DEV), v, m, n)
    w = torch.randn(vu.numel(), device=DEV)
    (vu * w).sum().backward()
    torch.testing.assert_close(v.grad, w[mp.long()])
    with pytest.raises(_lib.BackendError):
        coalesce(row.to(DEV), col.to(DEV), val.to(DEV), m, n - 50)


def _grad_case(m, k, n, e, seed):
    g = torch.Generator().manual_seed(seed)
    ia = torch.stack([torch.randint(0, m, (e,), generator=g), torch.randint(0, k, (e,), generator=g)])
    ib = torch.stack([torch.randint(0, k, (e,), generator=g), torch.randint(0, n, (e,), generator=g)])
    return ia, torch.randn(e, generator=g), ib, torch.randn(e, generator=g)


@pytest.mark.parametrize("m,k,n,e,seed", [(30, 40, 50, 300, 0), (120, 80, 60, 2000, 1), (8, 300, 9, 1500, 2)])
def test_gradients_against_float64_autograd(m, k, n, e, seed):
    """Duplicates included: spspmm-style coalesce -> spgemm, gradients into the ORIGINAL value vectors."""
    ia, va, ib, vb = _grad_case(m, k, n, e, seed)
    a = va.to(DEV).requires_grad_()
    b = vb.to(DEV).requires_grad_()
    rA, cA, vA = coalesce(ia[0].to(DEV), ia[1].to(DEV), a, m, k)
    rB, cB, vB = coalesce(ib[0].to(DEV), ib[1].to(DEV), b, k, n)
    rC, cC, vC = spgemm(rA, cA, vA, rB, cB, vB, n)
    gout = torch.randn(vC.numel(), generator=torch.Generator().manual_seed(seed + 7))
    (vC * gout.to(DEV)).sum().backward()
    a64, b64 = va.double().requires_grad_(), vb.double().requires_grad_()
    C = torch.sparse.mm(torch.sparse_coo_tensor(ia, a64, (m, k)).coalesce(), torch.sparse_coo_tensor(ib, b64, (k, n)).coalesce())
    C = C.coalesce()
    assert C.values().numel() == vC.numel()
    (C.values() * gout.double()).sum().backward()
    torch.testing.assert_close(a.grad.cpu().double(), a64.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(b.grad.cpu().double(), b64.grad, rtol=1e-4, atol=1e-4)


def test_gradient_through_the_global_path():
    a = _random(20, 300, 0.1, 12)
    a[3] = torch.randn(300)
    b = _random(300, 400, 0.5, 13)
    (rA, cA, vA), A64 = _csr(a)
    (rB, cB, vB), B64 = _csr(b)
    vA, vB = vA.requires_grad_(), vB.requires_grad_()
    rC, cC, vC = spgemm(rA, cA, vA, rB, cB, vB, 400)
    vC.sum().backward()
    a64, b64 = A64.values().requires_grad_(), B64.values().requires_grad_()
    torch.sparse.mm(torch.sparse_coo_tensor(A64.indices(), a64, A64.shape),
                    torch.sparse_coo_tensor(B64.indices(), b64, B64.shape)).coalesce().values().sum().backward()
    torch.testing.assert_close(vA.grad.cpu().double(), a64.grad, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(vB.grad.cpu().double(), b64.grad, rtol=1e-4, atol=1e-3)


def test_strict_refusals():
    (rA, cA, vA), _ = _csr(_random(10, 10, 0.3, 14))
    with pytest.raises(_lib.BackendError):
        spgemm(rA.cpu(), cA.cpu(), vA.cpu(), rA.cpu(), cA.cpu(), vA.cpu(), 10)
    with pytest.raises(_lib.BackendError):
        spgemm(rA, cA, vA.double(), rA, cA, vA.double(), 10)
    with pytest.raises(_lib.BackendError):
        spgemm(rA, cA, vA.half(), rA, cA, vA.half(), 10)
    with pytest.raises(_lib.BackendError):
        spgemm(rA.long(), cA.long(), vA, rA.long(), cA.long(), vA, 10)
    with pytest.raises(_lib.BackendError):
        coalesce(torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long), torch.ones(1), 1, 1)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    raised = []
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        try:
            with torch.cuda.graph(graph, stream=s):
                try:
                    spgemm(rA, cA, vA, rA, cA, vA, 10)
                except _lib.BackendError:
                    raised.append(True)
        except Exception:
            pass
    assert raised == [True]
    torch.cuda.synchronize()
    spgemm(rA, cA, vA, rA, cA, vA, 10)  # the device is usable afterwards
