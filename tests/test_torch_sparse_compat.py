"""cogdl_amd.torch_sparse_compat: install(torch_sparse=True) serves `import torch_sparse` only when asked (and only when
the real package is absent), spspmm / spmm match torch on CPU tensors, gradients included; on CUDA tensors both reach
the library's HIP entry points and match the CPU result."""
import collections
import subprocess
import sys

import pytest
import torch

from cogdl_amd import torch_sparse_compat as ts


def _coo(m, n, e, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randint(0, m, (e,), generator=g), torch.randint(0, n, (e,), generator=g)])
    return idx, torch.randn(e, generator=g, dtype=dtype)


def test_install_flag_serves_the_module_and_uninstall_removes_it():
    code = r'''
import importlib, sys
try:
    import torch_sparse
    print("real")
    sys.exit(0)
except ImportError:
    pass
import cogdl_amd
cogdl_amd.install()
try:
    import torch_sparse
    raise SystemExit("plain install() registered torch_sparse")
except ImportError:
    pass
cogdl_amd.install(torch_sparse=True)
from torch_sparse import spspmm, spmm
import torch_sparse
assert torch_sparse.__name__ == "cogdl_amd.torch_sparse_compat", torch_sparse.__name__
cogdl_amd.uninstall()
assert "torch_sparse" not in sys.modules
try:
    import torch_sparse
    raise SystemExit("uninstall() left torch_sparse")
except ImportError:
    pass
print("ok")
'''
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=root))
    assert out.returncode == 0, out.stderr[-2000:]
    if out.stdout.strip() == "real":
        pytest.skip("the real torch_sparse is installed")
    assert out.stdout.strip().endswith("ok")


def test_spspmm_cpu_matches_torch_with_gradients():
    m, k, n = 13, 17, 11
    ia, va = _coo(m, k, 60, 0)
    ib, vb = _coo(k, n, 70, 1)
    ia = torch.cat([ia, torch.tensor([[3, 3], [4, 4]])], 1)  # duplicates, appended out of order
    va = torch.cat([va, torch.tensor([1.0, -2.0], dtype=torch.float64)]).requires_grad_()
    vb = vb.requires_grad_()
    idx, val = ts.spspmm(ia, va, ib, vb, m, k, n, coalesced=True)
    dense = torch.sparse_coo_tensor(ia, va.detach(), (m, k)).to_dense() @ torch.sparse_coo_tensor(ib, vb.detach(), (k, n)).to_dense()
    assert idx.dtype == torch.int64 and idx.shape[0] == 2
    key = idx[0] * n + idx[1]
    assert bool((key[1:] > key[:-1]).all()), "not coalesced / row-major"
    torch.testing.assert_close(val.detach(), dense[idx[0], idx[1]])
    w = torch.randn(val.numel(), dtype=torch.float64)
    (val * w).sum().backward()
    a2, b2 = va.detach().clone().requires_grad_(), vb.detach().clone().requires_grad_()
    d2 = torch.sparse_coo_tensor(ia, a2, (m, k)).to_dense() @ torch.sparse_coo_tensor(ib, b2, (k, n)).to_dense()
    (d2[idx[0], idx[1]] * w).sum().backward()
    torch.testing.assert_close(va.grad, a2.grad)
    torch.testing.assert_close(vb.grad, b2.grad)


def test_spmm_cpu_matches_torch_with_gradients():
    m, n, f = 9, 14, 5
    idx, v = _coo(m, n, 40, 2)
    v = v.requires_grad_()
    x = torch.randn(n, f, dtype=torch.float64, requires_grad=True)
    out = ts.spmm(idx, v, m, n, x)
    a = torch.sparse_coo_tensor(idx, v, (m, n)).to_dense()
    torch.testing.assert_close(out, a @ x)
    out.sum().backward()
    v2, x2 = v.detach().clone().requires_grad_(), x.detach().clone().requires_grad_()
    (torch.sparse_coo_tensor(idx, v2, (m, n)).to_dense() @ x2).sum().backward()
    torch.testing.assert_close(v.grad, v2.grad)
    torch.testing.assert_close(x.grad, x2.grad)


def test_spgemm_abi_refuses_sizes_beyond_int32_before_any_launch():
    """COGDL_HIP_ERANGE (6) for m, k, n, nnz(C) or global-path products beyond the int32 CSR -- checked on the host before
    anything is enqueued, so no device is needed."""
    from cogdl_amd import _lib

    lib = _lib.hip()
    big = 2 ** 31
    assert lib.cogdl_hip_spgemm_count(None, None, None, None, big, 1, 1, None, None, None, 0, None) == 6
    assert lib.cogdl_hip_spgemm_count(None, None, None, None, 1, big, 1, None, None, None, 0, None) == 6
    assert lib.cogdl_hip_spgemm_count(None, None, None, None, 1, 1, big, None, None, None, 0, None) == 6
    assert lib.cogdl_hip_spgemm_fill(*([None] * 6), 4, 4, 4, None, None, big, None, None, 0, None, None, None, None) == 6
    assert lib.cogdl_hip_spgemm_expand(*([None] * 6), 4, None, 1, 2 ** 31 - 2 ** 20 + 1, None, None, None, None, 0, None) == 6
    assert lib.cogdl_hip_spgemm_grad_a(*([None] * 9), 4, big, None) == 6
    assert lib.cogdl_hip_spgemm_grad_b(*([None] * 10), 4, big, None) == 6
    assert lib.cogdl_hip_coo_dupsum(None, None, None, None, 4, big, None, None, None, None, None, 0, None) == 6
    assert lib.cogdl_hip_spgemm_count(None, None, None, None, -1, 1, 1, None, None, None, 0, None) == 1


@pytest.mark.gpu
def test_cuda_calls_reach_the_hip_entry_points_and_match_cpu(monkeypatch):
    from cogdl_amd import _lib

    lib = _lib.hip()
    counts = collections.Counter()
    for name in ("cogdl_hip_spgemm_count", "cogdl_hip_spgemm_fill", "cogdl_hip_coo_dupsum", "cogdl_hip_spgemm_grad_a",
                 "cogdl_hip_spgemm_grad_b", "cogdl_hip_gspmm"):
        fn = getattr(lib, name)

        def call(*a, _n=name, _f=fn):
            counts[_n] += 1
            return _f(*a)

        monkeypatch.setattr(lib, name, call)
    m, k, n = 40, 30, 50
    ia, va = _coo(m, k, 200, 3, torch.float32)
    ib, vb = _coo(k, n, 250, 4, torch.float32)
    a, b = va.cuda().requires_grad_(), vb.cuda().requires_grad_()
    idx, val = ts.spspmm(ia.cuda(), a, ib.cuda(), b, m, k, n)
    val.sum().backward()
    a_c, b_c = va.clone().requires_grad_(), vb.clone().requires_grad_()
    idx_c, val_c = ts.spspmm(ia, a_c, ib, b_c, m, k, n)
    val_c.sum().backward()
    assert torch.equal(idx.cpu(), idx_c)
    torch.testing.assert_close(val.detach().cpu(), val_c.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a.grad.cpu(), a_c.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(b.grad.cpu(), b_c.grad, rtol=1e-5, atol=1e-5)
    for name in ("cogdl_hip_spgemm_count", "cogdl_hip_spgemm_fill", "cogdl_hip_coo_dupsum", "cogdl_hip_spgemm_grad_a",
                 "cogdl_hip_spgemm_grad_b"):
        assert counts[name] >= 1, name
    x = torch.randn(n, 8)
    xs = x.cuda().requires_grad_()
    s = vb.cuda().requires_grad_()
    out = ts.spmm(ib.cuda(), s, k, n, xs)
    out.sum().backward()
    assert counts["cogdl_hip_gspmm"] >= 1
    s_c, x_c = vb.clone().requires_grad_(), x.clone().requires_grad_()
    out_c = ts.spmm(ib, s_c, k, n, x_c)
    out_c.sum().backward()
    torch.testing.assert_close(out.detach().cpu(), out_c.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(s.grad.cpu(), s_c.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xs.grad.cpu(), x_c.grad, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_cuda_empty_inputs_and_int32_limit():
    from cogdl_amd import _lib
    from cogdl_amd.operators.spgemm import coalesce, spgemm

    e = torch.zeros(2, 0, dtype=torch.long, device="cuda")
    v = torch.zeros(0, device="cuda")
    idx, val = ts.spspmm(e, v, e, v, 5, 4, 3)
    assert idx.shape == (2, 0) and val.numel() == 0
    rowptr, col, vals = coalesce(e[0], e[1], v, 5, 4)
    assert rowptr.tolist() == [0] * 6 and col.numel() == 0 and vals.numel() == 0
    ia, va = _coo(6, 5, 20, 5, torch.float32)
    idx, val = ts.spspmm(ia.cuda(), va.cuda(), e, v, 6, 5, 7)  # empty B
    assert idx.shape == (2, 0)
    r, c, x = coalesce(ia[0].cuda(), ia[1].cuda(), va.cuda(), 6, 5)
    with pytest.raises(_lib.BackendError, match="int32"):
        spgemm(r, c, x, r[:6], c, x, 2 ** 31)
    with pytest.raises(_lib.BackendError):  # malformed CSR: a column id beyond k
        spgemm(r, c + 3, x, r[:6], c, x, 5)
