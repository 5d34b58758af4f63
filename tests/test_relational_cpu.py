"""The relational operator without a GPU: the CPU route is the torch composition byte for byte (values and gradients), the
entry points are declared in the header and resolvable through the ctypes table, and install() takes the flag."""
import contextlib
import inspect
import os
import re
import warnings

import pytest
import torch

from cogdl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cogdl_hip_rel_gspmm_workspace_bytes", "cogdl_hip_rel_gspmm", "cogdl_hip_rel_gspmm_grad_rel_workspace_bytes",
           "cogdl_hip_rel_gspmm_grad_rel")
_OP = {"sub": torch.sub, "mul": torch.mul, "add": torch.add}


@contextlib.contextmanager
def _edge_order_autograd():
    """CPU autograd of x[col] / rel[etype] is index_put_(accumulate=True), which torch runs with atomic adds on several threads
    from 32768 elements on (sums in no fixed order).  Its deterministic form is the sequential loop over the edges: the
    reference order that the kernels reproduce."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was)


def _composition(x, rel, row, col, etype, w, op, n):
    msg = _OP[op](x[col], rel[etype])
    if w is not None:
        msg = msg * w.unsqueeze(-1)
    return torch.zeros(n, x.shape[1]).scatter_add_(0, row.unsqueeze(-1).repeat(1, x.shape[1]), msg)


@pytest.mark.parametrize("op", ["sub", "mul", "add"])
@pytest.mark.parametrize("weighted", [False, True])
def test_cpu_route_is_the_composition(op, weighted):
    from cogdl_amd.operators.relational import rel_gspmm

    gen = torch.Generator().manual_seed(0)
    n, e, r, k = 300, 4000, 6, 13
    row, col = torch.randint(0, n - 20, (e,), generator=gen), torch.randint(0, n, (e,), generator=gen)
    etype = torch.randint(0, r, (e,), generator=gen)
    x, rel, G = torch.randn(n, k, generator=gen), torch.randn(r, k, generator=gen), torch.randn(n, k, generator=gen)
    w = torch.rand(e, generator=gen) if weighted else None
    xa, ra = x.clone().requires_grad_(), rel.clone().requires_grad_()
    xb, rb = x.clone().requires_grad_(), rel.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the CPU route is the reference's own path: quiet
        got = rel_gspmm(xa, ra, row, col, etype, w, op)
    want = _composition(xb, rb, row, col, etype, w, op, n)
    with _edge_order_autograd():
        got.backward(G)
        want.backward(G)
    for a, b in ((got, want), (xa.grad, xb.grad), (ra.grad, rb.grad)):
        assert a.detach().numpy().tobytes() == b.detach().numpy().tobytes()
    assert rel_gspmm(x, rel, row, col, etype, w, op, num_nodes=n + 5).shape == (n + 5, k)


def test_arguments_are_checked():
    from cogdl_amd.operators.relational import rel_gspmm

    x, rel = torch.randn(5, 4), torch.randn(3, 4)
    idx = torch.tensor([0, 1, 2])
    with pytest.raises(ValueError):
        rel_gspmm(x, torch.randn(3, 5), idx, idx, idx)
    with pytest.raises(ValueError):
        rel_gspmm(x, rel, idx, idx, idx, op="corr")
    with pytest.raises(ValueError):
        rel_gspmm(x, rel, idx, idx[:2], idx)
    with pytest.raises(ValueError):
        rel_gspmm(x, rel, idx, idx, idx, weight=torch.ones(2))
    empty = torch.zeros(0, dtype=torch.int64)
    out = rel_gspmm(x, rel, empty, empty, empty)
    assert out.shape == (5, 4) and not out.any()


def test_symbols_are_declared_and_resolvable():
    text = open(os.path.join(ROOT, "include", "cogdl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.hip()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.HIP_SIGNATURES and callable(getattr(lib, name)), name
    assert lib.cogdl_hip_abi_version() == 9
    # pure host queries: the workspace of the two kernels is the engine's, zero without edges
    assert lib.cogdl_hip_rel_gspmm_workspace_bytes(0, 100) == 0 and lib.cogdl_hip_rel_gspmm_workspace_bytes(24000, 100) > 0
    assert lib.cogdl_hip_rel_gspmm_grad_rel_workspace_bytes(24000, 100) == lib.cogdl_hip_rel_gspmm_workspace_bytes(24000, 100)
    # argument validation happens before anything is launched (EINVAL = 1)
    assert lib.cogdl_hip_rel_gspmm(None, None, None, None, None, None, None, 0, None, 4, 4, 0, 1, None, 0, None) == 1
    assert lib.cogdl_hip_rel_gspmm_grad_rel(None, None, None, None, None, None, None, 0, None, 4, 4, 0, None, 0, None) == 1
    assert lib.cogdl_hip_rel_gspmm(None, None, None, None, None, None, None, 0, None, 0, 4, 0, 1, None, 0, None) == 0  # m == 0


def test_install_takes_the_flag():
    import cogdl_amd
    from cogdl_amd import relational_compat

    sig = inspect.signature(cogdl_amd.install)
    assert "relational" in sig.parameters and sig.parameters["relational"].default is False
    assert "relational=True" in cogdl_amd.install.__doc__
    assert callable(relational_compat.message_passing)
    assert "rel_gspmm" in dir(__import__("cogdl_amd.operators.relational", fromlist=["x"]))
