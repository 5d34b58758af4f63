"""cogdl_amd.operators.rgcn on the GPU (csrc/rgcn.hip) against the float64 CPU composition of the two laws
(tests/_rgcn_cases.py): forward and every gradient within |got - want| <= 1e-5 * sum |summands| per element (the bound of
tests/test_message_ops_gpu.py::test_hub_destinations; for bdd the summands are the (edge, i) terms), the same bytes from run to
run; bad ids; the torch routes."""
import warnings

import pytest
import torch

import _rgcn_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators import rgcn_basis_aggregate, rgcn_bdd_aggregate
from cogdl_amd.operators.ops import TorchRouteWarning

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASIS = [(1, 1), (3, 2), (20, 5), (64, 8), (100, 9), (260, 32), (260, 5), (20, 32), (64, None)]  # (in, B); None: alpha=None
BDD = [(1, 1, 1), (1, 7, 3), (4, 5, 5), (5, 40, 40), (8, 64, 64), (2, 16, 24), (3, 20, 4)]


@pytest.fixture(scope="module")
def graph():
    idx = C.coo()
    assert int(torch.bincount(idx[0], minlength=C.N).max()) >= 2500 and not bool((idx[2] == C.UNUSED).any())
    assert int((idx[2] == C.BIG).sum()) > C.E // 2 and int(torch.bincount(idx[0], minlength=C.N)[-C.N // 8:].sum()) == 0
    return idx, tuple(t.to(DEV) for t in idx)


def _check(op, law, a, b, idx, dev_idx, w, G, b_is_none=False, **kw):
    """Two runs of forward + backward: every result within the bound of the float64 law, and the same bytes both times.
    b_is_none: the operator gets None for `b` (the law gets b), and there is no gradient of b to compare."""
    (want, want_abs) = C.reference(law, a, b, *idx, w, C.N, G)
    runs = []
    for _ in range(2):
        ad, bd = a.to(DEV).requires_grad_(), (None if b_is_none else b.to(DEV).requires_grad_())
        out = op(ad, bd, *dev_idx, None if w is None else w.to(DEV), num_nodes=C.N, **kw)
        out.backward(G.to(DEV))
        runs.append((out.detach(), ad.grad) + (() if b_is_none else (bd.grad,)))
    for name, got, again, ref, scale in zip(("out", "grad a", "grad b"), runs[0], runs[1], want, want_abs):
        print("%s: max err %.3e, min slack %.3e" % (name, float((got.double().cpu() - ref).abs().max()),
                                                    float((1e-5 * scale - (got.double().cpu() - ref).abs()).min())))
        assert got.shape == ref.shape and C.within(got, ref, scale), name
        assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes(), name  # no atomics
    return runs[0]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k,n_bases", BASIS)
def test_basis(graph, k, n_bases, weighted):
    idx, dev_idx = graph
    gen = torch.Generator().manual_seed(k * 100 + (n_bases or 0))
    x, w = torch.randn(C.N, k, generator=gen), (torch.rand(C.E, generator=gen) if weighted else None)
    if n_bases is None:  # one basis per type: served with the identity; out and the gradient of x
        G = torch.randn(C.N, C.R, k, generator=gen)
        out, _ = _check(rgcn_basis_aggregate, C.basis_law, x, torch.eye(C.R), idx, dev_idx, w, G, b_is_none=True, num_types=C.R)
        assert out.shape == (C.N, C.R, k) and not out[:, C.UNUSED].any()
        return
    alpha, G = torch.randn(C.R, n_bases, generator=gen), torch.randn(C.N, n_bases, k, generator=gen)
    out, _, g_alpha = _check(rgcn_basis_aggregate, C.basis_law, x, alpha, idx, dev_idx, w, G)
    assert not out[-C.N // 8:].any() and not g_alpha[C.UNUSED].any()  # empty rows, the empty type


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_blocks,bi,bo", BDD)
def test_bdd(graph, n_blocks, bi, bo, weighted):
    idx, dev_idx = graph
    gen = torch.Generator().manual_seed(n_blocks * 10000 + bi * 100 + bo)
    x, W = torch.randn(C.N, n_blocks * bi, generator=gen), torch.randn(C.R, n_blocks, bi, bo, generator=gen)
    w, G = (torch.rand(C.E, generator=gen) if weighted else None), torch.randn(C.N, n_blocks * bo, generator=gen)
    out, _, g_w = _check(rgcn_bdd_aggregate, C.bdd_law, x, W, idx, dev_idx, w, G)
    assert not out[-C.N // 8:].any() and not g_w[C.UNUSED].any()


@pytest.mark.parametrize("which,bad", [(2, C.R), (1, C.N), (0, C.N)])  # a type == R, a source == N, a destination == num_nodes
def test_bad_ids_raise(graph, which, bad):
    idx = [t.clone() for t in graph[0]]
    idx[which][17] = bad
    idx = [t.to(DEV) for t in idx]
    x = torch.randn(C.N, 8, device=DEV)
    with pytest.raises(_lib.BackendError):
        rgcn_basis_aggregate(x, torch.randn(C.R, 2, device=DEV), *idx, num_nodes=C.N)
    with pytest.raises(_lib.BackendError):
        rgcn_bdd_aggregate(x, torch.randn(C.R, 2, 4, 4, device=DEV), *idx, num_nodes=C.N)


def _one_warning(call):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = call()
    assert [w.category for w in seen] == [TorchRouteWarning], [str(w.message) for w in seen]
    return got.cpu().double()


def test_torch_routes(graph):
    idx, dev_idx = graph
    gen = torch.Generator().manual_seed(9)
    x, alpha = torch.randn(C.N, 6, generator=gen), torch.randn(C.R, 33, generator=gen)
    got = _one_warning(lambda: rgcn_basis_aggregate(x.to(DEV), alpha.to(DEV), *dev_idx))
    assert C.within(got, C.basis_law(x.double(), alpha.double(), *idx, None, C.N), C.basis_law(x.double().abs(), alpha.double().abs(), *idx, None, C.N))
    x, W = torch.randn(C.N, 65, generator=gen), torch.randn(C.R, 1, 65, 64, generator=gen)  # bi * bo = 4160
    got = _one_warning(lambda: rgcn_bdd_aggregate(x.to(DEV), W.to(DEV), *dev_idx))
    assert C.within(got, C.bdd_law(x.double(), W.double(), *idx, None, C.N), C.bdd_law(x.double().abs(), W.double().abs(), *idx, None, C.N))
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    got = _one_warning(lambda: rgcn_bdd_aggregate(x[:, :4].to(DEV), W[:, :, :4, :3].to(DEV), empty, empty, empty))
    assert got.shape == (C.N, 3) and not got.any()
