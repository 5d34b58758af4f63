"""cogdl_amd.operators.disen.disen_route on the GPU (cogdl_hip_disen_route_fwd / _bwd_c / _bwd_z, csrc/disen.hip) on the cases of
tests/_disen_cases.py:
  * every (K, d, tau): output, g_c and g_z against the float64 oracle under the rule err_new <= 4 err_ref + 8 eps32 max|oracle|,
    hub rows included; two runs give the same bytes; destinations without edges return z normalised; the g_z of a source
    without out-edges is ga;
  * tau = 0.01: scores up to 100, finite and inside the rule (the maximum is carried);
  * c and z at a storage offset of 1 and 2 floats: the vector-width 1 and 2 paths chosen by pointer alignment;
  * an out-of-range col raises before any launch; d = 3 and float64 take the torch route with one warning each;
  * a second call on the same index tensors is captured and replayed on one stream."""
import warnings

import pytest
import torch

import _disen_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators import disen as D
from cogdl_amd.operators.ops import TorchRouteWarning

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dev_graph():
    """The same index tensors for every case: the plans are built once."""
    return tuple(t.to(DEV) for t in C.graph())


def _ours(dev_graph, K, tau):
    row, col = dev_graph
    return lambda c, z: D.disen_route(c, z, row, col, K, tau)


def _same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("K,d,tau", C.CASES)
def test_against_the_oracle(dev_graph, K, d, tau):
    row, col = C.graph()
    c, z, G = C.inputs(K, d)
    oracle, ref32 = C.reference(K, d, tau)
    seen = []
    real = D._ga_dl
    D._ga_dl = lambda *a: (seen.append(real(*a)), seen[-1])[1]  # what the backward hands to the two kernels
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the kernel's route: no TorchRouteWarning
            got = C.run(_ours(dev_graph, K, tau), c, z, G, device=DEV)
            again = C.run(_ours(dev_graph, K, tau), c, z, G, device=DEV)
    finally:
        D._ga_dl = real
    C.check("gpu K=%d d=%d tau=%g" % (K, d, tau), got, oracle, ref32)
    assert all(_same(again[k], got[k]) for k in got)  # no atomics, fixed merge order
    # destinations without edges: z / ||z||.  Against the float64 quotient: d squares and at most 3 + log2(d / VEC) <= 7 adds,
    # each half an ulp of a sum <= 1 (4 eps32), halved by the root, plus the root's and the quotient's rounding: 3 eps32.
    empty = torch.bincount(row, minlength=C.N) == 0
    assert int(empty.sum()) > 40
    assert float((got["out"][empty].double() - C.unit(z.double(), K)[empty]).abs().max()) <= 3 * C.G.EPS32
    # a source without out-edges: the direct term alone, bit for bit
    no_out = torch.bincount(col, minlength=C.N) == 0
    assert int(no_out.sum()) >= 20 and len(seen) == 2
    assert _same(got["g_z"][no_out], seen[0][0].cpu()[no_out])
    if tau < 0.1:
        top = float((C.softmax_parts(c, z, row, col, K, tau)[1]).abs().max())
        assert top > 40, top  # unit vectors of 64 columns: |cos| up to ~0.47, scores of 40 and more (exp: 2e17 and more)
        assert all(bool(torch.isfinite(v).all()) for v in got.values())


@pytest.mark.parametrize("offset", [1, 2])
@pytest.mark.parametrize("K,d,tau", [(16, 4, 1.0), (8, 8, 0.5)])
def test_misaligned_tables_take_the_narrow_vector_paths(dev_graph, offset, K, d, tau):
    """c and z that start 4 (8) bytes into their storage: vector width 1 (2) by pointer alignment, a channel 4 / 8 (2 / 4)
    lanes wide, with the workspace sized for every width."""
    c, z, G = C.inputs(K, d)
    oracle, ref32 = C.reference(K, d, tau)

    def shifted(t):
        store = torch.zeros(t.numel() + offset, device=DEV)
        view = store[offset:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
        return view.requires_grad_()

    cs, zs = shifted(c), shifted(z)
    out = _ours(dev_graph, K, tau)(cs, zs)
    out.backward(G.to(DEV))
    got = {"out": out.detach().cpu(), "g_c": cs.grad.cpu(), "g_z": zs.grad.cpu()}
    C.check("gpu K=%d d=%d offset %d" % (K, d, offset), got, oracle, ref32)


def test_errors_and_routes(dev_graph):
    row, col = C.graph()
    c, z, _ = C.inputs(3, 4)
    cd, zd = c.to(DEV), z.to(DEV)
    for which, bad in ((1, C.N), (1, -1), (0, C.N)):  # refused by the plan of that view: no kernel gathers
        idx = [row.clone(), col.clone()]
        idx[which][17] = bad
        with pytest.raises(_lib.BackendError):
            D.disen_route(cd, zd, idx[0].to(DEV), idx[1].to(DEV), 3)
    D._ROUTE_NOTED.clear()
    want = C.composition(c.double(), z.double(), row, col, 3, 1.0)
    with pytest.warns(TorchRouteWarning) as rec:  # another dtype
        got = D.disen_route(cd.double(), zd.double(), *dev_graph, 3)
    assert len([w for w in rec if w.category is TorchRouteWarning]) == 1
    assert got.dtype == torch.float64 and torch.allclose(got.cpu(), want, rtol=1e-12, atol=1e-12)
    with pytest.warns(TorchRouteWarning) as rec:  # d == 3
        got = D.disen_route(cd, zd, *dev_graph, 4)
    assert len([w for w in rec if w.category is TorchRouteWarning]) == 1
    assert torch.allclose(got.cpu().double(), C.composition(c.double(), z.double(), row, col, 4, 1.0), rtol=1e-4, atol=1e-5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the second call of each kind is silent
        D.disen_route(cd.double(), zd.double(), *dev_graph, 3)
        D.disen_route(cd, zd, *dev_graph, 4)
    with pytest.warns(TorchRouteWarning):  # d == 1: the output is a sign
        assert D.disen_route(cd, zd, *dev_graph, 12).abs().eq(1).all()
    with pytest.warns(TorchRouteWarning), pytest.raises(RuntimeError):  # tensors on two devices: said, then torch's own error
        D.disen_route(cd, z, *dev_graph, 3)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    with pytest.warns(TorchRouteWarning):  # E == 0: z normalised
        out = D.disen_route(cd, zd, empty, empty, 3)
    assert torch.allclose(out.cpu(), z, rtol=0, atol=1e-6)
    with pytest.warns(TorchRouteWarning):  # an empty z
        assert D.disen_route(cd[:0], zd[:0], empty.clone(), empty.clone(), 3).shape == (0, 12)


def test_capture_on_one_stream(dev_graph):
    K, d, tau = 16, 4, 1.0
    c, z, G = C.inputs(K, d)
    cd, zd = c.to(DEV).requires_grad_(), z.to(DEV).requires_grad_()
    Gd = G.to(DEV)

    def step():
        out = D.disen_route(cd, zd, *dev_graph, K, tau)
        g_c, g_z = torch.autograd.grad(out, [cd, zd], Gd)
        return out.detach(), g_c, g_z

    want = [t.clone() for t in step()]  # (the plans, the int32 copies and the workspaces exist after this)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(got, want))
