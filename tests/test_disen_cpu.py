"""cogdl_amd.operators.disen on the CPU (tests/_disen_cases.py): the CPU route is the torch composition; the closed-form backward
the HIP kernels implement (ga, dl, p, t, r as written in operators/disen.py, ga and dl from the package's `_ga_dl`) equals the
float64 autograd of the composition; neighbor_routing equals the layer's loop restated per channel, also when the caller hands
the same tensor in as c and z; the C ABI declares the entry points and the ctypes table binds them; shape errors."""
import os
import re
import warnings

import pytest
import torch

import _disen_cases as C
from cogdl_amd import _lib
from cogdl_amd import operators
from cogdl_amd.operators import disen as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cogdl_hip_disen_route_fwd", "cogdl_hip_disen_route_bwd_c", "cogdl_hip_disen_route_bwd_z")


def test_exported():
    assert operators.disen_route is D.disen_route and operators.neighbor_routing is D.neighbor_routing


@pytest.mark.parametrize("K,d,tau", C.CASES + ((4, 3, 1.0), (5, 1, 2.0)))
def test_cpu_route_is_the_composition(K, d, tau):
    row, col = C.graph()
    gen = torch.Generator().manual_seed(5)
    c, z, G = (torch.randn(C.N, K * d, generator=gen) for _ in range(3))
    if d > 1:
        c, z = C.unit(c, K), C.unit(z, K)
    with warnings.catch_warnings(), C.G.edge_order():  # (deterministic mode: the gathers' gradients add in edge order)
        warnings.simplefilter("error")  # the CPU route is quiet, any d
        got = C.run(lambda a, b: D.disen_route(a, b, row, col, K, tau), c, z, G)
        want = C.run(lambda a, b: C.composition(a, b, row, col, K, tau), c, z, G)
    for name in want:
        assert torch.equal(got[name], want[name]), name
    empty = torch.bincount(row, minlength=C.N) == 0
    assert int(empty.sum()) > 40
    assert torch.equal(got["out"][empty], C.unit(z, K)[empty])  # a node without edges: its own z, normalised


@pytest.mark.parametrize("K,d,tau", C.CASES)
def test_closed_form_backward_is_float64_autograd(K, d, tau):
    row, col = C.graph()
    c, z, G = (t.double() for t in C.inputs(K, d))
    oracle, _ = C.reference(K, d, tau)
    g_c, g_z = C.closed_form(c, z, row, col, K, tau, G)
    for name, got in (("g_c", g_c), ("g_z", g_z)):
        err = float((got - oracle[name]).abs().max())
        top = float(oracle[name].abs().max())
        print("K=%d d=%d tau=%g %s  max|closed form - autograd| %.3e  max|autograd| %.3e" % (K, d, tau, name, err, top))
        assert err <= 1e-12 * max(1.0, top)  # float64: 4e3 roundings of 1e-16 at most in a sum, a wrong term is O(1e-2 .. 1)
    no_out = torch.bincount(col, minlength=C.N) == 0
    ga, _ = D._ga_dl(G, *C.composition(c, z, row, col, K, tau, with_norm=True), z, K)
    assert int(no_out.sum()) >= 20 and torch.equal(g_z[no_out], ga[no_out])  # sources without out-edges: the direct term


@pytest.mark.parametrize("K,d", [(3, 4), (2, 5)])
def test_neighbor_routing_is_the_layers_loop(K, d):
    row, col = C.graph()
    gen = torch.Generator().manual_seed(11)
    h = torch.randn(C.N, K * d, generator=gen).double()
    G = torch.randn(C.N, K * d, generator=gen).double()
    ha, hb = h.clone().requires_grad_(), h.clone().requires_grad_()
    got = D.neighbor_routing(ha, row, col, K, 3, 0.7)
    want = C.reference_loop(hb, row, col, K, 3, 0.7)
    got.backward(G)
    want.backward(G)
    assert float((got.detach() - want.detach()).abs().max()) <= 1e-13 and float((ha.grad - hb.grad).abs().max()) <= 1e-12
    assert torch.equal(D.neighbor_routing(h, row, col, K, 0, 0.7), C.unit(h, K))  # no iteration: the normalised features
    # one tensor as c and as z (the loop's first step): autograd adds both gradients
    za, zb = C.unit(h, K).requires_grad_(), C.unit(h, K).requires_grad_()
    one = D.disen_route(za, za, row, col, K, 0.7)
    two = D.disen_route(zb, zb.clone(), row, col, K, 0.7)
    one.backward(G)
    two.backward(G)
    assert torch.equal(one, two) and float((za.grad - zb.grad).abs().max()) <= 1e-14
    assert float((one - C.reference_loop(h, row, col, K, 1, 0.7)).abs().max()) <= 1e-13


def test_symbols_in_the_header_and_the_ctypes_table():
    with open(os.path.join(ROOT, "include", "cogdl_hip.h")) as fh:
        header = fh.read()
    assert "#define COGDL_HIP_ABI_VERSION 9" in header  # additions only
    for name in ENTRY_POINTS:
        for sym in (name, name + "_workspace_bytes"):
            assert re.search(r"COGDL_API\s+\w+\s+%s\(" % sym, header), sym
            assert sym in _lib.HIP_SIGNATURES, sym
            assert hasattr(_lib.hip(), sym), sym
        decl = re.search(r"COGDL_API int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.HIP_SIGNATURES[name][0]), name
    # the workspace covers the piece records of every vector width; nothing for an empty edge list or an uncovered d
    lib = _lib.hip()
    assert lib.cogdl_hip_disen_route_fwd_workspace_bytes(5000, 16, 4) >= lib.cogdl_hip_disen_route_bwd_c_workspace_bytes(5000, 16, 4) > 0
    assert lib.cogdl_hip_disen_route_fwd_workspace_bytes(0, 16, 4) == 0 and lib.cogdl_hip_disen_route_bwd_z_workspace_bytes(5000, 16, 3) == 0


def test_value_errors():
    row, col = C.graph()
    c, z, _ = C.inputs(3, 4)
    with pytest.raises(ValueError):
        D.disen_route(c[:, :8], z, row, col, 3)  # c and z differ
    with pytest.raises(ValueError):
        D.disen_route(c, z, row, col, 5)  # 12 columns, K = 5
    with pytest.raises(ValueError):
        D.disen_route(c, z, row, col, 0)
    with pytest.raises(ValueError):
        D.disen_route(c, z, row[:-1], col, 3)
    with pytest.raises(ValueError):
        D.disen_route(c[0], z[0], row, col, 3)
    with pytest.raises(ValueError):
        D.disen_route(c, z, row, col, 3, tau=0.0)
    with pytest.raises(ValueError):
        D.neighbor_routing(c, row, col, 5, 2)
    with pytest.raises(ValueError):
        D.neighbor_routing(c[0], row, col, 3, 2)
