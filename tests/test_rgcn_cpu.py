"""cogdl_amd.operators.rgcn without a GPU: the CPU route of both operators equals the float64 composition of the laws
(tests/_rgcn_cases.py) to float32 rounding; the library exports the entry points; install(rgcn=True) / uninstall() rebinds and
restores RGCNLayer's two methods and the rebound layer runs on CPU tensors (tests/_rgcn_layer_run.py, in a fresh interpreter
against the reference package build() stages under oracle/_ref/pkg, or $COGDL_REFERENCE)."""
import inspect
import os
import subprocess
import sys
import warnings

import pytest
import torch

import _rgcn_cases as C
from cogdl_amd.operators import rgcn_basis_aggregate, rgcn_bdd_aggregate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")


@pytest.mark.parametrize("op,law,shapes", [(rgcn_basis_aggregate, C.basis_law, ((C.N, 12), (C.R, 5), (C.N, 5, 12))),
                                           (rgcn_bdd_aggregate, C.bdd_law, ((C.N, 12), (C.R, 3, 4, 5), (C.N, 15)))])
def test_cpu_route_is_the_law(op, law, shapes):
    gen = torch.Generator().manual_seed(1)
    a, b, G = (torch.randn(*s, generator=gen) for s in shapes)
    idx, w = C.coo(), torch.rand(C.E, generator=gen)
    want, scale = C.reference(law, a, b, *idx, w, C.N, G)
    ar, br = a.clone().requires_grad_(), b.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the CPU route is quiet
        out = op(ar, br, *idx, w, num_nodes=C.N)
    out.backward(G)
    for got, ref, s in zip((out.detach(), ar.grad, br.grad), want, scale):
        assert C.within(got, ref, s)


def test_alpha_none_is_the_identity():
    idx, x = C.coo(), torch.randn(C.N, 6, generator=torch.Generator().manual_seed(2))
    xr = x.clone().requires_grad_()
    got = rgcn_basis_aggregate(xr, None, *idx, num_types=C.R)
    got.backward(torch.ones_like(got))
    xe = x.clone().requires_grad_()
    want = rgcn_basis_aggregate(xe, torch.eye(C.R), *idx)
    want.backward(torch.ones_like(want))
    assert got.shape == (C.N, C.R, 6) and torch.allclose(got, want, atol=1e-5) and torch.allclose(xr.grad, xe.grad, atol=1e-4)


def test_install_takes_the_flag_and_the_library_sizes_its_workspaces():
    import cogdl_amd
    from cogdl_amd import _lib

    assert inspect.signature(cogdl_amd.install).parameters["rgcn"].default is False
    lib = _lib.hip()
    assert lib.cogdl_hip_rgcn_basis_workspace_bytes(0, 100) == 0 and lib.cogdl_hip_rgcn_basis_workspace_bytes(5000, 100) > 0
    assert lib.cogdl_hip_rgcn_bdd_grad_w_workspace_bytes(5000, 7, 4, 5, 5) > 0
    assert lib.cogdl_hip_rgcn_bdd_grad_w_workspace_bytes(5000, 7, 1, 65, 64) == 0  # bi * bo > 4096: not served


@pytest.mark.skipif(not REF or not os.path.isdir(os.path.join(REF, "cogdl")), reason="reference package not present")
def test_rebound_layer_runs_on_cpu_tensors():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_rgcn_layer_run.py"), ROOT, REF, "cpu"],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0 and "RGCN-LAYER-OK" in proc.stdout, proc.stdout[-3000:] + proc.stderr[-4000:]
