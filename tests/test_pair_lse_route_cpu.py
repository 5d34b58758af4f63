"""The route argument of pair_lse / grace_loss without a GPU: route="hip" never falls back, an unknown route is an error, the
torch route is the default on CPU tensors, and the slice rule of csrc/contrast.hip keeps its workspace inside the stated cap."""
import pytest
import torch

from cogdl_amd import _lib
from cogdl_amd.operators import contrast


def test_route_hip_refuses_what_the_kernels_do_not_serve():
    q, k = torch.randn(6, 4), torch.randn(5, 4)
    for args in ((q, k), (q.double(), k.double())):
        with pytest.raises(_lib.BackendError):
            contrast.pair_lse(*args, 0.5, route="hip")
        with pytest.raises(_lib.BackendError):
            contrast.grace_loss(*args, 0.5, route="hip")
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k, 0.5, route="triton")
    with pytest.raises(_lib.BackendError):
        contrast.grace_loss(q, k, 0.5, route="auto")


def test_torch_route_is_the_default_on_cpu_tensors():
    q, k = torch.randn(6, 4), torch.randn(5, 4)
    skip = torch.tensor([0, 1, -1, 3, 4, 0])
    assert torch.equal(contrast.pair_lse(q, k, 0.5, skip), contrast.pair_lse(q, k, 0.5, skip, route="torch"))
    assert torch.equal(contrast.grace_loss(q, k, 0.5), contrast.grace_loss(q, k, 0.5, route="torch"))


def test_slice_rule_and_workspace_cap():
    lib = _lib.hip()
    m, n, d = 40, 169343 + 40, 256
    assert lib.cogdl_hip_pair_lse_workspace_bytes(m, n, d, 1) == 0
    for which, name in enumerate(("fwd", "grad_q", "grad_k")):
        for shape in ((1, 1, 1), (2708, 5416, 256), (m, n, d)):
            s = lib.cogdl_hip_pair_lse_slices(*shape, which)
            assert s >= 1 and s == contrast.slices(*shape, name)
            rows, other = (shape[1], shape[0]) if which == 2 else (shape[0], shape[1])
            width = 2 if which == 0 else shape[2]
            assert lib.cogdl_hip_pair_lse_workspace_bytes(rows, other, width, s) <= min(64 << 20, shape[0] * shape[1] * 4 // 8)
    assert lib.cogdl_hip_pair_lse_slices(m, n, d, 1) > 1  # few queries, many keys: the keys are cut
