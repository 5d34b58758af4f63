"""pair_lse on GPU tensors: the blocked composition on torch's kernels (no HIP kernel serves the operator), never silent.  Every
case of tests/_contrast_cases.py against the float64 oracle under the rule there, with a block of 16 rows; the route says so once;
an out-of-range skip raises before anything is computed; and the memory condition: what a forward + backward needs does not grow
with M x N."""
import warnings

import pytest
import torch

import _contrast_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
@pytest.mark.filterwarnings("ignore::cogdl_amd.operators.ops.TorchRouteWarning")
def test_blocked_route_against_the_oracle(case):
    from cogdl_amd.operators.contrast import pair_lse

    q, k, skip, G = C.inputs(case)
    oracle, ref32 = C.reference(case)
    got = C.run(lambda qa, ka, sa: pair_lse(qa, ka, C.tau_of(case), sa, block=16), q, k, skip, G, device=DEV)
    C.check(C.case_id(case), got, oracle, ref32)


def test_gpu_calls_say_that_they_run_torch_kernels_once():
    from cogdl_amd.operators import contrast
    from cogdl_amd.operators.ops import _ROUTE_NOTED, TorchRouteWarning

    _ROUTE_NOTED.difference_update({n for n in _ROUTE_NOTED if n[0] == "pair_lse"})
    q, k = torch.randn(8, 4, device=DEV), torch.randn(5, 4, device=DEV)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        a = contrast.pair_lse(q, k, 0.5)
        b = contrast.pair_lse(q, k, 0.5)
    assert [w.category for w in seen] == [TorchRouteWarning], [str(w.message) for w in seen]
    assert torch.equal(a, b)


@pytest.mark.filterwarnings("ignore::cogdl_amd.operators.ops.TorchRouteWarning")
def test_out_of_range_skip_raises_before_anything_is_computed():
    from cogdl_amd import _lib
    from cogdl_amd.operators import contrast

    q, k = torch.randn(8, 4, device=DEV), torch.randn(5, 4, device=DEV)
    ran = []
    real = contrast._BlockedLse.apply
    contrast._BlockedLse.apply = lambda *a: ran.append(a)
    try:
        for bad in ([0, 1, 2, 3, 4, 5, 0, 0], [0, -2, 0, 0, 0, 0, 0, 0]):
            with pytest.raises(_lib.BackendError):
                contrast.pair_lse(q, k, 0.5, torch.tensor(bad, device=DEV))
        with pytest.raises(_lib.BackendError):
            contrast.pair_lse(q, k, 0.5, torch.zeros(7, dtype=torch.int64, device=DEV))
        with pytest.raises(_lib.BackendError):
            contrast.pair_lse(q, k.cpu(), 0.5)
    finally:
        contrast._BlockedLse.apply = real
    assert not ran


@pytest.mark.filterwarnings("ignore::cogdl_amd.operators.ops.TorchRouteWarning")
def test_memory_condition():
    """Derived, not measured: forward + backward at M = N = 4096, d = 64 with blocks of 64 rows may raise the peak by less than
    a quarter of one M x N float32 matrix (16 MiB).  Kept: lse (16 KiB) and the two gradients (2 MiB); working set: scores,
    mask, exp, p, w of one block, 64 x 4096 x 4 bytes = 1 MiB each, and their matmul results.  Any tensor of size M x N fails."""
    from cogdl_amd.operators.contrast import pair_lse

    gen = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(4096, 64, generator=gen), dim=1).to(DEV).requires_grad_()
    k = torch.nn.functional.normalize(torch.randn(4096, 64, generator=gen), dim=1).to(DEV).requires_grad_()
    skip = torch.arange(4096, device=DEV)
    G = torch.ones(4096, device=DEV)
    pair_lse(q.detach()[:64], k.detach(), 0.4, skip[:64], block=64)  # (torch's matmul workspace is in place)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    lse = pair_lse(q, k, 0.4, skip, block=64)
    lse.backward(G)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.2f MiB" % (rise / 2 ** 20))
    assert rise < 4096 * 4096 * 4 // 4
    want = C.composition(q.detach().cpu().double(), k.detach().cpu().double(), 0.4, skip.cpu())
    assert float((lse.detach().cpu().double() - want).abs().max()) <= 64 * C.EPS32 * float(want.abs().max())
