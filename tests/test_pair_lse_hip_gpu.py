"""pair_lse(route="hip"): the streaming MFMA kernels of csrc/contrast.hip against the float64 oracle of tests/_contrast_cases.py
under the rule there (err_new <= 4 err_ref + 8 eps32 max|oracle|, -inf exactly where the oracle has it) -- every case, plus split
cases in the reserved slot (several slices of the walked side; in the last one every row skips key 64, the only key of the second
slice of 64); equal bits from run to run; grace_loss by default on the kernels, silently; one gradient at a time; memory."""
import warnings

import pytest
import torch

import _contrast_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SPLIT_CASES = [(40, 2100, 128, "tile_edges", "unit", 3), (129, 257, 64, "arange", "hot", 2), (70, 150, 24, "last_tile", "unit", 2),
               (33, 65, 6, "last_tile", "unit", 2)]


def _hip(case):
    from cogdl_amd.operators.contrast import pair_lse

    return lambda qa, ka, sa: pair_lse(qa, ka, C.tau_of(case), sa, route="hip", split=case[5])


@pytest.mark.parametrize("case", C.CASES + SPLIT_CASES, ids=C.case_id)
def test_kernels_against_the_oracle_and_equal_from_run_to_run(case):
    q, k, skip, G = C.inputs(case)
    oracle, ref32 = C.reference(case)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = C.run(_hip(case), q, k, skip, G, device=DEV)
        again = C.run(_hip(case), q, k, skip, G, device=DEV)
    C.check(C.case_id(case), got, oracle, ref32)
    for name in got:  # no float atomics
        assert torch.equal(got[name], again[name]), name


def _reference_loss(z1, z2, tau):
    """grace_mw.py:64-77 but for self.tau, as in tests/test_contrast_cpu.py."""
    z1, z2 = torch.nn.functional.normalize(z1, p=2, dim=-1), torch.nn.functional.normalize(z2, p=2, dim=-1)
    score = lambda a, b: torch.exp(torch.matmul(a, b.t()) / tau)
    intro, inter = score(z1, z1), score(z1, z2)
    return torch.mean(-torch.log(intro.diag() / (intro.sum(1) - intro.diag() + inter.sum(1))))


def _loss_run(fn, z1, z2, dtype, device="cpu"):
    a, b = (z.detach().clone().to(device=device, dtype=dtype).requires_grad_() for z in (z1, z2))
    loss = fn(a, b)
    loss.backward()
    return {"loss": loss.detach().reshape(1).cpu(), "g_z1": a.grad.cpu(), "g_z2": b.grad.cpu()}


@pytest.mark.parametrize("tau", [0.4, 0.5])
def test_grace_loss_runs_the_kernels_by_default_without_a_warning(tau):
    from cogdl_amd.operators.contrast import grace_loss

    gen = torch.Generator().manual_seed(70)
    z1, z2 = torch.randn(70, 24, generator=gen), torch.randn(70, 24, generator=gen)
    z1[3] = 0  # a zero row
    oracle = _loss_run(lambda a, b: _reference_loss(a, b, tau), z1, z2, torch.float64)
    ref32 = _loss_run(lambda a, b: _reference_loss(a, b, tau), z1, z2, torch.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = _loss_run(lambda a, b: grace_loss(a, b, tau), z1, z2, torch.float32, device=DEV)
    C.check("grace_loss tau %s" % tau, got, oracle, ref32)


@pytest.mark.parametrize("side", ["q", "k"])
def test_one_gradient_alone_is_the_same_bits(side):
    case = (129, 257, 64, "arange", "unit", 2)
    q, k, skip, G = C.inputs(case)
    both = C.run(_hip(case), q, k, skip, G, device=DEV)
    qa, ka = q.to(DEV).requires_grad_(side == "q"), k.to(DEV).requires_grad_(side == "k")
    _hip(case)(qa, ka, skip.to(DEV)).backward(G.to(DEV))
    wanted, other = (qa, ka) if side == "q" else (ka, qa)
    assert other.grad is None
    assert torch.equal(wanted.grad.cpu(), both["g_" + side])


def test_memory_condition():
    """Derived, not measured: forward + backward at M = N = 4096, d = 64 may raise the peak by less than a quarter of one M x N
    float32 matrix (16 MiB).  Kept: lse and its companion vector (16 KiB each) and the two gradients (1 MiB each).  Workspace:
    cogdl_hip_pair_lse_slices cuts the walked side into 1024 / 64 = 16 slices, capped by an eighth of M x N floats = 8 MiB of
    partials: the forward's 16 x 4096 (max, sum) pairs are 512 KiB (freed before the backward), a gradient's 8 slices of 1 MiB
    are 8 MiB, one workspace for both passes.  2 + 8 MiB and small change; any tensor of size M x N fails."""
    from cogdl_amd import _lib
    from cogdl_amd.operators.contrast import pair_lse, slices

    m = n = 4096
    ws = max(_lib.hip().cogdl_hip_pair_lse_workspace_bytes(m, n, 64, slices(m, n, 64, w)) for w in ("grad_q", "grad_k"))
    assert ws <= m * n * 4 // 8
    gen = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(m, 64, generator=gen), dim=1).to(DEV).requires_grad_()
    k = torch.nn.functional.normalize(torch.randn(n, 64, generator=gen), dim=1).to(DEV).requires_grad_()
    skip = torch.arange(m, device=DEV)
    G = torch.ones(m, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    lse = pair_lse(q, k, 0.4, skip, route="hip")
    lse.backward(G)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.2f MiB, workspace %.2f MiB" % (rise / 2 ** 20, ws / 2 ** 20))
    assert rise < m * n * 4 // 4
    want = C.composition(q.detach().cpu().double(), k.detach().cpu().double(), 0.4, skip.cpu())
    assert float((lse.detach().cpu().double() - want).abs().max()) <= 64 * C.EPS32 * float(want.abs().max())
