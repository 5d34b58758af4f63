"""pair_lse and grace_loss on the CPU: the blocked torch route against the float64 oracle of tests/_contrast_cases.py under the
rule there, the block size honoured, grace_loss against the reference's formula in float64, the reference's own float32
formula inside the same rule (so the GPU tests' yardstick is known to be satisfiable by the reference alone), and the
argument errors."""
import pytest
import torch

import _contrast_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators import contrast


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_blocked_route_against_the_oracle(case):
    q, k, skip, G = C.inputs(case)
    oracle, ref32 = C.reference(case)
    for block in (None, 16):
        got = C.run(lambda qa, ka, sa: contrast.pair_lse(qa, ka, C.tau_of(case), sa, block=block), q, k, skip, G)
        C.check("%s block %s" % (C.case_id(case), block), got, oracle, ref32)


def test_block_size_is_honoured(monkeypatch):
    case = (70, 150, 24, "arange", "unit", None)
    q, k, skip, _ = C.inputs(case)
    seen = []
    real = torch.logsumexp
    monkeypatch.setattr(torch, "logsumexp", lambda s, *a, **kw: (seen.append(tuple(s.shape)), real(s, *a, **kw))[1])
    out = contrast.pair_lse(q, k, 0.4, skip, block=16)
    assert seen == [(16, 150)] * 4 + [(6, 150)] and out.shape == (70,)
    seen.clear()
    monkeypatch.setattr(contrast, "_BLOCK_BYTES", 150 * 4 * 10)  # the default block: the rows that fit the byte budget
    contrast.pair_lse(q, k, 0.4, skip)
    assert seen == [(10, 150)] * 7


def test_nothing_of_size_m_by_n_is_kept_for_the_backward():
    case = (70, 150, 24, "arange", "unit", None)
    q, k, skip, G = C.inputs(case)
    qa, ka = q.clone().requires_grad_(), k.clone().requires_grad_()
    lse = contrast.pair_lse(qa, ka, 0.4, skip, block=16)
    kept = sorted(tuple(t.shape) for t in lse.grad_fn.saved_tensors if t is not None)
    assert kept == [(70,), (70,), (70, 24), (150, 24)], kept
    seen = []
    real = torch.matmul
    torch.matmul = lambda a, b: (seen.append((tuple(a.shape), tuple(b.shape))), real(a, b))[1]
    try:
        lse.backward(G)
    finally:
        torch.matmul = real
    assert seen and not any(shape in ((70, 150), (150, 70)) for pair in seen for shape in pair), seen  # (blocks of 16 rows only)
    assert ((16, 24), (24, 150)) in seen and ((16, 150), (150, 24)) in seen and ((150, 16), (16, 24)) in seen, seen


def reference_loss(z1, z2, tau):
    """grace_mw.py:64-77, verbatim but for self.tau."""
    z1 = torch.nn.functional.normalize(z1, p=2, dim=-1)
    z2 = torch.nn.functional.normalize(z2, p=2, dim=-1)
    score = lambda a, b: torch.exp(torch.matmul(a, b.t()) / tau)
    intro, inter = score(z1, z1), score(z1, z2)
    return torch.mean(-torch.log(intro.diag() / (intro.sum(1) - intro.diag() + inter.sum(1))))


def _loss_run(fn, z1, z2, dtype):
    a, b = z1.to(dtype).clone().requires_grad_(), z2.to(dtype).clone().requires_grad_()
    loss = fn(a, b)
    loss.backward()
    return {"loss": loss.detach().reshape(1), "g_z1": a.grad, "g_z2": b.grad}


@pytest.mark.parametrize("tau", [0.4, 0.5])
def test_grace_loss_equals_the_reference_formula(tau):
    gen = torch.Generator().manual_seed(70)
    z1, z2 = torch.randn(70, 24, generator=gen), torch.randn(70, 24, generator=gen)
    z1[3] = 0  # a zero row: F.normalize maps it to zero, <a_i, a_i> = 0
    oracle = _loss_run(lambda a, b: reference_loss(a, b, tau), z1, z2, torch.float64)
    ref32 = _loss_run(lambda a, b: reference_loss(a, b, tau), z1, z2, torch.float32)
    ours64 = _loss_run(lambda a, b: contrast.grace_loss(a, b, tau), z1, z2, torch.float64)
    ours32 = _loss_run(lambda a, b: contrast.grace_loss(a, b, tau), z1, z2, torch.float32)
    for name in oracle:  # in float64 the two are one function to rounding
        assert float((ours64[name] - oracle[name]).abs().max()) <= 1e-12 * max(1.0, float(oracle[name].abs().max())), name
    C.check("reference f32 tau %s" % tau, ref32, oracle, ref32)  # (the yardstick itself: satisfiable by the reference)
    C.check("grace_loss tau %s" % tau, ours32, oracle, ref32)


def test_argument_errors_raise_backend_error():
    q, k = torch.randn(6, 4), torch.randn(5, 4)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, torch.randn(5, 3), 0.5)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q[0], k, 0.5)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k, 0.0)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k, -1.0)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k.double(), 0.5)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, torch.randn(0, 4), 0.5)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k, 0.5, torch.zeros(5, dtype=torch.int64))       # one entry per query
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k, 0.5, torch.zeros(6))                          # an index dtype
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k, 0.5, torch.tensor([0, 1, 2, 3, 4, 5]))        # 5 is outside [-1, 5)
    with pytest.raises(_lib.BackendError):
        contrast.pair_lse(q, k, 0.5, torch.tensor([0, 1, -2, 3, 4, 0]))
    assert contrast.pair_lse(q, k, 0.5, torch.tensor([0, 1, -1, 3, 4, 0])).shape == (6,)


def test_exported_from_the_operators_package():
    import cogdl_amd.operators as ops

    assert ops.pair_lse is contrast.pair_lse and ops.grace_loss is contrast.grace_loss
