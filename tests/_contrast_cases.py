"""Shared cases of the pair_lse tests (tests/test_contrast_cpu.py, tests/test_contrast_gpu.py): the shapes, the inputs, the
float64 oracle and the acceptance rule.

Oracle: the torch composition -- q k^T / tau, the skipped entry masked to -inf, torch.logsumexp over the keys -- in float64
on the float32 inputs, and the gradients of sum(G * lse) from its autograd, G exactly representable.  (The logsumexp form
stays finite where the reference's plain exp does not.)  Rule, per compared tensor, the project's own (tests/_gen_cases.py):

    err_new <= 4 * err_ref + 8 * eps32 * max|oracle|

err_ref = the error of the SAME composition in float32 on the CPU against the oracle, err_new = the error of the result under
test (max |. - oracle| over the finite entries of the oracle).  Where the oracle is -inf (an empty sum) the result must be
-inf; everything else must be finite.

Cases (M, N, d): the empty sum; odd sizes on both sides with a small d; sizes that are no multiple of 16, 32 or 64 (the row
blocks of the tests, the tiles of any later kernel); d not a multiple of 4 and above 128; d = 256; many keys for few queries.
The last tuple entry is reserved (None).  Queries and keys are random and asymmetric (q is never k): a transposed product
does not pass."""
import functools

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)

SHAPES = [(33, 31, 6), (70, 150, 24), (129, 257, 64), (64, 96, 130), (96, 96, 256), (40, 2100, 128)]
SKIPS = ("none", "minus1", "arange", "tile_edges", "last_tile")

# (M, N, d, skip, tau, reserved): tau "unit" = 0.4 on unit rows, "hot" = 0.01 on unnormalised rows (scores of 100 and more)
CASES = [(1, 1, 1, "none", "unit", None), (1, 1, 1, "zero", "unit", None)]
CASES += [(m, n, d, "arange" if n >= m else "minus1", "unit", None) for (m, n, d) in SHAPES]
CASES += [(70, 150, 24, s, "unit", None) for s in SKIPS if s != "arange"]
CASES += [(40, 2100, 128, s, "unit", None) for s in SKIPS if s != "arange"]
CASES += [(70, 150, 24, "arange", "hot", None), (129, 257, 64, "none", "hot", None), (40, 2100, 128, "tile_edges", "hot", None)]


def case_id(case):
    m, n, d, skip, tau, split = case
    return "%dx%dx%d-%s-%s%s" % (m, n, d, skip, tau, "" if split is None else "-split%d" % split)


def tau_of(case):
    return 0.4 if case[4] == "unit" else 0.01


def make_skip(kind, m, n):
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(m, dtype=torch.int64)
    if kind == "minus1":
        return torch.full((m,), -1, dtype=torch.int64)
    if kind == "arange":
        return torch.arange(m, dtype=torch.int64)
    if kind == "tile_edges":  # the first and last column of 32- and 64-wide key tiles (and -1 now and then)
        edges = [c for c in (0, 31, 32, 63, 64, 127, 128, -1, 447, 448, 2047, 2048) if c < n]
        return torch.tensor([edges[i % len(edges)] for i in range(m)], dtype=torch.int64)
    if kind == "last_tile":  # the ragged last tile: columns 64 * ((n - 1) // 64) .. n - 1
        lo = 64 * ((n - 1) // 64)
        return torch.tensor([lo + (i * 5) % (n - lo) for i in range(m)], dtype=torch.int64)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(q [M, d], k [N, d], skip or None, G [M]) float32 / int64 on the CPU."""
    m, n, d, skip, tau, _ = case
    gen = torch.Generator().manual_seed(7919 * m + 31 * n + d)
    q, k = torch.randn(m, d, generator=gen), torch.randn(n, d, generator=gen)
    if tau == "unit":
        q, k = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(k, dim=1)
    else:
        q, k = q * 1.5, k * 1.5
        assert float((q @ k.t()).abs().max()) / 0.01 >= 100.0  # scores of 100 and more occur
    G = (((torch.arange(m) * 7) % 11 - 5).float() / 4)
    return q, k, make_skip(skip, m, n), G


def composition(q, k, tau, skip):
    s = torch.matmul(q, k.t()) / tau
    if skip is not None:
        s = s.masked_fill(skip.unsqueeze(1) == torch.arange(k.shape[0]).unsqueeze(0), float("-inf"))
    return torch.logsumexp(s, dim=1)


def run(fn, q, k, skip, G, device="cpu", dtype=torch.float32):
    """fn(q, k, skip) -> lse; {"lse", "g_q", "g_k"} on the CPU, the gradients those of sum(G * lse)."""
    qa = q.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    ka = k.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    sa = None if skip is None else skip.to(device)
    lse = fn(qa, ka, sa)
    lse.backward(G.to(device=device, dtype=lse.dtype))
    return {"lse": lse.detach().cpu(), "g_q": qa.grad.cpu(), "g_k": ka.grad.cpu()}


@functools.lru_cache(maxsize=None)
def reference(case):
    """(oracle, ref32): the composition in float64 and in float32 on the CPU, on the same float32 inputs."""
    q, k, skip, G = inputs(case)
    fn = lambda qa, ka, sa: composition(qa, ka, tau_of(case), sa)
    return run(fn, q, k, skip, G, dtype=torch.float64), run(fn, q, k, skip, G)


def check(label, got, oracle, ref32):
    """Print both errors of every tensor, then assert the rule, -inf where the oracle has it and finite values elsewhere."""
    bad = []
    for name, want in oracle.items():
        have = got[name].double()
        finite = torch.isfinite(want)
        assert bool((want[~finite] == float("-inf")).all()) and tuple(have.shape) == tuple(want.shape)
        top = float(want[finite].abs().max()) if bool(finite.any()) else 0.0
        err_ref = float((ref32[name].double() - want)[finite].abs().max()) if bool(finite.any()) else 0.0
        err_new = float((have - want)[finite].abs().max()) if bool(finite.any()) else 0.0
        bound = 4 * err_ref + 8 * EPS32 * top
        line = "%s %-4s err_new %.3e  err_ref %.3e  bound %.3e" % (label, name, err_new, err_ref, bound)
        print(line)
        ok = bool(torch.isfinite(have[finite]).all()) and bool((have[~finite] == float("-inf")).all()) and err_new <= bound
        if not ok:
            bad.append(line)
    assert not bad, bad
