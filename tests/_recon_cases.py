"""Inputs and the float64 reference shared by tests/test_recon_cpu.py and tests/test_recon_gpu.py.

A case is (N, d, edges, scale): z = randn(N, d) d^-1/4 (scores of about N(0, 1)), or rescaled so that the largest |score| is
`scale`; edges "none", "dup" (int64, 3 N random edges, the first five repeated, a self loop at every seventh node, no weight) or
"w32" (int32, 3 N random edges with weights in (0, 2)).  The reference is the plain formula, dense, in float64 on the CPU:
softplus(z z^T).sum() - (w * (z[row] * z[col]).sum(1)).sum(), and its autograd gradient."""
import functools

import torch


@functools.lru_cache(maxsize=None)
def inputs(n, d, edges, scale=None):
    gen = torch.Generator().manual_seed(1000 * n + d)
    z = torch.randn(n, d, generator=gen) * d ** -0.25
    if scale is not None:
        z = z * (scale / float((z.double() @ z.double().t()).abs().max())) ** 0.5
    e = 0 if edges == "none" else 3 * n
    row, col = torch.randint(0, n, (e,), generator=gen), torch.randint(0, n, (e,), generator=gen)
    weight = None
    if edges == "dup":
        loops = torch.arange(0, n, 7)
        row, col = torch.cat([row, row[:5], loops]), torch.cat([col, col[:5], loops])
    elif edges == "w32":
        row, col, weight = row.int(), col.int(), 2 * torch.rand(e, generator=gen)
    return z, row, col, weight


@functools.lru_cache(maxsize=None)
def reference(n, d, edges, scale=None):
    """-> (loss, gradient) in float64."""
    z, row, col, weight = inputs(n, d, edges, scale)
    z = z.double().requires_grad_()
    w = torch.ones(row.numel(), dtype=torch.float64) if weight is None else weight.double()
    loss = torch.nn.functional.softplus(z @ z.t(), threshold=1e4).sum() - (w * (z[row.long()] * z[col.long()]).sum(1)).sum()
    loss.backward()
    return loss.detach(), z.grad


def run(fn, n, d, edges, scale=None, device="cpu"):
    """fn(z, row, col, weight) -> loss; -> (loss, gradient) on the CPU."""
    z, row, col, weight = inputs(n, d, edges, scale)
    z = z.clone().to(device).requires_grad_()
    loss = fn(z, row.to(device), col.to(device), None if weight is None else weight.to(device))
    loss.backward()
    return loss.detach().cpu(), z.grad.cpu()


def errors(got, want):
    """|loss - want|, and the worst row of the gradient: max_i |g_i - want_i|_inf / |want_i|_inf."""
    d_loss = float((got[0].double() - want[0]).abs())
    rows = (got[1].double() - want[1]).abs().amax(1) / want[1].abs().amax(1).clamp_min(1e-300)
    return d_loss, float(rows.max()) if rows.numel() else 0.0
