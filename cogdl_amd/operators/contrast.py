"""The row-wise log-sum-exp of a dense pairwise score matrix, and GRACE's contrastive loss on it.

    pair_lse(q, k, tau, skip=None) -> lse [M]                                                (autograd: q, k)
        q [M, d], k [N, d]; skip None, or int32 / int64 [M] with entries in [-1, N) (-1: nothing skipped)
            lse[i] = log SUM_{j != skip[i]} exp(<q[i], k[j]> / tau)             an empty sum gives -inf

    grace_loss(z1, z2, tau) -> scalar
        the reference's contrastive_loss(z1, z2) (cogdl/wrappers/model_wrapper/node_classification/grace_mw.py:64-77):
            a = normalize(z1), b = normalize(z2)
            lse = pair_lse(a, cat([a, b]), tau, skip=arange(M))
            loss = mean(lse - <a_i, a_i> / tau)

The reference computes -log(diag / (refl.sum(1) - diag + between.sum(1))) with refl = exp(a a^T / tau), between =
exp(a b^T / tau) as two [N, N] float32 tensors and diag_i = exp(<a_i, a_i> / tau).  Subtracting diag from the row sum is
leaving j = i out of it -- which is what `skip` does, without the cancellation of the subtraction -- and -log(diag / rest)
= log(rest) - <a_i, a_i> / tau.  <a_i, a_i> is kept as computed: 1 only up to rounding, and 0 for a zero row, which
F.normalize maps to zero.  batched_loss calls contrastive_loss(z1[idx], z2): the keys are then cat([a[idx], b]) with skip =
arange(B), the reference's [B, B] plus [B, N] blocks.

The operator is the torch composition -- matmul, the skipped entry masked to -inf, torch.logsumexp (the maximum subtracted: no
precondition on the size of the scores) -- evaluated in row blocks of the queries, forward AND backward: the forward keeps q,
k, skip and lse only, and the backward recomputes every block's scores.  With p_ij = exp(<q_i, k_j> / tau - lse_i), 0 at j =
skip[i], and g the upstream gradient:

    grad_q[i] = (g_i / tau) * SUM_j p_ij k[j]              grad_k[j] = (1 / tau) * SUM_i g_i p_ij q[i]

So nothing of size [M, N] is kept and the working memory is a few tensors of block x N (`block` rows; by default as many as
keep one of them near 64 MB).  There is NO HIP kernel behind this operator: CPU tensors run it quietly, GPU tensors run the
same blocked composition on torch's kernels and say so once with a TorchRouteWarning, as operators/ops.py does.  A `skip`
entry outside [-1, N) raises BackendError before anything is computed (one read-back of the tensor).
"""
import torch

from .. import _lib
from .ops import _ROUTE_NOTED, TorchRouteWarning

_BLOCK_BYTES = 64 << 20


def _note_torch_route(why):
    if ("pair_lse", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("pair_lse", why))
    import warnings

    warnings.warn("cogdl_amd.operators.contrast.pair_lse: GPU tensors on the torch route (%s): the blocked composition on torch's "
                  "kernels" % why, TorchRouteWarning, stacklevel=3)


def _block_rows(q, k, block):
    m, n = q.shape[0], k.shape[0]
    if block is None:
        block = max(1, _BLOCK_BYTES // (max(n, 1) * q.element_size()))
    return max(1, min(int(block), max(m, 1)))


def _scores(qb, k, tau, skip_b, cols):
    """q_b k^T / tau with the skipped entry at -inf, and the mask (or None)."""
    s = torch.matmul(qb, k.t()) / tau
    if skip_b is None:
        return s, None
    mask = skip_b.to(torch.int64).unsqueeze(1) == cols
    return s.masked_fill(mask, float("-inf")), mask


class _BlockedLse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, skip, tau, block):
        m, n = q.shape[0], k.shape[0]
        cols = torch.arange(n, device=q.device).unsqueeze(0)
        parts = []
        for r0 in range(0, m, block):
            s, _ = _scores(q[r0:r0 + block], k, tau, None if skip is None else skip[r0:r0 + block], cols)
            parts.append(torch.logsumexp(s, dim=1))
        lse = torch.cat(parts) if parts else q.new_empty((0,))
        ctx.tau, ctx.block = tau, block
        ctx.save_for_backward(q, k, skip, lse)
        return lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        q, k, skip, lse = ctx.saved_tensors
        tau, block = ctx.tau, ctx.block
        m, n = q.shape[0], k.shape[0]
        cols = torch.arange(n, device=q.device).unsqueeze(0)
        want_q, want_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_q = torch.empty_like(q) if want_q else None
        g_k = torch.zeros_like(k) if want_k else None
        for r0 in range(0, m, block):
            qb, lb = q[r0:r0 + block], lse[r0:r0 + block]
            s, mask = _scores(qb, k, tau, None if skip is None else skip[r0:r0 + block], cols)
            dead = torch.isinf(lb).unsqueeze(1)  # an empty sum: lse = -inf, every entry masked
            p = torch.exp(s - lb.masked_fill(dead.squeeze(1), 0.0).unsqueeze(1))  # (exponent <= 0 up to rounding)
            p = p.masked_fill(dead if mask is None else (mask | dead), 0.0)
            w = p * (grad[r0:r0 + block] / tau).unsqueeze(1)
            if want_q:
                g_q[r0:r0 + block] = torch.matmul(w, k)
            if want_k:
                g_k += torch.matmul(w.t(), qb)
        return g_q, g_k, None, None, None


def _check_skip(skip, m, n):
    if skip.dim() != 1 or skip.numel() != m or skip.dtype not in (torch.int32, torch.int64):
        raise _lib.BackendError("pair_lse: skip must be int32 or int64 of shape [%d] (got %s %s)"
                                % (m, skip.dtype, tuple(skip.shape)))
    if m == 0:
        return
    lo, hi = int(skip.min()), int(skip.max())
    if lo < -1 or hi >= n:
        raise _lib.BackendError("pair_lse: skip entries must lie in [-1, %d) (got %d .. %d)" % (n, lo, hi))


def pair_lse(q, k, tau, skip=None, *, block=None, _skip_checked=False):
    """q [M, d], k [N, d] -> lse [M] in the dtype of q.  block: query rows per step of the blocked composition.  BackendError
    for arguments that are not 2-D floating tensors of one width and dtype, a tau that is not positive, and a skip of another
    shape, dtype or range."""
    if not (torch.is_tensor(q) and torch.is_tensor(k)) or q.dim() != 2 or k.dim() != 2 or q.shape[1] != k.shape[1]:
        raise _lib.BackendError("pair_lse: q and k must be 2-D of one width (got %s, %s)"
                                % (tuple(getattr(q, "shape", ())), tuple(getattr(k, "shape", ()))))
    (m, d), n = q.shape, k.shape[0]
    if d < 1 or n < 1:
        raise _lib.BackendError("pair_lse: needs at least one key and one column (got N = %d, d = %d)" % (n, d))
    tau = float(tau)
    if not tau > 0:
        raise _lib.BackendError("pair_lse: tau must be positive (got %r)" % tau)
    if q.dtype != k.dtype or not q.is_floating_point():
        raise _lib.BackendError("pair_lse: q and k must be of one floating dtype (got %s, %s)" % (q.dtype, k.dtype))
    if skip is not None:
        if not torch.is_tensor(skip):
            raise _lib.BackendError("pair_lse: skip must be a tensor or None")
        if not _skip_checked:
            _check_skip(skip, m, n)
    tensors = [q, k] + ([] if skip is None else [skip])
    if len({t.device for t in tensors}) != 1:
        raise _lib.BackendError("pair_lse: tensors on %s" % sorted({str(t.device) for t in tensors}))
    if m == 0:
        return q.new_empty((0,))
    if q.is_cuda:
        _note_torch_route("no HIP kernel serves this operator")
    return _BlockedLse.apply(q, k, skip, tau, _block_rows(q, k, block))


def grace_loss(z1, z2, tau, *, block=None):
    """The reference's GRACEModelWrapper.contrastive_loss(z1, z2) with self.tau = tau: z1 [M, d], z2 [N, d] -> scalar."""
    a = torch.nn.functional.normalize(z1, p=2, dim=-1)
    b = torch.nn.functional.normalize(z2, p=2, dim=-1)
    skip = torch.arange(a.shape[0], device=a.device)  # (in range by construction: M <= M + N keys)
    lse = pair_lse(a, torch.cat([a, b]), tau, skip=skip, block=block, _skip_checked=True)
    return torch.mean(lse - (a * a).sum(1) / float(tau))
