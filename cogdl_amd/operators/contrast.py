"""The row-wise log-sum-exp of a dense pairwise score matrix, and GRACE's contrastive loss on it.

    pair_lse(q, k, tau, skip=None, *, block=None, route=None, split=None) -> lse [M]         (autograd: q, k)
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

Two routes compute it.  route="hip" (float32 CUDA tensors, d <= 256; what grace_loss picks for such inputs): the streaming MFMA
kernels of csrc/contrast.hip -- score tiles of 64 x 64 from v_mfma_f32_32x32x2_f32, an online {max, sum} per query in the forward,
the scores recomputed in two backward passes (one per gradient), no float atomics, nothing of size block x N; it keeps q, k,
skip, lse and one more [M] vector (what lse * tau does not hold of the row's normaliser in float32).  d above 256 is not
chunked: route="hip" raises BackendError there and grace_loss takes the torch route with its warning.  split= overrides the
number of slices the walked side is cut into (tests).  float16 and bfloat16 CUDA tensors run the same passes on
v_mfma_f32_32x32x16_f16 / _bf16 (csrc/contrast16.hip): fp32 arithmetic on the operands as given, lse and its companion vector
kept in float32, the returned lse and each gradient rounded once to the operands' dtype.

The torch route (route=None or "torch" in pair_lse) is the torch composition -- matmul, the skipped entry masked to -inf, torch.logsumexp (the maximum subtracted: no
precondition on the size of the scores) -- evaluated in row blocks of the queries, forward AND backward: the forward keeps q,
k, skip and lse only, and the backward recomputes every block's scores.  With p_ij = exp(<q_i, k_j> / tau - lse_i), 0 at j =
skip[i], and g the upstream gradient:

    grad_q[i] = (g_i / tau) * SUM_j p_ij k[j]              grad_k[j] = (1 / tau) * SUM_i g_i p_ij q[i]

So nothing of size [M, N] is kept and the working memory is a few tensors of block x N (`block` rows; by default as many as
keep one of them near 64 MB).  CPU tensors run it quietly, GPU tensors run the same blocked composition on torch's kernels and
say so once with a TorchRouteWarning that names route="hip", as operators/ops.py does.  On either route a `skip` entry outside
[-1, N) raises BackendError before anything is computed (one read-back of the tensor).  Which route is faster where:
profiles/contrast_bench.txt (tools/contrast_bench.py), DESIGN.md.
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


ROUTES = (None, "torch", "hip")
HIP_MAX_D = 256  # the widest rows csrc/contrast.hip keeps in LDS; wider rows are the torch route's
# grace_loss(route=None) takes the torch route where the score matrix has strictly between these many entries: forward + backward
# measured slower on the kernels at M = 2708, N' = 5416 (1.11x at d = 128, 1.69x at d = 256: too few workgroups), faster or level
# at 1024 x 2048 = 2^21 and from 8192 x 16384 = 2^27 up; what lies between those two is unmeasured (profiles/contrast_bench.txt)
_TORCH_FASTER = (1 << 21, 1 << 27)


def slices(m, n, d, which):
    """The slices csrc/contrast.hip cuts the walked side into: which = "fwd", "grad_q" or "grad_k"."""
    return int(_lib.hip().cogdl_hip_pair_lse_slices(int(m), int(n), int(d), ("fwd", "grad_q", "grad_k").index(which)))


# the 16-bit operand types csrc/contrast16.hip serves, and their COGDL_HIP_* codes
_HIP16 = {torch.float16: 1, torch.bfloat16: 2}
# grace_loss(route=None) on 16-bit inputs: as _TORCH_FASTER, but measured on the 16-bit kernels against what those inputs ran
# before (the blocked composition in their own dtype), and for d > 128 only.  Forward + backward, kernels / torch, float16 and
# bfloat16: d <= 128 faster at every measured size (0.76x to 0.80x from 70 x 140 to 2708 x 5416, 0.48x at 8192 x 16384);
# d = 256 0.88x / 0.91x at 1024 x 2048 = 2^21, SLOWER at 2708 x 5416 (1.24x / 1.19x: too few workgroups, as for float32),
# 0.95x / 0.92x at 8192 x 16384 = 2^27, 0.84x / 0.82x and 0.59x / 0.57x beyond (profiles/contrast_bench.txt)
_TORCH_FASTER16 = (1 << 21, 1 << 27)
_TORCH_FASTER16_ABOVE_D = 128


def _hip_served(q):
    return q.is_cuda and (q.dtype == torch.float32 or q.dtype in _HIP16) and q.shape[1] <= HIP_MAX_D


class _HipLse(torch.autograd.Function):
    """The kernels of csrc/contrast.hip (float32 q, k) and csrc/contrast16.hip (float16, bfloat16).  Keeps q, k, skip, lse and
    corr ([M]: what lse * tau does not hold of a row's normaliser in float32), and nothing else.  lse and corr are float32 for
    every operand dtype; the gradients arrive in the operands' dtype."""

    @staticmethod
    def forward(ctx, q, k, skip, tau, split):
        (m, d), n = q.shape, k.shape[0]
        dev = q.device
        lse, corr = torch.empty(m, dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.float32, device=dev)
        n_slices = slices(m, n, d, "fwd") if split is None else split
        ws, ws_bytes = _lib.workspace("cogdl_hip_pair_lse_workspace_bytes", dev, m, n, 2, n_slices)
        with _lib.on_device(dev):
            if q.dtype in _HIP16:
                rc = _lib.hip().cogdl_hip_pair_lse16_fwd(_lib.ptr(q), _lib.ptr(k), _HIP16[q.dtype], _lib.ptr(skip), m, n, d, tau,
                                                         n_slices, _lib.ptr(lse), _lib.ptr(corr), _lib.ptr(ws), ws_bytes,
                                                         _lib.stream_of(q))
            else:
                rc = _lib.hip().cogdl_hip_pair_lse_fwd(_lib.ptr(q), _lib.ptr(k), _lib.ptr(skip), m, n, d, tau, n_slices,
                                                       _lib.ptr(lse), _lib.ptr(corr), _lib.ptr(ws), ws_bytes, _lib.stream_of(q))
        _lib.check(rc, "pair_lse_fwd")
        ctx.tau, ctx.split = tau, split
        ctx.save_for_backward(q, k, skip, lse, corr)
        ctx.mark_non_differentiable(corr)
        return lse, corr

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad, _grad_corr):
        q, k, skip, lse, corr = ctx.saved_tensors
        (m, d), n = q.shape, k.shape[0]
        dev = q.device
        want_q, want_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_q or want_k):
            return None, None, None, None, None
        grad = grad.to(torch.float32).contiguous()
        g_q = torch.empty_like(q) if want_q else None
        g_k = torch.empty_like(k) if want_k else None
        s_q = (slices(m, n, d, "grad_q") if ctx.split is None else ctx.split) if want_q else 1
        s_k = (slices(m, n, d, "grad_k") if ctx.split is None else ctx.split) if want_k else 1
        # one workspace, the larger of the two passes' (they run one after the other)
        rows, other, n_slices = max([(m, n, s_q), (n, m, s_k)], key=lambda a: a[0] * a[2] * (a[2] > 1))
        half = q.dtype in _HIP16
        ws, ws_bytes = _lib.workspace("cogdl_hip_pair_lse16_workspace_bytes" if half else "cogdl_hip_pair_lse_workspace_bytes", dev,
                                      rows, other, d, n_slices)
        with _lib.on_device(dev):
            if half:
                rc = _lib.hip().cogdl_hip_pair_lse16_grad(_lib.ptr(q), _lib.ptr(k), _HIP16[q.dtype], _lib.ptr(skip), _lib.ptr(lse),
                                                          _lib.ptr(corr), _lib.ptr(grad), m, n, d, ctx.tau, s_q, s_k, _lib.ptr(g_q),
                                                          _lib.ptr(g_k), _lib.ptr(ws), ws_bytes, _lib.stream_of(q))
            else:
                rc = _lib.hip().cogdl_hip_pair_lse_grad(_lib.ptr(q), _lib.ptr(k), _lib.ptr(skip), _lib.ptr(lse), _lib.ptr(corr),
                                                        _lib.ptr(grad), m, n, d, ctx.tau, s_q, s_k, _lib.ptr(g_q), _lib.ptr(g_k),
                                                        _lib.ptr(ws), ws_bytes, _lib.stream_of(q))
        _lib.check(rc, "pair_lse_grad")
        return g_q, g_k, None, None, None


def pair_lse(q, k, tau, skip=None, *, block=None, route=None, split=None, _skip_checked=False, _lse32=False):
    """q [M, d], k [N, d] -> lse [M] in the dtype of q.  route: None or "torch" -- the blocked composition (block: its query rows
    per step), "hip" -- the kernels of csrc/contrast.hip (float32) or csrc/contrast16.hip (float16, bfloat16: fp32 arithmetic on
    the operands as given, lse the kernel's float32 value rounded once, the gradients rounded once in the operands' dtype);
    split: their slice count, for tests; by default the library's rule.
    BackendError for arguments that are not 2-D floating tensors of one width and dtype, a tau that is not positive, a skip of
    another shape, dtype or range, an unknown route, and for route="hip" on what the kernels do not serve: CPU tensors, float64,
    d above 256."""
    if route not in ROUTES:
        raise _lib.BackendError("pair_lse: route must be one of %s (got %r)" % (ROUTES, route))
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
    if route == "hip":
        if not _hip_served(q):
            raise _lib.BackendError("pair_lse: route=\"hip\" serves float32, float16 and bfloat16 CUDA tensors with d <= %d (got %s on %s, d = %d); "
                                    "there is no fallback behind it" % (HIP_MAX_D, q.dtype, q.device, d))
        if split is not None and int(split) < 1:
            raise _lib.BackendError("pair_lse: split must be at least 1 (got %r)" % (split,))
        if max(m, n) >= 2 ** 31 - 1:
            raise _lib.BackendError("pair_lse: sizes beyond int32 indexing")
    if m == 0:
        return q.new_empty((0,))
    if route == "hip":
        skip32 = None if skip is None else skip.to(torch.int32).contiguous()
        lse = _HipLse.apply(q.contiguous(), k.contiguous(), skip32, tau, None if split is None else int(split))[0]
        return lse if _lse32 else lse.to(q.dtype)  # (16-bit operands: the kernel's float32 value, rounded once)
    if q.is_cuda:
        _note_torch_route("the blocked composition; route=\"hip\" runs the kernels of csrc/contrast.hip")
    return _BlockedLse.apply(q, k, skip, tau, _block_rows(q, k, block))


def _grace_loss16(z1, z2, tau, dtype):
    """grace_loss on the 16-bit kernels: the rows normalised in float32 and rounded once to `dtype`, the kernel's float32 lse
    (not its rounded copy), <a_i, a_i> of the rounded rows in float32; a float32 scalar.  The gradient reaches z1, z2 in their own
    dtype through the casts."""
    a = torch.nn.functional.normalize(z1.float(), p=2, dim=-1).to(dtype)
    b = torch.nn.functional.normalize(z2.float(), p=2, dim=-1).to(dtype)
    skip = torch.arange(a.shape[0], device=a.device)
    lse = pair_lse(a, torch.cat([a, b]), tau, skip=skip, route="hip", _skip_checked=True, _lse32=True)
    a32 = a.float()
    return torch.mean(lse - (a32 * a32).sum(1) / float(tau))


def grace_loss(z1, z2, tau, *, block=None, route=None, cast=None):
    """The reference's GRACEModelWrapper.contrastive_loss(z1, z2) with self.tau = tau: z1 [M, d], z2 [N, d] -> scalar.
    route=None: the kernels for what they serve (float32, float16 and bfloat16 CUDA tensors, d <= 256) except where they measured
    slower (_TORCH_FASTER: between 2^21 and 2^27 scores; _TORCH_FASTER16 for 16-bit operands with d > 128), the torch route for everything
    else; "torch" / "hip" as for pair_lse.  On the 16-bit kernels the rows are normalised in float32 and rounded once, and the loss
    is a float32 scalar.  cast: torch.float16 or torch.bfloat16 -- what contrast_compat passes under torch.autocast: float32 or
    16-bit CUDA inputs run the 16-bit kernels in that dtype wherever route=None picks them for such operands, and are treated as
    without `cast` elsewhere."""
    if route not in ROUTES:
        raise _lib.BackendError("grace_loss: route must be one of %s (got %r)" % (ROUTES, route))
    if cast is not None and cast not in _HIP16:
        raise _lib.BackendError("grace_loss: cast must be torch.float16 or torch.bfloat16 (got %r)" % (cast,))
    if route != "torch" and torch.is_tensor(z1) and torch.is_tensor(z2) and z1.dim() == 2 and z2.dim() == 2:
        as16 = cast if cast is not None and z1.dtype == torch.float32 else z1.dtype
        scores = z1.shape[0] * (z1.shape[0] + z2.shape[0])
        if (as16 in _HIP16 and z1.is_cuda and z2.device == z1.device and z2.dtype == z1.dtype and z1.shape[0] >= 1
                and z2.shape[1] == z1.shape[1] and 1 <= z1.shape[1] <= HIP_MAX_D and max(z1.shape[0], z2.shape[0]) < 2 ** 30
                and (route == "hip" or z1.shape[1] <= _TORCH_FASTER16_ABOVE_D
                     or not _TORCH_FASTER16[0] < scores < _TORCH_FASTER16[1])):
            return _grace_loss16(z1, z2, tau, as16)
    a = torch.nn.functional.normalize(z1, p=2, dim=-1)
    b = torch.nn.functional.normalize(z2, p=2, dim=-1)
    if route is None:
        served = (a.dim() == 2 and b.dim() == 2 and a.shape[0] >= 1 and b.is_cuda and b.dtype == a.dtype
                  and a.dtype == torch.float32 and _hip_served(a))
        scores = a.shape[0] * (a.shape[0] + b.shape[0]) if served else 0
        route = "hip" if served and not _TORCH_FASTER[0] < scores < _TORCH_FASTER[1] else "torch"
    skip = torch.arange(a.shape[0], device=a.device)  # (in range by construction: M <= M + N keys)
    lse = pair_lse(a, torch.cat([a, b]), tau, skip=skip, block=block, route=route, _skip_checked=True)
    return torch.mean(lse - (a * a).sum(1) / float(tau))
