"""Dense products over a ragged segmentation of the rows, and DiffPool's coarsening on them.

    segment_matmul_tn(s, panels, ptr, *, route=None, split=None) -> tuple of [B, K, F_p]          (autograd: s, every panel)
        s [N, K], panels: one to three [N, F_p] tensors (s itself may be one), ptr int64 [B + 1] on the operands' device,
        non-decreasing from 0 to N:      out_p[g] = s[ptr[g] : ptr[g + 1]]^T @ panels[p][ptr[g] : ptr[g + 1]]
    segment_matmul_nn(x, w, ptr, *, route=None) -> [N, Q]                                         (autograd: x, w)
        x [N, P], w [B, P, Q]:           out[i] = x[i] @ w[g(i)],  g(i) the segment that holds row i
    diffpool_coarsen(rowptr, colind, weight, s, embed, ptr) -> (h [B * K, F], adj_blocks [B, K, K], gram [B, K, K])
        h = S_g^T embed_g stacked, adj_blocks[g] = S_g^T (A S)_g, gram[g] = S_g^T S_g for the CSR matrix A (rowptr, colind int32,
        weight [E] or None): BatchedDiffPoolLayer.forward, cogdl/models/nn/diffpool.py:169-175, without the [N, B * K] mask, the
        [B * K, N] x [N, F] products that are zero outside one block per graph, and the [N, N] matrices of the link loss.
        One csrspmm and one three-panel segment_matmul_tn.

Each product is the other's gradient: d s = SUM_p nn(panels[p], d out_p^T), d panels[p] = nn(s, d out_p); d x = nn(d out, w^T),
d w = tn(x, d out).  route="hip" (float32 CUDA tensors): the MFMA kernels of csrc/segmm.hip -- ptr is never read on the host, no
float atomics, equal bytes from run to run; split= overrides the number of slices every segment's rows are cut into (tests).
route="torch": the segments padded to [B, n_max, .] and torch.bmm, differentiable by torch itself, for CPU and GPU tensors of
any floating dtype (one read-back of ptr) -- GPU tensors with one TorchRouteWarning, as operators/recon.py does.  route=None takes
the kernels wherever they serve.  BackendError before anything is launched: operands that are not 2-D (w: 3-D) floating tensors
of one dtype and device, panels whose row counts differ from s's, no panel or more than three, a ptr that is not int64 [B + 1]
on that device (B >= 1 for tn; w.shape[0] + 1 entries for nn), and route="hip" on anything but float32 CUDA tensors.
"""
import torch

from .. import _lib
from .ops import _ROUTE_NOTED, TorchRouteWarning

ROUTES = (None, "torch", "hip")
MAX_PANELS = 3


def _note_torch_route(op):
    if (op, "torch") in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add((op, "torch"))
    import warnings

    warnings.warn("cogdl_amd.operators.segmm.%s: GPU tensors on the torch route (route=\"hip\" runs the kernels of csrc/segmm.hip "
                  "on float32): padded segments on torch's bmm" % op, TorchRouteWarning, stacklevel=3)


def _tn_raw(s, panels, ptr, split=0):
    """The tn launch: s, panels contiguous float32 on one GPU -> a list of [B, K, F_p]."""
    (n, k), b = s.shape, ptr.numel() - 1
    widths = [p.shape[1] for p in panels] + [0] * (MAX_PANELS - len(panels))
    outs = [torch.empty((b, k, f), dtype=torch.float32, device=s.device) for f in widths[:len(panels)]]
    ws, ws_bytes = _lib.workspace("cogdl_hip_segment_matmul_workspace_bytes", s.device, n, b, k, *widths, split)
    pad = [None] * (MAX_PANELS - len(panels))
    with _lib.on_device(s.device):
        rc = _lib.hip().cogdl_hip_segment_matmul_tn(_lib.ptr(s), *[_lib.ptr(p) for p in list(panels) + pad], _lib.ptr(ptr), n, b, k,
                                                    *widths, split, *[_lib.ptr(o) for o in outs + pad], _lib.ptr(ws), ws_bytes,
                                                    _lib.stream_of(s))
    _lib.check(rc, "segment_matmul_tn")
    return outs


def _nn_raw(x, w, ptr, out=None):
    """The nn launch: x [N, P], w [B, P, Q] contiguous float32 on one GPU; out given: the product is added to it."""
    accumulate = out is not None
    if out is None:
        out = torch.empty((x.shape[0], w.shape[2]), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        rc = _lib.hip().cogdl_hip_segment_matmul_nn(_lib.ptr(x), _lib.ptr(w), _lib.ptr(ptr), x.shape[0], w.shape[0], x.shape[1],
                                                    w.shape[2], int(accumulate), _lib.ptr(out), _lib.stream_of(x))
    _lib.check(rc, "segment_matmul_nn")
    return out


class _HipTN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ptr, split, s, *panels):
        s, panels = s.contiguous(), tuple(p.contiguous() for p in panels)
        ctx.save_for_backward(ptr, s, *panels)
        return tuple(_tn_raw(s, panels, ptr, split))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        ptr, s, *panels = ctx.saved_tensors
        grads = [g.contiguous() for g in grads]
        g_s = None
        if ctx.needs_input_grad[2]:
            for x, g in zip(panels, grads):  # the terms sum in one buffer: no [N, K] temporaries
                g_s = _nn_raw(x, g.transpose(1, 2).contiguous(), ptr, out=g_s)
        g_panels = [_nn_raw(s, g, ptr) if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])]
        return (None, None, g_s) + tuple(g_panels)


class _HipNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ptr, x, w):
        x, w = x.contiguous(), w.contiguous()
        ctx.save_for_backward(ptr, x, w)
        return _nn_raw(x, w, ptr)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        ptr, x, w = ctx.saved_tensors
        grad = grad.contiguous()
        g_x = _nn_raw(grad, w.transpose(1, 2).contiguous(), ptr) if ctx.needs_input_grad[1] else None
        g_w = _tn_raw(x, (grad,), ptr)[0] if ctx.needs_input_grad[2] else None
        return None, g_x, g_w


def _padded(ptr, n):
    """-> (segment of every row, its position inside the segment, the longest segment): one read-back."""
    counts = ptr[1:] - ptr[:-1]
    seg = torch.repeat_interleave(torch.arange(counts.numel(), device=ptr.device), counts, output_size=n)
    pos = torch.arange(n, device=ptr.device) - ptr[:-1][seg]
    return seg, pos, int(counts.max()) if counts.numel() else 0


def _pad(t, seg, pos, b, n_max):
    return t.new_zeros((b, n_max, t.shape[1])).index_put((seg, pos), t)


def _torch_tn(s, panels, ptr):
    b = ptr.numel() - 1
    seg, pos, n_max = _padded(ptr, s.shape[0])
    st = _pad(s, seg, pos, b, n_max).transpose(1, 2)
    return tuple(torch.bmm(st, _pad(p, seg, pos, b, n_max)) for p in panels)


def _torch_nn(x, w, ptr):
    seg, pos, n_max = _padded(ptr, x.shape[0])
    return torch.bmm(_pad(x, seg, pos, w.shape[0], n_max), w)[seg, pos]


def _check(op, route, ptr, b, n, tensors):
    if route not in ROUTES:
        raise _lib.BackendError("%s: route must be one of %s (got %r)" % (op, ROUTES, route))
    first = tensors[0][1]
    for name, t, dim in tensors:
        if not torch.is_tensor(t) or t.dim() != dim or not t.is_floating_point():
            raise _lib.BackendError("%s: %s must be a %d-D floating tensor (got %s %s)"
                                    % (op, name, dim, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
        if t.dtype != first.dtype or t.device != first.device:
            raise _lib.BackendError("%s: %s is %s on %s, the first operand %s on %s" % (op, name, t.dtype, t.device, first.dtype, first.device))
        if dim == 2 and t.shape[0] != n:
            raise _lib.BackendError("%s: %s has %d rows, the first operand %d" % (op, name, t.shape[0], n))
    if not torch.is_tensor(ptr) or ptr.dtype != torch.int64 or ptr.dim() != 1 or ptr.device != first.device or (
            ptr.numel() != b + 1 if b is not None else ptr.numel() < 2):
        raise _lib.BackendError("%s: ptr must be an int64 tensor of %s entries on %s (got %s %s)"
                                % (op, "B + 1 >= 2" if b is None else b + 1, first.device, getattr(ptr, "dtype", type(ptr)),
                                   tuple(getattr(ptr, "shape", ()))))
    served = first.is_cuda and first.dtype == torch.float32
    if route == "hip" and not served:
        raise _lib.BackendError("%s: route=\"hip\" serves float32 CUDA tensors (got %s on %s); there is no fallback behind it"
                                % (op, first.dtype, first.device))
    if route is None:
        route = "hip" if served else "torch"
    if route == "torch" and first.is_cuda:
        _note_torch_route(op)
    return route


def segment_matmul_tn(s, panels, ptr, *, route=None, split=None):
    """s [N, K], panels (1 .. 3 tensors [N, F_p]), ptr int64 [B + 1] -> tuple of out_p [B, K, F_p] (module docstring)."""
    panels = tuple(panels)
    if not 1 <= len(panels) <= MAX_PANELS:
        raise _lib.BackendError("segment_matmul_tn: one to %d panels (got %d)" % (MAX_PANELS, len(panels)))
    n = s.shape[0] if torch.is_tensor(s) and s.dim() == 2 else -1
    route = _check("segment_matmul_tn", route, ptr, None, n,
                   [("s", s, 2)] + [("panels[%d]" % i, p, 2) for i, p in enumerate(panels)])
    if s.shape[1] < 1 or min(p.shape[1] for p in panels) < 1:
        raise _lib.BackendError("segment_matmul_tn: an operand without columns")
    if split is not None and not 1 <= int(split) <= 1024:
        raise _lib.BackendError("segment_matmul_tn: split must lie in 1 .. 1024 (got %r)" % (split,))
    if route == "hip":
        return _HipTN.apply(ptr.contiguous(), 0 if split is None else int(split), s, *panels)
    return _torch_tn(s, panels, ptr)


def segment_matmul_nn(x, w, ptr, *, route=None):
    """x [N, P], w [B, P, Q], ptr int64 [B + 1] -> out [N, Q], out[i] = x[i] @ w[segment of i] (module docstring)."""
    n = x.shape[0] if torch.is_tensor(x) and x.dim() == 2 else -1
    b = w.shape[0] if torch.is_tensor(w) and w.dim() == 3 else -1
    route = _check("segment_matmul_nn", route, ptr, b, n, [("x", x, 2), ("w", w, 3)])
    if w.shape[1] != x.shape[1] or x.shape[1] < 1 or w.shape[2] < 1:
        raise _lib.BackendError("segment_matmul_nn: x %s against w %s" % (tuple(x.shape), tuple(w.shape)))
    if route == "hip":
        return _HipNN.apply(ptr.contiguous(), x, w)
    return _torch_nn(x, w, ptr)


def diffpool_coarsen(rowptr, colind, weight, s, embed, ptr):
    """-> (h [B * K, F], adj_blocks [B, K, K], gram [B, K, K]) for the assignment s [N, K], the features embed [N, F] and the CSR
    matrix (rowptr, colind, weight) of the batch (module docstring).  Differentiable in s, embed and weight."""
    if s.is_cuda:
        from .spmm import csrspmm

        y = csrspmm(rowptr.int(), colind.int(), s, weight)
    else:
        row = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), (rowptr[1:] - rowptr[:-1]).long())
        msg = s[colind.long()]
        y = torch.zeros_like(s).index_add(0, row, msg if weight is None else msg * weight.unsqueeze(1))
    h, adj_blocks, gram = segment_matmul_tn(s, (embed, y, s), ptr)
    return h.reshape(-1, embed.shape[1]), adj_blocks, gram
