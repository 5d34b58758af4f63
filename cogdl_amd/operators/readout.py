"""Batched graph readout: the step that turns the node rows x [N, F] of a mini-batch of graphs into graph rows.

    segment_ptr(batch)              the sorted int64 `batch` vector -> (ptr int32 [B + 1], B): graph g owns rows [ptr[g], ptr[g + 1])
    segment_pool(x, ptr, mode)      "sum" / "mean" / "max" over each range -> [B, F]          (autograd)
    sort_pool(x, ptr, k, key_col)   per graph the k rows with the largest x[:, key_col], descending, equal keys in row
                                    order -> (out [B, k, F] zero-padded, idx int32 [B, k] with -1 on padding)   (autograd)

CUDA tensors go to the HIP kernels (csrc/readout.hip), CPU tensors to the host twin in libcogdl_host.so (OpenMP over the
graphs; libcogdl_hip.so is not loaded).  Both follow csrc/readout_law.h and return the same bytes; there are no atomics, so
the result is also the same from run to run.  A segment of up to `exact_nodes()` rows is summed in row order from +0.0f:
bit for bit what the reference's zeros + scatter_add_ gives on the CPU (cogdl/utils/utils.py:192-203, models/nn/gin.py:111).
With `ptr` in hand neither operator reads anything back, so both run inside torch.cuda.graph capture; segment_ptr reads the
last id (as the reference does to size its output) and the validity flag.  float32 only: anything else raises BackendError
-- what to do about it is the caller's decision (cogdl_amd/readout_compat.py delegates to the reference).
"""
import torch

from .. import _lib

MODES = {"sum": 0, "mean": 1, "max": 2}


def exact_nodes():
    """Segments of up to this many rows are summed strictly in row order (longer ones in a fixed chunked order)."""
    return _lib.host().cogdl_host_segment_exact_nodes()


def _device(name, *tensors):
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise _lib.BackendError("%s: tensors on different devices: %s vs %s" % (name, dev, t.device))
    if dev.type not in ("cuda", "cpu"):
        raise _lib.BackendError("%s: no implementation for device %s" % (name, dev))
    return dev


def _checked(name, x, ptr):
    if x.dtype != torch.float32:
        raise _lib.BackendError("%s: x must be float32 (got %s)" % (name, x.dtype))
    if x.dim() != 2 or x.shape[1] < 1:
        raise _lib.BackendError("%s: x must be [N, F] with F >= 1 (got shape %s)" % (name, tuple(x.shape)))
    if ptr.dtype != torch.int32 or ptr.dim() != 1 or ptr.numel() < 1:
        raise _lib.BackendError("%s: ptr must be int32 [B + 1] (got %s %s)" % (name, ptr.dtype, tuple(ptr.shape)))
    return _device(name, x, ptr), x.contiguous(), ptr.contiguous()


def _call(dev, name, what, hip_args, host_args, ref):
    if dev.type == "cuda":
        with _lib.on_device(dev):
            rc = getattr(_lib.hip(), "cogdl_hip_" + name)(*hip_args, _lib.stream_of(ref))
        _lib.check(rc, what)
    else:
        _lib.check_host(getattr(_lib.host(), "cogdl_host_" + name)(*host_args), what)


def segment_ptr(batch, num_graphs=None):
    """-> (ptr, B).  `batch` int64 [N], non-decreasing, ids in [0, B); B = batch[-1] + 1 unless num_graphs gives it (ids that
    do not occur get empty segments).  BackendError for a batch that is unsorted or holds an id outside [0, B)."""
    if batch.dtype != torch.int64 or batch.dim() != 1:
        raise _lib.BackendError("segment_ptr: batch must be int64 [N] (got %s %s)" % (batch.dtype, tuple(batch.shape)))
    dev, batch, n = _device("segment_ptr", batch), batch.contiguous(), batch.numel()
    b = int(num_graphs) if num_graphs is not None else (int(batch[-1]) + 1 if n else 0)
    if b < 0 or (n and b < 1):
        raise _lib.BackendError("segment_ptr: graph ids must lie in [0, B) (last id %d)" % (b - 1))
    if n == 0:
        return torch.zeros(b + 1, dtype=torch.int32, device=dev), b
    ptr = torch.empty(b + 1, dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    args = (_lib.ptr(batch), n, b, _lib.ptr(ptr), _lib.ptr(flag))
    _call(dev, "segment_ptr", "segment_ptr", args, args, batch)
    if int(flag):
        raise _lib.BackendError("segment_ptr: batch is not non-decreasing with ids in [0, %d)" % b)
    return ptr, b


class _SegmentPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr, mode):
        dev, x, ptr = _checked("segment_pool", x, ptr)
        (n, f), b = x.shape, ptr.numel() - 1
        # (nothing is launched for n == 0 or b == 0: the answer for empty segments stands)
        launches = n > 0 and b > 0
        out = (torch.empty if launches else torch.zeros)((b, f), dtype=torch.float32, device=dev)
        argmax = None
        if mode == MODES["max"]:
            argmax = torch.empty((b, f), dtype=torch.int32, device=dev) if launches else torch.full(
                (b, f), -1, dtype=torch.int32, device=dev)
        args = (_lib.ptr(x), _lib.ptr(ptr), n, b, f, mode, _lib.ptr(out), _lib.ptr(argmax))
        _call(dev, "segment_pool_fwd", "segment_pool", args, args, x)
        ctx.mode, ctx.n = mode, n
        ctx.save_for_backward(ptr, argmax)
        return out

    @staticmethod
    def backward(ctx, grad):
        ptr, argmax = ctx.saved_tensors
        (b, f), n, dev = grad.shape, ctx.n, grad.device
        grad = grad.contiguous()
        if grad.dtype != torch.float32:
            raise _lib.BackendError("segment_pool backward: grad must be float32 (got %s)" % grad.dtype)
        grad_x = torch.empty((n, f), dtype=torch.float32, device=dev)
        args = (_lib.ptr(grad), _lib.ptr(ptr), None, _lib.ptr(argmax), n, b, f, ctx.mode, _lib.ptr(grad_x))
        _call(dev, "segment_pool_bwd", "segment_pool backward", args, args, grad)
        return grad_x, None, None


def segment_pool(x, ptr, mode):
    """x float32 [N, F], ptr int32 [B + 1] on the same device -> [B, F].  An empty segment gives 0."""
    if mode not in MODES:
        raise ValueError("segment_pool: mode must be one of %s (got %r)" % (sorted(MODES), mode))
    return _SegmentPool.apply(x, ptr, MODES[mode])


class _SortPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr, k, key_col):
        dev, x, ptr = _checked("sort_pool", x, ptr)
        (n, f), b = x.shape, ptr.numel() - 1
        out = torch.empty((b, k, f), dtype=torch.float32, device=dev)
        idx = torch.empty((b, k), dtype=torch.int32, device=dev)
        host_args = (_lib.ptr(x), _lib.ptr(ptr), n, b, f, k, key_col, _lib.ptr(out), _lib.ptr(idx))
        ws, ws_bytes = None, 0
        if dev.type == "cuda":
            ws, ws_bytes = _lib.workspace("cogdl_hip_sort_pool_workspace_bytes", dev, n)
        _call(dev, "sort_pool_fwd", "sort_pool", host_args + (_lib.ptr(ws), ws_bytes), host_args, x)
        ctx.n = n
        ctx.save_for_backward(idx)
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, grad, _grad_idx):
        (idx,) = ctx.saved_tensors
        (b, k, f), n, dev = grad.shape, ctx.n, grad.device
        grad = grad.contiguous()
        if grad.dtype != torch.float32:
            raise _lib.BackendError("sort_pool backward: grad must be float32 (got %s)" % grad.dtype)
        grad_x = torch.empty((n, f), dtype=torch.float32, device=dev)
        args = (_lib.ptr(grad), _lib.ptr(idx), n, b, f, k, _lib.ptr(grad_x))
        _call(dev, "sort_pool_bwd", "sort_pool backward", args, args, grad)
        return grad_x, None, None, None


def sort_pool(x, ptr, k, key_col=-1):
    """-> (out float32 [B, k, F], idx int32 [B, k]): per graph its min(k, n_g) rows with the largest x[:, key_col] in
    descending key order, equal keys in increasing row order; rows past n_g are zero and idx is -1 there."""
    k, key_col = int(k), int(key_col)
    if k < 1:
        raise ValueError("sort_pool: k must be at least 1 (got %r)" % (k,))
    f = x.shape[1] if x.dim() == 2 else 0
    if key_col < 0:
        key_col += f
    if f and not 0 <= key_col < f:
        raise ValueError("sort_pool: key_col outside [0, %d)" % f)
    return _SortPool.apply(x, ptr, k, key_col)
