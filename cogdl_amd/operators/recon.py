"""The inner-product decoder loss of the graph auto-encoders, without an [N, N] matrix.

    inner_product_bce(z, row, col, weight=None, *, route=None, block=None, split=None) -> scalar         (autograd: z)
        z [N, d]; row, col int32 / int64 [E] with entries in [0, N); weight None (ones) or floating [E], not differentiable
            loss = SUM_ij softplus(<z_i, z_j>) - SUM_e weight[e] <z_row[e], z_col[e]>       all ordered pairs, diagonal included

The reference writes F.binary_cross_entropy(torch.sigmoid(torch.mm(z, z.t())), adj, reduction="sum") against a dense adjacency
(VGAE.make_loss, cogdl/models/nn/gae.py:76-84; DAEGC.recon_loss, cogdl/models/nn/daegc.py:82-84): four or five [N, N] float32
tensors.  For a sigmoid link -a log sigmoid(s) - (1 - a) log(1 - sigmoid(s)) = softplus(s) - a s, so the sum over all pairs
splits into a dense term that needs no adjacency and a term over the edges; with A = sparse_coo_tensor((row, col),
weight).to_dense() -- duplicated edges add up, a self loop counts once -- this is the same number, up to two things.  torch's
BCE clamps each log at -100, and in float32 1 - sigmoid(s) is 0 from about s > 17, so the reference charges 100 for such a
pair where the formula gives s: the operator follows the formula.  And the sums are taken in another order.  The gradient is

    grad_z = 2 g sigmoid(Z Z^T) Z - g (A + A^T) Z

Two routes compute it.  route="hip" (float32 CUDA tensors, 1 <= d <= 256): the kernels of csrc/recon.hip -- 64 x 64 score tiles
from v_mfma_f32_32x32x2_f32, the forward over the tiles on and above the diagonal only, double partial sums folded in index
order; the backward recomputes the scores and chains a second MFMA for sigmoid(S) Z; the edge term is per-edge dots forward and
two CSR gathers backward (the edges sorted by row and by column with torch.sort).  It keeps z and the sorted edges, allocates
nothing of size [N, N], [E, d] or block x N, uses no float atomics and returns equal bytes from run to run.  split= overrides
the number of slices a row tile's walk is cut into (tests).  route="torch": the same formula as a torch composition in row
blocks of `block` rows (by default as many as keep one block x N tensor near 64 MB), forward and backward, the edges in chunks;
it keeps z and the edges only, and takes CPU and GPU tensors of any floating dtype -- GPU tensors with one TorchRouteWarning, as
operators/contrast.py does.  route=None takes the kernels wherever they serve and the composition elsewhere.  Every route
raises BackendError before anything is launched for a z that is not a 2-D floating tensor, index tensors of another shape,
dtype or device, and endpoints outside [0, N) (one read-back).  N == 0 and E == 0 are legal.
"""
import torch

from .. import _lib
from .ops import _ROUTE_NOTED, TorchRouteWarning

ROUTES = (None, "torch", "hip")
HIP_MAX_D = 256  # the widest rows csrc/recon.hip keeps in LDS
_BLOCK_BYTES = 64 << 20
_EDGE_CHUNK = 1 << 18


def _note_torch_route(why):
    if ("inner_product_bce", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("inner_product_bce", why))
    import warnings

    warnings.warn("cogdl_amd.operators.recon.inner_product_bce: GPU tensors on the torch route (%s): the blocked composition on "
                  "torch's kernels" % why, TorchRouteWarning, stacklevel=3)


def slices(n, d, which):
    """The slices csrc/recon.hip cuts a row tile's walk into: which = "fwd" or "grad"."""
    return int(_lib.hip().cogdl_hip_recon_bce_slices(int(n), int(d), ("fwd", "grad").index(which)))


def _hip_served(z):
    return z.is_cuda and z.dtype == torch.float32 and 1 <= z.shape[1] <= HIP_MAX_D


class _BlockedRecon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, row, col, weight, block):
        n = z.shape[0]
        loss = z.new_zeros(())
        for r0 in range(0, n, block):
            loss += torch.nn.functional.softplus(torch.matmul(z[r0:r0 + block], z.t())).sum()
        for e0 in range(0, row.numel(), _EDGE_CHUNK):
            r, c = row[e0:e0 + _EDGE_CHUNK], col[e0:e0 + _EDGE_CHUNK]
            dots = (z[r] * z[c]).sum(1)
            loss -= (dots if weight is None else dots * weight[e0:e0 + _EDGE_CHUNK]).sum()
        ctx.block = block
        ctx.save_for_backward(z, row, col, weight)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        z, row, col, weight = ctx.saved_tensors
        g_z = torch.empty_like(z)
        for r0 in range(0, z.shape[0], ctx.block):
            g_z[r0:r0 + ctx.block] = torch.matmul(torch.sigmoid(torch.matmul(z[r0:r0 + ctx.block], z.t())), z)
        g_z *= 2 * grad
        for e0 in range(0, row.numel(), _EDGE_CHUNK):
            r, c = row[e0:e0 + _EDGE_CHUNK], col[e0:e0 + _EDGE_CHUNK]
            w = grad if weight is None else grad * weight[e0:e0 + _EDGE_CHUNK]
            g_z.index_add_(0, r, -(z[c] * w.reshape(-1, 1)))
            g_z.index_add_(0, c, -(z[r] * w.reshape(-1, 1)))
        return g_z, None, None, None, None


def _csr(key, other, weight, n):
    """The edges sorted by `key` (stable): int32 pointer [n + 1], the other endpoint and the weight in that order."""
    order = torch.sort(key, stable=True)[1]
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=key.device)
    ptr[1:] = torch.cumsum(torch.bincount(key, minlength=n), 0)
    return ptr, other[order].to(torch.int32), None if weight is None else weight[order].contiguous()


class _HipRecon(torch.autograd.Function):
    """The kernels of csrc/recon.hip.  Keeps z, the int32 edges and the weight, and nothing else."""

    @staticmethod
    def forward(ctx, z, row, col, weight, split):
        (n, d), e = z.shape, row.numel()
        dev = z.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        n_slices = slices(n, d, "fwd") if split is None else split
        ws, ws_bytes = _lib.workspace("cogdl_hip_recon_bce_workspace_bytes", dev, n, d, e, n_slices, 0)
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_recon_bce_fwd(_lib.ptr(z), _lib.ptr(row) if e else None, _lib.ptr(col) if e else None,
                                                    _lib.ptr(weight) if e else None, n, d, e, n_slices, _lib.ptr(loss),
                                                    _lib.ptr(ws), ws_bytes, _lib.stream_of(z))
        _lib.check(rc, "recon_bce_fwd")
        ctx.split = split
        ctx.save_for_backward(z, row, col, weight)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        z, row, col, weight = ctx.saved_tensors
        n, d = z.shape
        dev = z.device
        grad = grad.to(torch.float32).contiguous()
        g_z = torch.empty_like(z)
        a = t = (None, None, None)
        if row.numel():
            row64, col64 = row.long(), col.long()
            a, t = _csr(row64, col64, weight, n), _csr(col64, row64, weight, n)
        n_slices = slices(n, d, "grad") if ctx.split is None else ctx.split
        ws, ws_bytes = _lib.workspace("cogdl_hip_recon_bce_workspace_bytes", dev, n, d, 0, n_slices, 1)
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_recon_bce_grad(_lib.ptr(z), _lib.ptr(grad), _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]),
                                                     _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), n, d, n_slices,
                                                     _lib.ptr(g_z), _lib.ptr(ws), ws_bytes, _lib.stream_of(z))
        _lib.check(rc, "recon_bce_grad")
        return g_z, None, None, None, None


def inner_product_bce(z, row, col, weight=None, *, route=None, block=None, split=None):
    """z [N, d], edges (row[e], col[e]) with optional weight[e] -> the scalar loss in the dtype of z (module docstring).
    route: None -- the kernels where they serve, the composition elsewhere; "torch" -- the blocked composition (block: its rows
    per step); "hip" -- the kernels of csrc/recon.hip (split: their slice count, for tests).  BackendError for a z that is not a
    2-D floating tensor, for row / col / weight of another shape, dtype or device, for endpoints outside [0, N), an unknown
    route, and for route="hip" on what the kernels do not serve: CPU tensors, a dtype other than float32, d outside 1 .. 256."""
    if route not in ROUTES:
        raise _lib.BackendError("inner_product_bce: route must be one of %s (got %r)" % (ROUTES, route))
    if not torch.is_tensor(z) or z.dim() != 2 or not z.is_floating_point():
        raise _lib.BackendError("inner_product_bce: z must be a 2-D floating tensor (got %s %s)"
                                % (getattr(z, "dtype", type(z)), tuple(getattr(z, "shape", ()))))
    n, d = z.shape
    for name, idx in (("row", row), ("col", col)):
        if not torch.is_tensor(idx) or idx.dim() != 1 or idx.dtype not in (torch.int32, torch.int64):
            raise _lib.BackendError("inner_product_bce: %s must be a 1-D int32 or int64 tensor" % name)
    if row.shape != col.shape:
        raise _lib.BackendError("inner_product_bce: row and col of %d and %d edges" % (row.numel(), col.numel()))
    e = row.numel()
    if weight is not None and (not torch.is_tensor(weight) or not weight.is_floating_point() or tuple(weight.shape) != (e,)):
        raise _lib.BackendError("inner_product_bce: weight must be None or a floating tensor of shape [%d]" % e)
    tensors = [z, row, col] + ([] if weight is None else [weight])
    if len({t.device for t in tensors}) != 1:
        raise _lib.BackendError("inner_product_bce: tensors on %s" % sorted({str(t.device) for t in tensors}))
    if e:
        lo, hi = min(int(row.min()), int(col.min())), max(int(row.max()), int(col.max()))
        if lo < 0 or hi >= n:
            raise _lib.BackendError("inner_product_bce: edge endpoints must lie in [0, %d) (got %d .. %d)" % (n, lo, hi))
    if route == "hip":
        if not _hip_served(z):
            raise _lib.BackendError("inner_product_bce: route=\"hip\" serves float32 CUDA tensors with 1 <= d <= %d (got %s on %s, "
                                    "d = %d); there is no fallback behind it" % (HIP_MAX_D, z.dtype, z.device, d))
        if split is not None and int(split) < 1:
            raise _lib.BackendError("inner_product_bce: split must be at least 1 (got %r)" % (split,))
    if route is None:
        route = "hip" if _hip_served(z) else "torch"
    if route == "hip" and max(n, e) >= 2 ** 31 - 1:
        raise _lib.BackendError("inner_product_bce: sizes beyond int32 indexing")
    if weight is not None:
        weight = weight.detach().to(z.dtype)
    if route == "hip":
        return _HipRecon.apply(z.contiguous(), row.to(torch.int32).contiguous(), col.to(torch.int32).contiguous(),
                               None if weight is None else weight.contiguous(), None if split is None else int(split))
    if z.is_cuda:
        _note_torch_route("route=\"hip\" runs the kernels of csrc/recon.hip on float32 rows of up to %d columns" % HIP_MAX_D)
    if block is None:
        block = _BLOCK_BYTES // (max(n, 1) * z.element_size())
    return _BlockedRecon.apply(z, row.long(), col.long(), weight, max(1, min(int(block), max(n, 1))))
