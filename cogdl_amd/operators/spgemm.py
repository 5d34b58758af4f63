"""spgemm: C = A . B of two sparse matrices on the GPU (csrc/spgemm.hip), with gradients for both value vectors, and
coalesce: arbitrary COO (unsorted, duplicates) -> canonical CSR with the duplicates summed.

The product of torch_sparse.spspmm, which the reference's srgcn / graph_unet / gtn models call
(models/nn/srgcn.py, models/nn/graph_unet.py, models/nn/gtn.py); cogdl_amd.torch_sparse_compat serves it under that name.
Strict like every GPU operator of this library: CUDA tensors, int32 CSR indices, float32 values, or BackendError.
The size of C depends on the data: a product reads nnz(C) back to the host once (twice when some row has more than 4096
products, include/cogdl_hip.h), so it cannot run inside a stream capture and says so instead of hanging.
"""
import torch

from .. import _lib
from ..plan import csr2csc

__all__ = ["spgemm", "coalesce"]

_ERANGE = 6  # COGDL_HIP_ERANGE
_I32_MAX = 2 ** 31 - 1
_SEGMENT_MAX_EDGES = 2 ** 31 - 2 ** 20  # COGDL_HIP_SEGMENT_MAX_EDGES


def _not_capturing(what):
    if torch.cuda.is_current_stream_capturing():
        raise _lib.BackendError("%s: the output size depends on the data (one device-to-host read); it cannot run inside a "
                                "stream capture" % what)


def _erange(what, detail):
    raise _lib.BackendError("%s failed: %s (%s)" % (what, _lib.hip().cogdl_hip_strerror(_ERANGE).decode(), detail))


def _i32(n, dev):
    return torch.empty(int(n), dtype=torch.int32, device=dev)


def _gather(perm, src):
    """out[i] = src[perm[i]] for 4-byte 1-D src of any length (cogdl_hip_gather_rows)."""
    out = torch.empty(perm.numel(), dtype=src.dtype, device=src.device)
    if perm.numel():
        rc = _lib.hip().cogdl_hip_gather_rows(_lib.ptr(perm), _lib.ptr(src), _lib.ptr(out), perm.numel(), 1, 4,
                                              _lib.stream_of(src))
        _lib.check(rc, "gather_rows")
    return out


def _sort_rows(rowptr, col, rows, cols):
    """Every row of a CSR stably sorted by column: two stable transposes.  -> (rowptr, col, order), order[t] = the input
    position now at t (equal columns keep their input order)."""
    t1 = csr2csc(rowptr, col, cols)
    t2 = csr2csc(t1.colptr, t1.rowind, rows)
    return t2.colptr, t2.rowind, _gather(t2.perm, t1.perm)


def _dupsum(rowptr, col, order, val, rows, want_map):
    """cogdl_hip_coo_dupsum -> (rowptr_u, col_u, val_u, map); col_u / val_u have room for nnz entries (the distinct
    count is rowptr_u[rows], on the device)."""
    dev = col.device
    nnz = col.numel()
    rowptr_u, col_u = _i32(rows + 1, dev), _i32(nnz, dev)
    val_u = None if val is None else torch.empty(nnz, dtype=torch.float32, device=dev)
    mp = _i32(nnz, dev) if want_map else None
    ws, ws_bytes = _lib.workspace("cogdl_hip_coo_dupsum_workspace_bytes", dev, nnz)
    rc = _lib.hip().cogdl_hip_coo_dupsum(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(order), _lib.ptr(val), rows, nnz,
                                         _lib.ptr(rowptr_u), _lib.ptr(col_u), _lib.ptr(val_u), _lib.ptr(mp), _lib.ptr(ws),
                                         ws_bytes, _lib.stream_of(col))
    _lib.check(rc, "coo_dupsum")
    return rowptr_u, col_u, val_u, mp


def _forward(rA, cA, vA, rB, cB, vB, m, k, n):
    dev = vA.device
    lib = _lib.hip()
    stream = _lib.stream_of(vA)
    plan = torch.empty(lib.cogdl_hip_spgemm_plan_bytes(m), dtype=torch.uint8, device=dev)
    rowptrC = _i32(m + 1, dev)
    ws, ws_bytes = _lib.workspace("cogdl_hip_spgemm_count_workspace_bytes", dev, m)
    _lib.check(lib.cogdl_hip_spgemm_count(_lib.ptr(rA), _lib.ptr(cA), _lib.ptr(rB), _lib.ptr(cB), m, k, n, _lib.ptr(plan),
                                          _lib.ptr(rowptrC), _lib.ptr(ws), ws_bytes, stream), "spgemm_count")
    hdr = plan[:64].view(torch.int64).tolist()  # the synchronisation: bin sizes, hub products, nnz(C)
    n_hub, hub_products, nnz_c = hdr[3], hdr[4], hdr[5]
    hub = (None, None, None)
    if n_hub:
        if hub_products > _SEGMENT_MAX_EDGES:
            _erange("spgemm", "%d products in rows beyond the LDS path" % hub_products)
        hub_rowptr, hub_col = _i32(n_hub + 1, dev), _i32(hub_products, dev)
        hub_val = torch.empty(hub_products, dtype=torch.float32, device=dev)
        ws2, ws2_bytes = _lib.workspace("cogdl_hip_spgemm_expand_workspace_bytes", dev, n_hub)
        _lib.check(lib.cogdl_hip_spgemm_expand(_lib.ptr(rA), _lib.ptr(cA), _lib.ptr(vA), _lib.ptr(rB), _lib.ptr(cB), _lib.ptr(vB),
                                               m, _lib.ptr(plan), n_hub, hub_products, _lib.ptr(hub_rowptr), _lib.ptr(hub_col),
                                               _lib.ptr(hub_val), _lib.ptr(ws2), ws2_bytes, stream), "spgemm_expand")
        srt_rowptr, srt_col, order = _sort_rows(hub_rowptr, hub_col, n_hub, n)
        hub = _dupsum(srt_rowptr, srt_col, order, hub_val, n_hub, False)[:3]
        _lib.check(lib.cogdl_hip_spgemm_rowptr(_lib.ptr(plan), m, n_hub, _lib.ptr(hub[0]), _lib.ptr(rowptrC), _lib.ptr(ws),
                                               ws_bytes, stream), "spgemm_rowptr")
        nnz_c = int(plan[40:48].view(torch.int64).item())  # (second synchronisation: the hub rows' distinct columns)
    if nnz_c > _I32_MAX:
        _erange("spgemm", "nnz(C) = %d" % nnz_c)
    colC = _i32(nnz_c, dev)
    valC = torch.empty(nnz_c, dtype=torch.float32, device=dev)
    _lib.check(lib.cogdl_hip_spgemm_fill(_lib.ptr(rA), _lib.ptr(cA), _lib.ptr(vA), _lib.ptr(rB), _lib.ptr(cB), _lib.ptr(vB), m, k, n,
                                         _lib.ptr(plan), _lib.ptr(rowptrC), nnz_c, _lib.ptr(colC), _lib.ptr(valC), n_hub,
                                         _lib.ptr(hub[0]), _lib.ptr(hub[1]), _lib.ptr(hub[2]), stream), "spgemm_fill")
    return rowptrC, colC, valC


class _SpGEMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vA, vB, rA, cA, rB, cB, m, k, n):
        with _lib.on_device(vA.device):
            rC, cC, vC = _forward(rA, cA, vA, rB, cB, vB, m, k, n)
        ctx.save_for_backward(rA, cA, vA, rB, cB, vB, rC, cC)
        ctx.dims = (m, k, n)
        ctx.mark_non_differentiable(rC, cC)
        return rC, cC, vC

    @staticmethod
    def backward(ctx, _g_rowptr, _g_col, g):
        rA, cA, vA, rB, cB, vB, rC, cC = ctx.saved_tensors
        m, k, _ = ctx.dims
        lib = _lib.hip()
        if cC.numel() == 0:
            # C has no entry (an empty operand, or A's columns meet only empty rows of B): both gradients are zero, and
            # the empty colC / g (and an empty operand's arrays) have no address for the entry points, which refuse NULL
            return (torch.zeros_like(vA) if ctx.needs_input_grad[0] else None,
                    torch.zeros_like(vB) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None, None)
        g = g.contiguous()
        stream = _lib.stream_of(g)
        gA = gB = None
        with _lib.on_device(g.device):
            if ctx.needs_input_grad[0]:
                gA = torch.empty_like(vA)
                _lib.check(lib.cogdl_hip_spgemm_grad_a(_lib.ptr(rA), _lib.ptr(cA), _lib.ptr(rB), _lib.ptr(cB), _lib.ptr(vB),
                                                       _lib.ptr(rC), _lib.ptr(cC), _lib.ptr(g), _lib.ptr(gA), m, cA.numel(),
                                                       stream), "spgemm_grad_a")
            if ctx.needs_input_grad[1]:
                gB = torch.empty_like(vB)
                at = csr2csc(rA, cA, k)  # column k of A = row k of its stable transpose
                _lib.check(lib.cogdl_hip_spgemm_grad_b(_lib.ptr(at.colptr), _lib.ptr(at.rowind), _lib.ptr(at.perm), _lib.ptr(vA),
                                                       _lib.ptr(rB), _lib.ptr(cB), _lib.ptr(rC), _lib.ptr(cC), _lib.ptr(g),
                                                       _lib.ptr(gB), k, cB.numel(), stream), "spgemm_grad_b")
        return gA, gB, None, None, None, None, None, None, None


def _check_csr(rowptr, col, val, what):
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32:
        raise _lib.BackendError("spgemm: %s's rowptr / col must be int32 (got %s / %s)" % (what, rowptr.dtype, col.dtype))
    if val.dtype != torch.float32:
        raise _lib.BackendError("spgemm: %s's values must be float32 (got %s); the HIP path has no other dtype" % (what, val.dtype))
    if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or val.shape != col.shape:
        raise _lib.BackendError("spgemm: %s must be a CSR (rowptr [rows+1], col [nnz], val [nnz]); got shapes %s %s %s"
                                % (what, tuple(rowptr.shape), tuple(col.shape), tuple(val.shape)))
    return rowptr.contiguous(), col.contiguous(), val.contiguous()


def spgemm(rowptrA, colA, valA, rowptrB, colB, valB, n):
    """C = A . B with A [m, k] and B [k, n] in int32 CSR (m = rowptrA.numel() - 1, k = rowptrB.numel() - 1; column ids
    of A below k, of B below n) -> (rowptrC int32 [m+1], colC int32, valC float32): canonical CSR (columns ascending and
    unique per row) with the STRUCTURAL pattern -- an entry whose products cancel is kept as 0.0, as torch.sparse.mm
    keeps it.  A and B need not be canonical.  Differentiable in valA and valB (a product without any entry gives zero
    gradients of the operands' shapes).  Bit-identical results on every call.
    Limits (BackendError with COGDL_HIP_ERANGE): m, k, n and nnz(C) below 2^31, and the rows with more than 4096 products
    (the global-memory path) at most COGDL_HIP_SEGMENT_MAX_EDGES = 2^31 - 2^20 products in all.
    Both CSRs are validated first (rowptr starts at 0, never decreases, ends at nnz; column ids in range): one more
    device-to-host read, so that a malformed index is an error here instead of an out-of-bounds read on the device."""
    _lib.require_cuda(rowptrA, colA, valA, rowptrB, colB, valB)
    rA, cA, vA = _check_csr(rowptrA, colA, valA, "A")
    rB, cB, vB = _check_csr(rowptrB, colB, valB, "B")
    m, k, n = rA.numel() - 1, rB.numel() - 1, int(n)
    if n < 0:
        raise _lib.BackendError("spgemm: n must be >= 0")
    if max(m, k, n) > _I32_MAX:
        _erange("spgemm", "m, k, n = %d, %d, %d" % (m, k, n))
    _not_capturing("spgemm")
    _validate(rA, cA, k, "A")
    _validate(rB, cB, n, "B")
    return _SpGEMM.apply(vA, vB, rA, cA, rB, cB, m, k, n)


def _spgemm_trusted(rA, cA, vA, rB, cB, vB, m, k, n):
    """spgemm on CSRs that coalesce() has just built (canonical and in range): no validation read."""
    _not_capturing("spgemm")
    return _SpGEMM.apply(vA, vB, rA, cA, rB, cB, m, k, n)


def _validate(rowptr, col, n_cols, what):
    bad = (rowptr[0] != 0) | (rowptr[-1] != col.numel())
    if rowptr.numel() > 1:
        bad = bad | (rowptr[1:] < rowptr[:-1]).any()
    if col.numel():
        bad = bad | (col.min() < 0) | (col.max() >= n_cols)
    if bool(bad):
        raise _lib.BackendError("spgemm: %s is not a CSR with column ids in [0, %d) (rowptr must start at 0, never decrease "
                                "and end at col.numel())" % (what, n_cols))


class _Coalesce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, rowptr, col, order, rows):
        rowptr_u, col_u, val_u, mp = _dupsum(rowptr, col, order, val, rows, True)
        u = int(rowptr_u[-1].item())  # (the distinct count: a device-to-host read, the size of the outputs)
        col_u, val_u = col_u[:u].clone(), val_u[:u].clone()
        ctx.save_for_backward(mp)
        ctx.mark_non_differentiable(rowptr_u, col_u, mp)
        return rowptr_u, col_u, val_u, mp

    @staticmethod
    def backward(ctx, _g_rowptr, _g_col, g, _g_map):
        (mp,) = ctx.saved_tensors
        return _gather(mp, g.contiguous()), None, None, None, None


def coalesce(row, col, val, m, n, return_map=False):
    """COO [m, n] (row / col int64 or int32, val float32; any order, duplicates allowed) -> canonical CSR (rowptr int32
    [m+1], col int32, val float32) with the duplicates summed in input order; differentiable in val.  return_map=True
    also returns map (int32 [nnz]): the canonical position of every input entry."""
    _lib.require_cuda(row, col, val)
    if val.dtype != torch.float32:
        raise _lib.BackendError("coalesce: values must be float32 (got %s)" % val.dtype)
    if row.dim() != 1 or row.shape != col.shape or col.shape != val.shape:
        raise _lib.BackendError("coalesce: row, col, val must be 1-D of one length")
    m, n, nnz = int(m), int(n), row.numel()
    if m < 0 or n < 0:
        raise _lib.BackendError("coalesce: m and n must be >= 0")
    if max(m, n) > _I32_MAX or nnz > _SEGMENT_MAX_EDGES:
        _erange("coalesce", "m, n, nnz = %d, %d, %d" % (m, n, nnz))
    _not_capturing("coalesce")
    dev = val.device
    if nnz:
        lo = torch.stack([row.min(), col.min()]).tolist()
        hi = torch.stack([row.max(), col.max()]).tolist()
        if min(lo) < 0 or hi[0] >= m or hi[1] >= n:
            raise _lib.BackendError("coalesce: an index lies outside [0, %d) x [0, %d)" % (m, n))
    with _lib.on_device(dev):
        row32, col32 = row.to(torch.int32).contiguous(), col.to(torch.int32).contiguous()
        # first pass: the entries as ONE row, stably transposed = sorted by column; second: back, sorted by row
        one = torch.tensor([0, nnz], dtype=torch.int32, device=dev)
        t1 = csr2csc(one, col32, n)
        t2 = csr2csc(t1.colptr, _gather(t1.perm, row32), m)
        order = _gather(t2.perm, t1.perm)
        rowptr_u, col_u, val_u, mp = _Coalesce.apply(val.contiguous(), t2.colptr, t2.rowind, order, m)
    return (rowptr_u, col_u, val_u, mp) if return_map else (rowptr_u, col_u, val_u)

