"""Message passing of a relational GCN layer: every edge (row <- col) carries a type, and its message is the source row times
that type's MATRIX,

    h[v] = sum over the edges e with row[e] == v of  weight[e] * x[col[e]] @ W[etype[e]]

in the two regularisations of the paper (and of cogdl/layers/rgcn_layer.py):

    rgcn_basis_aggregate(x, alpha, row, col, etype, weight=None, num_nodes=None, num_types=None) -> Z [num_nodes, B, in]
        Z[v, b, :] = sum_{e: row[e] == v}  weight[e] * alpha[etype[e], b] * x[col[e], :]                    (autograd: x, alpha)
        W[t] = sum_b alpha[t, b] V[b], so the layer is  Z.view(N, B * in) @ V.view(B * in, out):  one dense matmul behind the
        sparse sum.  alpha=None is the identity (one basis per type; num_types then names R, else it is read from etype).

    rgcn_bdd_aggregate(x, W, row, col, etype, weight=None, num_nodes=None) -> H [num_nodes, B * bo]
        W [R, B, bi, bo] block diagonal, x [N, B * bi]                                                      (autograd: x, W)
        H[v, b*bo:(b+1)*bo] = sum_{e: row[e] == v}  weight[e] * x[col[e], b*bi:(b+1)*bi] @ W[etype[e], b]

fp32 GPU tensors go to the HIP kernels of csrc/rgcn.hip: nothing of size [E, .] is written, nothing scales with R * N, no float
atomics, so results are equal from run to run.  The edge views are the memoised plans of operators/ops.py (`edge_plan`):
destination-, source- and type-sorted for basis; for bdd the destination and source views are taken over the type-sorted
order, so that inside a row the edges of one type are adjacent and a run of one type is summed before it is multiplied.
Building the type plan is the range check of `etype`, the source plan that of `col`, the destination plan that of `row`.

CPU tensors run the plain torch composition of the two laws.  A GPU call the kernels do not cover (other dtypes, a weight
that requires grad, E == 0, zero widths, B > 32 for basis, in or out > 512 or bi * bo > 4096 for bdd) runs the same composition
and says so once per reason with a TorchRouteWarning, as operators/ops.py does.
"""
import torch

from .. import _lib
from .ops import _ROUTE_NOTED, TorchRouteWarning, edge_plan
from .relational import _aux, _is_index

MAX_BASES = 32        # cogdl_hip_rgcn_basis_*: beyond, COGDL_HIP_EUNSUPPORTED
MAX_BDD_WIDTH = 512   # cogdl_hip_rgcn_bdd_*: in, out
MAX_BDD_BLOCK = 4096  # bi * bo


def _note_torch_route(op, why):
    if (op, why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add((op, why))
    import warnings

    warnings.warn("cogdl_amd.operators.rgcn.%s: GPU tensors on the torch composition (%s); the HIP kernels cover float32 "
                  "tensors with 1-D int64 row, col and etype and a weight outside autograd, basis with at most %d bases, bdd "
                  "with in, out <= %d and bi * bo <= %d" % (op, why, MAX_BASES, MAX_BDD_WIDTH, MAX_BDD_BLOCK),
                  TorchRouteWarning, stacklevel=3)


# ----------------------------------------------------------------------------------------------------------- torch compositions
def _basis_composition(x, alpha, row, col, etype, weight, num_nodes, num_types):
    if alpha is None:  # the identity: edge e lands in slot (row[e], etype[e]) -- no one-hot, nothing of size [E, R, in]
        msg = x[col] if weight is None else x[col] * weight.unsqueeze(-1)
        out = torch.zeros((num_nodes * num_types, x.shape[1]), dtype=msg.dtype, device=msg.device)
        return out.index_add_(0, row * num_types + etype, msg).view(num_nodes, num_types, x.shape[1])
    coef = alpha[etype]
    if weight is not None:
        coef = coef * weight.unsqueeze(-1)
    msg = coef.unsqueeze(-1) * x[col].unsqueeze(1)  # [E, B, in]
    out = torch.zeros((num_nodes,) + tuple(msg.shape[1:]), dtype=msg.dtype, device=msg.device)
    return out.index_add_(0, row, msg)


def _bdd_composition(x, W, row, col, etype, weight, num_nodes):
    n_blocks, bi, bo = W.shape[1:]
    # (a broadcast product and a sum, not an einsum: that would be a batched matmul of E * B batches of 1 x bi x bo)
    msg = (x[col].view(-1, n_blocks, bi, 1) * W[etype]).sum(2).reshape(-1, n_blocks * bo)
    if weight is not None:
        msg = msg * weight.unsqueeze(-1)
    out = torch.zeros((num_nodes, n_blocks * bo), dtype=msg.dtype, device=msg.device)
    return out.index_add_(0, row, msg)


# ------------------------------------------------------------------------------------------------------------------ edge views
def _by_type(tplan, etype, ids, kind):
    """`ids` (row or col) in type-sorted order as int32, memoised."""
    return _aux(kind, lambda: (ids if tplan.sorted else ids.index_select(0, tplan.perm.long())).int().contiguous(), etype, ids)


def _typed_view(tplan, etype, key, other, n):
    """The view sorted by (key, type), stable: (rowptr [n + 1], `other` in view order, the types in view order, view position
    -> edge id), all int32.  It is the stable sort by `key` of the type-sorted order, so it is a plan like the others (and the
    range check of `key`)."""
    key_t = _aux("rgcn_key_by_type", lambda: key if tplan.sorted else key.index_select(0, tplan.perm.long()), etype, key)
    plan = edge_plan(key_t, n)

    def make():
        eid = tplan.perm.long().index_select(0, plan.perm.long())
        return other.index_select(0, eid).int(), etype.index_select(0, eid).int(), eid.int()

    return (plan.rowptr,) + _aux("rgcn_typed_view", make, etype, key, other)


def _eid(plan):
    return None if plan.sorted else plan.perm


# ----------------------------------------------------------------------------------------------------------------------- basis
def _basis_rows(entry, plan, gathered_ids, etype32, table, alpha, weight, k, n_rel, n_bases, out):
    dev, nnz = table.device, plan.perm.numel()
    ws, ws_bytes = _lib.workspace("cogdl_hip_rgcn_basis_workspace_bytes", dev, nnz, k)
    with _lib.on_device(dev):
        rc = getattr(_lib.hip(), entry)(_lib.ptr(plan.rowptr), _lib.ptr(gathered_ids), _lib.ptr(_eid(plan)), _lib.ptr(etype32),
                                        _lib.ptr(table), _lib.ptr(alpha), _lib.ptr(weight), _lib.ptr(out), plan.n, k, nnz, n_rel,
                                        n_bases, _lib.ptr(ws), ws_bytes, _lib.stream_of(out))
    _lib.check(rc, entry)
    return out


class _BasisAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha, weight, row, col, etype, num_nodes, num_types):
        x = x.contiguous()
        alpha = None if alpha is None else alpha.contiguous()
        weight = None if weight is None else weight.contiguous()
        n_bases = num_types if alpha is None else alpha.shape[1]
        tplan = edge_plan(etype, num_types)  # (first: an id outside [0, R) raises before any kernel reads alpha)
        splan = edge_plan(col, x.shape[0])
        dplan = edge_plan(row, num_nodes)
        etype32 = _aux("etype", lambda: etype.int().contiguous(), etype)
        ctx.plans, ctx.etype32, ctx.sizes = (splan, tplan), etype32, (num_types, n_bases)
        ctx.save_for_backward(x, alpha, weight, row, col, etype)
        k = x.shape[1]
        z = torch.empty((num_nodes, n_bases, k), dtype=torch.float32, device=x.device)
        return _basis_rows("cogdl_hip_rgcn_basis_fwd", dplan, dplan.colind(col), etype32, x, alpha, weight, k, num_types, n_bases, z)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, alpha, weight, row, col, etype = ctx.saved_tensors
        splan, tplan = ctx.plans
        n_rel, n_bases = ctx.sizes
        if grad.dtype != torch.float32:
            raise _lib.BackendError("rgcn_basis_aggregate backward: grad must be float32 (got %s)" % grad.dtype)
        grad = grad.contiguous()
        k, dev = x.shape[1], grad.device
        g_x = g_alpha = None
        if ctx.needs_input_grad[0]:
            g_x = torch.empty_like(x)
            _basis_rows("cogdl_hip_rgcn_basis_grad_x", splan, splan.colind(row), ctx.etype32, grad, alpha, weight, k, n_rel,
                        n_bases, g_x)
        if alpha is not None and ctx.needs_input_grad[1]:
            nnz = row.numel()
            g_alpha = torch.empty_like(alpha)
            ws, ws_bytes = _lib.workspace("cogdl_hip_rgcn_basis_grad_alpha_workspace_bytes", dev, nnz, n_rel, n_bases)
            with _lib.on_device(dev):
                rc = _lib.hip().cogdl_hip_rgcn_basis_grad_alpha(
                    _lib.ptr(tplan.rowptr), _lib.ptr(_by_type(tplan, etype, col, "src_by_type")), _lib.ptr(tplan.colind(row)),
                    _lib.ptr(_eid(tplan)), _lib.ptr(x), _lib.ptr(grad), _lib.ptr(weight), _lib.ptr(g_alpha), n_rel, n_bases, k,
                    nnz, _lib.ptr(ws), ws_bytes, _lib.stream_of(grad))
            _lib.check(rc, "rgcn_basis_grad_alpha")
        return g_x, g_alpha, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------------------- block diagonal
def _bdd_rows(view, table, blocks, weight, m, n_rel, n_blocks, bi, bo):
    rowptr, gathered, types, eid = view
    out = torch.empty((m, n_blocks * bo), dtype=torch.float32, device=table.device)
    with _lib.on_device(table.device):
        rc = _lib.hip().cogdl_hip_rgcn_bdd_fwd(_lib.ptr(rowptr), _lib.ptr(gathered), _lib.ptr(types), _lib.ptr(eid), _lib.ptr(table),
                                               _lib.ptr(blocks), _lib.ptr(weight), _lib.ptr(out), m, gathered.numel(), n_rel,
                                               n_blocks, bi, bo, _lib.stream_of(out))
    _lib.check(rc, "rgcn_bdd")
    return out


class _BddAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, weight, row, col, etype, num_nodes):
        x, W = x.contiguous(), W.contiguous()
        weight = None if weight is None else weight.contiguous()
        n_rel, n_blocks, bi, bo = W.shape
        tplan = edge_plan(etype, n_rel)
        sview = _typed_view(tplan, etype, col, row, x.shape[0])  # (the range check of col)
        dview = _typed_view(tplan, etype, row, col, num_nodes)
        ctx.views = (sview, tplan)
        ctx.save_for_backward(x, W, weight, row, col, etype)
        return _bdd_rows(dview, x, W, weight, num_nodes, n_rel, n_blocks, bi, bo)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, W, weight, row, col, etype = ctx.saved_tensors
        sview, tplan = ctx.views
        n_rel, n_blocks, bi, bo = W.shape
        if grad.dtype != torch.float32:
            raise _lib.BackendError("rgcn_bdd_aggregate backward: grad must be float32 (got %s)" % grad.dtype)
        grad = grad.contiguous()
        dev = grad.device
        g_x = g_w = None
        if ctx.needs_input_grad[0]:  # the same kernel, blocks transposed, the upstream gradient gathered
            g_x = _bdd_rows(sview, grad, W.transpose(2, 3).contiguous(), weight, x.shape[0], n_rel, n_blocks, bo, bi)
        if ctx.needs_input_grad[1]:
            nnz = row.numel()
            g_w = torch.empty_like(W)
            ws, ws_bytes = _lib.workspace("cogdl_hip_rgcn_bdd_grad_w_workspace_bytes", dev, nnz, n_rel, n_blocks, bi, bo)
            with _lib.on_device(dev):
                rc = _lib.hip().cogdl_hip_rgcn_bdd_grad_w(
                    _lib.ptr(tplan.rowptr), _lib.ptr(_by_type(tplan, etype, col, "src_by_type")), _lib.ptr(tplan.colind(row)),
                    _lib.ptr(_eid(tplan)), _lib.ptr(x), _lib.ptr(grad), _lib.ptr(weight), _lib.ptr(g_w), n_rel, n_blocks, bi, bo,
                    nnz, _lib.ptr(ws), ws_bytes, _lib.stream_of(grad))
            _lib.check(rc, "rgcn_bdd_grad_w")
        return g_x, g_w, None, None, None, None, None


# ----------------------------------------------------------------------------------------------------------------------- fronts
def _edges_ok(name, row, col, etype, weight):
    e = row.numel()
    if col.numel() != e or etype.numel() != e or (weight is not None and (weight.dim() != 1 or weight.numel() != e)):
        raise ValueError("%s: row, col, etype and weight must hold one entry per edge (%d, %d, %d, %s)"
                         % (name, e, col.numel(), etype.numel(), None if weight is None else tuple(weight.shape)))
    return e


def _route(floats, row, col, etype, weight, e):
    """None: every tensor on the CPU (quiet composition); "" : the kernels; otherwise the reason for the torch route."""
    tensors = floats + (row, col, etype) + (() if weight is None else (weight,))
    if not any(t.is_cuda for t in tensors):
        return None
    if not all(t.is_cuda for t in tensors):
        return "tensors on %s" % sorted({str(t.device) for t in tensors})
    if not all(t.dtype == torch.float32 for t in floats + (() if weight is None else (weight,))):
        return "dtypes %s" % ", ".join(str(t.dtype) for t in floats + (() if weight is None else (weight,)))
    if not (_is_index(row, e) and _is_index(col, e) and _is_index(etype, e)):
        return "row %s %s, col %s %s, etype %s %s" % (row.dtype, tuple(row.shape), col.dtype, tuple(col.shape), etype.dtype,
                                                     tuple(etype.shape))
    if weight is not None and weight.requires_grad and torch.is_grad_enabled():
        return "weight requires grad"
    if e == 0:
        return "E == 0"
    return ""


def rgcn_basis_aggregate(x, alpha, row, col, etype, weight=None, num_nodes=None, num_types=None):
    """x [N_src, in], alpha [R, B] or None (identity: B = R = num_types, read from etype when that is None too), row / col /
    etype int64 [E], weight [E] or None -> Z [num_nodes, B, in] (num_nodes defaults to x.shape[0]).  BackendError (GPU route)
    for a type outside [0, R), a source outside x or a destination outside [0, num_nodes)."""
    if x.dim() != 2 or (alpha is not None and alpha.dim() != 2):
        raise ValueError("rgcn_basis_aggregate: x and alpha must be 2-D (got %s and %s)"
                         % (tuple(x.shape), None if alpha is None else tuple(alpha.shape)))
    e = _edges_ok("rgcn_basis_aggregate", row, col, etype, weight)
    num_nodes = int(x.shape[0] if num_nodes is None else num_nodes)
    if alpha is not None:
        num_types = alpha.shape[0]
    elif num_types is None:
        num_types = int(etype.max()) + 1 if e else 0
    num_types = int(num_types)
    n_bases = num_types if alpha is None else alpha.shape[1]
    why = _route((x,) if alpha is None else (x, alpha), row, col, etype, weight, e)
    if why == "":
        if x.shape[1] == 0 or n_bases == 0 or num_nodes == 0 or x.shape[0] == 0:
            why = "a zero width or an empty x or output"
        elif n_bases > MAX_BASES:
            why = "B = %d > %d" % (n_bases, MAX_BASES)
    if why == "":
        return _BasisAggregate.apply(x, alpha, weight, row, col, etype, num_nodes, num_types)
    if why is not None:
        _note_torch_route("rgcn_basis_aggregate", why)
    return _basis_composition(x, alpha, row, col, etype, weight, num_nodes, num_types)


def rgcn_bdd_aggregate(x, W, row, col, etype, weight=None, num_nodes=None):
    """x [N_src, B * bi], W [R, B, bi, bo], row / col / etype int64 [E], weight [E] or None -> H [num_nodes, B * bo].
    BackendError (GPU route) for a type outside [0, R), a source outside x or a destination outside [0, num_nodes)."""
    if x.dim() != 2 or W.dim() != 4 or x.shape[1] != W.shape[1] * W.shape[2]:
        raise ValueError("rgcn_bdd_aggregate: x must be [N, B * bi] and W [R, B, bi, bo] (got %s and %s)"
                         % (tuple(x.shape), tuple(W.shape)))
    e = _edges_ok("rgcn_bdd_aggregate", row, col, etype, weight)
    num_nodes = int(x.shape[0] if num_nodes is None else num_nodes)
    n_rel, n_blocks, bi, bo = W.shape
    why = _route((x, W), row, col, etype, weight, e)
    if why == "":
        if 0 in (n_rel, n_blocks, bi, bo, num_nodes, x.shape[0]):
            why = "a zero width or an empty x, W or output"
        elif n_blocks * bi > MAX_BDD_WIDTH or n_blocks * bo > MAX_BDD_WIDTH:
            why = "in = %d, out = %d > %d" % (n_blocks * bi, n_blocks * bo, MAX_BDD_WIDTH)
        elif bi * bo > MAX_BDD_BLOCK:
            why = "bi * bo = %d > %d" % (bi * bo, MAX_BDD_BLOCK)
    if why == "":
        return _BddAggregate.apply(x, W, weight, row, col, etype, num_nodes)
    if why is not None:
        _note_torch_route("rgcn_bdd_aggregate", why)
    return _bdd_composition(x, W, row, col, etype, weight, num_nodes)
