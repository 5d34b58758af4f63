"""Message passing on a multi-relational graph: every edge (row <- col) carries a type, and its message combines the source
row with that type's row of a small relation table.

    rel_gspmm(x, rel, row, col, etype, weight=None, op="sub", num_nodes=None) -> [num_nodes, F]          (autograd: x, rel)

        out[v] = sum over the edges e with row[e] == v of  weight[e] * ( x[col[e]]  OP  rel[etype[e]] )     OP: sub | mul | add

This is what CompGCNLayer.message_passing computes in front of its weight (cogdl/models/nn/compgcn.py:124-140), where the
reference gathers x[col] and rel_embed[edge_type] into two [E, F] tensors, combines them, multiplies by the layer weight and
scatter_add_s [E, out] rows -- atomics on a GPU.  fp32 GPU tensors go to one HIP kernel (cogdl_hip_rel_gspmm,
csrc/relspmm.hip) over the destination-sorted view of the edges: no [E, F] tensor, no atomics, per output element the edges
are added in the caller's edge order.  The backward is the same kernel over the source-sorted view (grad of x) and the
relation-gradient kernel over the type-sorted view (grad of rel, cogdl_hip_rel_gspmm_grad_rel): deterministic as well.  The
three views are the memoised plans of operators/ops.py (`edge_plan`); building the type plan is also the range check of
`etype`, and the source plan that of `col`.  Once the plans exist nothing is read back, so a later call on the same index
tensors can be captured in a graph.

CPU tensors run the plain torch composition -- the reference's arithmetic.  A GPU call the kernel does not cover (other
dtypes, a weight that requires grad, F == 0, E == 0) runs the same composition and says so once per reason with a
TorchRouteWarning, as operators/ops.py does.
"""
import collections

import torch

from .. import _lib
from ..plan import tensor_key
from .ops import _BINARY, _OPS, _OPS_WMUL, _ROUTE_NOTED, TorchRouteWarning, edge_plan

OPS = ("sub", "mul", "add")

# int32 copies in the order a kernel wants them, memoised like the plans on the identity of their source tensors (which the
# entry keeps alive, so an address cannot be recycled under the same key)
_AUX = collections.OrderedDict()
_MAX_AUX = 32


def _aux(kind, make, *sources):
    key = (kind,) + tuple(tensor_key(t) for t in sources)
    hit = _AUX.get(key)
    if hit is None:
        hit = (make(), sources)
        _AUX[key] = hit
        while len(_AUX) > _MAX_AUX:
            _AUX.popitem(last=False)
    else:
        _AUX.move_to_end(key)
    return hit[0]


def clear_plans():
    _AUX.clear()


def _note_torch_route(why):
    """Never silent, as in operators/ops.py: the first GPU call per reason that takes the torch route says so."""
    if ("rel_gspmm", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("rel_gspmm", why))
    import warnings

    warnings.warn("cogdl_amd.operators.relational.rel_gspmm: GPU tensors on the reference's torch route (%s); the fused HIP "
                  "kernel covers 2-D float32 x and rel with 1-D int64 row, col and etype and a weight outside autograd" % why,
                  TorchRouteWarning, stacklevel=3)


def _composition(x, rel, row, col, etype, weight, op, num_nodes):
    """The reference's expression: gather, combine, scale, scatter_add_."""
    msg = _BINARY[op](x[col], rel[etype])
    if weight is not None:
        msg = msg * weight.unsqueeze(-1)
    out = torch.zeros((num_nodes, msg.shape[1]), dtype=msg.dtype, device=msg.device)
    return out.scatter_add_(0, row.unsqueeze(-1).expand(-1, msg.shape[1]), msg)


def _launch(plan, colind, etype32, x, rel, weight, op, k):
    """out[v] = sum_{j in row v of plan} weight[id] * (x[colind[j]] OP rel[etype32[id]]); colind int32 in sorted order."""
    dev = x.device
    nnz = plan.perm.numel()
    out = torch.empty((plan.n, k), dtype=torch.float32, device=dev)
    ws, ws_bytes = _lib.workspace("cogdl_hip_rel_gspmm_workspace_bytes", dev, nnz, k)
    eid = None if plan.sorted else plan.perm
    with _lib.on_device(dev):
        rc = _lib.hip().cogdl_hip_rel_gspmm(_lib.ptr(plan.rowptr), _lib.ptr(colind), _lib.ptr(eid), _lib.ptr(etype32),
                                            _lib.ptr(x), _lib.ptr(rel), _lib.ptr(weight), op, _lib.ptr(out), plan.n, k, nnz,
                                            0 if rel is None else rel.shape[0], _lib.ptr(ws), ws_bytes, _lib.stream_of(out))
    _lib.check(rc, "rel_gspmm")
    return out


class _RelGspmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rel, weight, row, col, etype, op, num_nodes):
        x, rel = x.contiguous(), rel.contiguous()
        weight = None if weight is None else weight.contiguous()
        tplan = edge_plan(etype, rel.shape[0])  # (first: an id outside [0, R) raises before any kernel reads rel)
        splan = edge_plan(col, x.shape[0])      # (and a source outside x)
        dplan = edge_plan(row, num_nodes)
        etype32 = _aux("etype", lambda: etype.int().contiguous(), etype)
        ctx.plans, ctx.op, ctx.etype32 = (dplan, splan, tplan), op, etype32
        ctx.save_for_backward(x, rel, weight, row, col, etype)
        return _launch(dplan, dplan.colind(col), etype32, x, rel, weight, _OPS[op], x.shape[1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        """grad of x: the same kernel over the source-sorted view (rows = sources, gathered operand = the upstream gradient
        rows, autograd's rounding order); grad of rel: the relation-gradient kernel over the type-sorted view.  Per element
        the edges are added in the caller's edge order, as index_add_ does on the CPU."""
        x, rel, weight, row, col, etype = ctx.saved_tensors
        _, splan, tplan = ctx.plans
        if grad.dtype != torch.float32:
            raise _lib.BackendError("rel_gspmm backward: grad must be float32 (got %s)" % grad.dtype)
        grad = grad.contiguous()
        k, dev = x.shape[1], grad.device
        g_x = g_rel = None
        if ctx.needs_input_grad[0]:
            dst_sorted = splan.colind(row)
            if ctx.op == "mul":
                g_x = _launch(splan, dst_sorted, ctx.etype32, grad, rel, weight, _OPS_WMUL, k)
            else:  # d msg / d src = 1: the message is the gradient row alone (times the weight)
                g_x = _launch(splan, dst_sorted, None, grad, None, weight, _OPS["add"], k)
        if ctx.needs_input_grad[1]:
            n_rel, nnz = rel.shape[0], row.numel()
            dst_by_type = tplan.colind(row)
            src_by_type = None
            if ctx.op == "mul":
                src_by_type = _aux("src_by_type", lambda: (col if tplan.sorted else col.index_select(0, tplan.perm.long())).int().contiguous(),
                                   etype, col)
            g_rel = torch.empty((n_rel, k), dtype=torch.float32, device=dev)
            ws, ws_bytes = _lib.workspace("cogdl_hip_rel_gspmm_grad_rel_workspace_bytes", dev, nnz, k)
            eid = None if tplan.sorted else tplan.perm
            with _lib.on_device(dev):
                rc = _lib.hip().cogdl_hip_rel_gspmm_grad_rel(_lib.ptr(tplan.rowptr), _lib.ptr(dst_by_type), _lib.ptr(src_by_type),
                                                             _lib.ptr(eid), _lib.ptr(grad), _lib.ptr(x), _lib.ptr(weight),
                                                             _OPS[ctx.op], _lib.ptr(g_rel), n_rel, k, nnz, _lib.ptr(ws), ws_bytes,
                                                             _lib.stream_of(grad))
            _lib.check(rc, "rel_gspmm_grad_rel")
        return g_x, g_rel, None, None, None, None, None, None


def _is_index(t, e):
    return t.dim() == 1 and t.dtype == torch.int64 and t.numel() == e


def rel_gspmm(x, rel, row, col, etype, weight=None, op="sub", num_nodes=None):
    """x [N_src, F], rel [R, F], row / col / etype int64 [E] (destination, source, relation of every edge), weight [E] or
    None -> [num_nodes, F] (num_nodes defaults to x.shape[0]).  ValueError for an unknown op or a rel of another width;
    BackendError (GPU route) for a type outside [0, R), a source outside x or a destination outside [0, num_nodes)."""
    if op not in OPS:
        raise ValueError("rel_gspmm: op must be one of %s (got %r)" % (OPS, op))
    if x.dim() != 2 or rel.dim() != 2:
        raise ValueError("rel_gspmm: x and rel must be 2-D (got %s and %s)" % (tuple(x.shape), tuple(rel.shape)))
    if rel.shape[1] != x.shape[1]:
        raise ValueError("rel_gspmm: rel has %d columns, x has %d" % (rel.shape[1], x.shape[1]))
    e = row.numel()
    if col.numel() != e or etype.numel() != e or (weight is not None and (weight.dim() != 1 or weight.numel() != e)):
        raise ValueError("rel_gspmm: row, col, etype and weight must hold one entry per edge (%d, %d, %d, %s)"
                         % (e, col.numel(), etype.numel(), None if weight is None else tuple(weight.shape)))
    num_nodes = int(x.shape[0] if num_nodes is None else num_nodes)
    tensors = (x, rel, row, col, etype) + (() if weight is None else (weight,))
    if not any(t.is_cuda for t in tensors):
        return _composition(x, rel, row, col, etype, weight, op, num_nodes)  # the reference's own path: quiet
    why = None
    if not all(t.is_cuda for t in tensors):
        why = "tensors on %s" % sorted({str(t.device) for t in tensors})
    elif not all(t.dtype == torch.float32 for t in (x, rel) + (() if weight is None else (weight,))):
        why = "x %s, rel %s, weight %s" % (x.dtype, rel.dtype, None if weight is None else weight.dtype)
    elif not (_is_index(row, e) and _is_index(col, e) and _is_index(etype, e)):
        why = "row %s %s, col %s %s, etype %s %s" % (row.dtype, tuple(row.shape), col.dtype, tuple(col.shape), etype.dtype,
                                                     tuple(etype.shape))
    elif weight is not None and weight.requires_grad and torch.is_grad_enabled():
        why = "weight requires grad"
    elif x.shape[1] == 0:
        why = "F == 0"
    elif e == 0:
        why = "E == 0"
    elif num_nodes == 0 or x.shape[0] == 0 or rel.shape[0] == 0:
        why = "an empty x, rel or output"
    if why is not None:
        _note_torch_route(why)
        return _composition(x, rel, row, col, etype, weight, op, num_nodes)
    return _RelGspmm.apply(x, rel, weight, row, col, etype, op, num_nodes)
