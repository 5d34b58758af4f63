"""The aggregation of GENConv, DeeperGCN's layer (cogdl/layers/deepergcn_layer.py:67-93), as one operator.

    gen_aggregate(x, row, col, eterm=None, aggr="softmax", beta=None, eps=1e-7, num_nodes=None) -> [num_nodes, F]
                                                                                          (autograd: x, eterm, beta)
        m[e]   = relu(x[col[e]] + eterm[e]) + eps
        softmax:  out[v] = sum over the edges e with row[e] == v of  softmax_{row[e] == v}(beta * m[e]) * m[e]   (per column)
        sum:      out[v] = sum of m[e]           mean:  out[v] = sum of m[e] * (1 / deg(v))      (an empty row gives 0)

The reference gathers x[col] into an [E, F] tensor, makes a second with relu + eps, a third with beta *, a fourth with
edge_softmax (one channel per column), a fifth with the product and scatter_add_s it -- atomics on a GPU.  fp32 GPU tensors go
to one HIP kernel (cogdl_hip_gen_aggr_fwd, csrc/genaggr.hip) over the destination-sorted view of the edges: an online softmax
per column in the caller's edge order, no [E, F] tensor, no atomics.  The backward is one kernel over the source-sorted view
(cogdl_hip_gen_aggr_bwd): it recomputes m, gathers the gradient, output and log-sum-exp rows of the destination and adds

    d = g[v] * exp(beta * m - lse[v]) * (1 + beta * (m - out[v])) * [x[u] + eterm[e] > 0]          (sum / mean: g[v] * w_v * [..])

per source in the caller's edge order; the same pass stores d as the gradient of eterm when that is wanted (an [E, F] tensor
the caller asked for).  The gradient of beta is  sum(g * (q - out^2))  with q[v] = sum_e softmax_e * m_e^2  from the forward:
[N, F] tensors only.  Saved for the backward: x, eterm, out, lse and (beta requires grad) q.  Both views are the memoised plans
of operators/ops.py (`edge_plan`); building them is also the range check of row and col.  Once they exist nothing is read back
(beta, when a tensor, is read by the kernel through its address), so a later call on the same index tensors can be captured
in a graph.

CPU tensors run the torch composition: the same formula with a true per-row softmax, the row maximum subtracted.  A GPU call
the kernel does not cover (other dtypes, tensors on several devices, F == 0, E == 0, an empty x or output) runs the same
composition and says so once per reason with a TorchRouteWarning, as operators/ops.py does.
"""
import torch

from .. import _lib
from .ops import _ROUTE_NOTED, TorchRouteWarning, edge_plan

AGGRS = ("softmax", "sum", "mean")
_MODE = {"softmax": 0, "sum": 1, "mean": 2}  # COGDL_HIP_GEN_*


def _note_torch_route(why):
    """Never silent, as in operators/ops.py: the first GPU call per reason that takes the torch route says so."""
    if ("gen_aggregate", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("gen_aggregate", why))
    import warnings

    warnings.warn("cogdl_amd.operators.genaggr.gen_aggregate: GPU tensors on the torch route (%s); the fused HIP kernel covers "
                  "2-D float32 x and eterm with 1-D int64 row and col, all on one device" % why, TorchRouteWarning, stacklevel=3)


def _composition(x, row, col, eterm, aggr, beta, eps, num_nodes):
    """The layer's expression with a true per-row softmax (row maximum subtracted): gather, relu + eps, softmax, scatter_add_."""
    pre = x[col]
    if eterm is not None:
        pre = pre + eterm
    m = torch.relu(pre) + eps
    f = m.shape[1]
    idx = row.unsqueeze(-1).expand(-1, f)
    zeros = torch.zeros((num_nodes, f), dtype=m.dtype, device=m.device)
    if aggr == "softmax":
        z = m if beta is None else beta * m
        top = torch.full((num_nodes, f), float("-inf"), dtype=m.dtype, device=m.device)
        top = top.scatter_reduce(0, idx, z.detach(), "amax", include_self=True)  # (a constant shift: outside autograd)
        p = torch.exp(z - top[row])
        h = m * (p / zeros.scatter_add(0, idx, p)[row])
    elif aggr == "mean":
        inv = torch.bincount(row, minlength=num_nodes).to(m.dtype).pow(-1)
        inv = torch.where(torch.isinf(inv), torch.zeros_like(inv), inv)
        h = m * inv[row].unsqueeze(-1)
    else:
        h = m
    return zeros.scatter_add(0, idx, h)


def _beta_args(beta_t, beta_f):
    return (_lib.ptr(beta_t), 1.0) if beta_t is not None else (None, float(beta_f))


class _GenAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eterm, beta_t, row, col, aggr, beta_f, eps, num_nodes):
        x = x.contiguous()
        eterm = None if eterm is None else eterm.contiguous()
        splan = edge_plan(col, x.shape[0])  # (first: a source outside x raises before any kernel gathers it)
        dplan = edge_plan(row, num_nodes)
        dev, k, nnz = x.device, x.shape[1], row.numel()
        softmax = aggr == "softmax"
        want_beta = softmax and beta_t is not None and ctx.needs_input_grad[2]
        want_bwd = any(ctx.needs_input_grad[:3])
        out = torch.empty((num_nodes, k), dtype=torch.float32, device=dev)
        lse = torch.empty_like(out) if softmax and want_bwd else None
        q = torch.empty_like(out) if want_beta else None
        ws, ws_bytes = _lib.workspace("cogdl_hip_gen_aggr_fwd_workspace_bytes", dev, nnz, k)
        eid = None if dplan.sorted else dplan.perm
        bptr, bval = _beta_args(beta_t if softmax else None, beta_f)
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_gen_aggr_fwd(_lib.ptr(dplan.rowptr), _lib.ptr(dplan.colind(col)), _lib.ptr(eid), _lib.ptr(x),
                                                   _lib.ptr(eterm), _MODE[aggr], bptr, bval, eps, _lib.ptr(out), _lib.ptr(lse),
                                                   _lib.ptr(q), num_nodes, k, nnz, _lib.ptr(ws), ws_bytes, _lib.stream_of(out))
        _lib.check(rc, "gen_aggr_fwd")
        ctx.plans, ctx.aggr, ctx.beta_f, ctx.eps = (dplan, splan), aggr, beta_f, eps
        ctx.save_for_backward(x, eterm, beta_t, row, out, lse, q)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, eterm, beta_t, row, out, lse, q = ctx.saved_tensors
        dplan, splan = ctx.plans
        if grad.dtype != torch.float32:
            raise _lib.BackendError("gen_aggregate backward: grad must be float32 (got %s)" % grad.dtype)
        grad = grad.contiguous()
        softmax = ctx.aggr == "softmax"
        dev, k, nnz = x.device, x.shape[1], row.numel()
        g_x = g_t = g_beta = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gs = grad
            if ctx.aggr == "mean":  # autograd's `grad[row] * deg_rev[row]`, one rounding: taken per destination, then gathered
                inv = (dplan.rowptr[1:] - dplan.rowptr[:-1]).float().pow(-1)
                gs = grad * torch.where(torch.isinf(inv), torch.zeros_like(inv), inv).view(-1, 1)
            g_x = torch.empty_like(x)
            if ctx.needs_input_grad[1]:
                g_t = torch.empty((nnz, k), dtype=torch.float32, device=dev)
            ws, ws_bytes = _lib.workspace("cogdl_hip_gen_aggr_bwd_workspace_bytes", dev, nnz, k)
            eid = None if splan.sorted else splan.perm
            bptr, bval = _beta_args(beta_t if softmax else None, ctx.beta_f)
            with _lib.on_device(dev):
                rc = _lib.hip().cogdl_hip_gen_aggr_bwd(_lib.ptr(splan.rowptr), _lib.ptr(splan.colind(row)), _lib.ptr(eid),
                                                       _lib.ptr(x), _lib.ptr(eterm), _lib.ptr(gs), _lib.ptr(out), _lib.ptr(lse),
                                                       _MODE[ctx.aggr], bptr, bval, ctx.eps, _lib.ptr(g_x), _lib.ptr(g_t),
                                                       x.shape[0], k, nnz, _lib.ptr(ws), ws_bytes, _lib.stream_of(grad))
            _lib.check(rc, "gen_aggr_bwd")
            if not ctx.needs_input_grad[0]:
                g_x = None
        if q is not None and ctx.needs_input_grad[2]:
            g_beta = (grad * (q - out * out)).sum().reshape(beta_t.shape)
        return g_x, g_t, g_beta, None, None, None, None, None, None


def _is_index(t, e):
    return t.dim() == 1 and t.dtype == torch.int64 and t.numel() == e


def gen_aggregate(x, row, col, eterm=None, aggr="softmax", beta=None, eps=1e-7, num_nodes=None):
    """x [N_src, F]; row / col int64 [E] (destination, source of every edge); eterm [E, F] or None (the encoded edge features);
    beta None (1.0), a float or a one-element tensor (may require grad; `softmax` only) -> [num_nodes, F] (num_nodes defaults to
    x.shape[0]).  ValueError for an unknown aggr or mismatched shapes; BackendError (GPU route) for a source outside x or a
    destination outside [0, num_nodes)."""
    if aggr not in AGGRS:
        raise ValueError("gen_aggregate: aggr must be one of %s (got %r)" % (AGGRS, aggr))
    if x.dim() != 2:
        raise ValueError("gen_aggregate: x must be 2-D (got %s)" % (tuple(x.shape),))
    e = row.numel()
    if col.numel() != e:
        raise ValueError("gen_aggregate: row and col must hold one entry per edge (%d, %d)" % (e, col.numel()))
    if eterm is not None and tuple(eterm.shape) != (e, x.shape[1]):
        raise ValueError("gen_aggregate: eterm must be [E, F] = (%d, %d) (got %s)" % (e, x.shape[1], tuple(eterm.shape)))
    beta_t = beta if torch.is_tensor(beta) else None
    if beta_t is not None and beta_t.numel() != 1:
        raise ValueError("gen_aggregate: beta must hold one element (got %s)" % (tuple(beta_t.shape),))
    beta_f = 1.0 if beta is None or beta_t is not None else float(beta)
    num_nodes = int(x.shape[0] if num_nodes is None else num_nodes)
    if aggr != "softmax":
        beta_t, beta_f = None, 1.0
    tensors = (x, row, col) + tuple(t for t in (eterm, beta_t) if t is not None)
    beta_c = beta_t if beta_t is not None else (None if beta is None or aggr != "softmax" else beta_f)
    if not any(t.is_cuda for t in tensors):
        return _composition(x, row, col, eterm, aggr, beta_c, eps, num_nodes)  # the CPU route: quiet
    why = None
    floats = (x,) + tuple(t for t in (eterm, beta_t) if t is not None)
    if not all(t.is_cuda and t.device == x.device for t in tensors):
        why = "tensors on %s" % sorted({str(t.device) for t in tensors})
    elif not all(t.dtype == torch.float32 for t in floats):
        why = "x %s, eterm %s, beta %s" % (x.dtype, None if eterm is None else eterm.dtype, None if beta_t is None else beta_t.dtype)
    elif not (_is_index(row, e) and _is_index(col, e)):
        why = "row %s %s, col %s %s" % (row.dtype, tuple(row.shape), col.dtype, tuple(col.shape))
    elif x.shape[1] == 0:
        why = "F == 0"
    elif num_nodes == 0 or x.shape[0] == 0:
        why = "an empty x or output"
    elif e == 0:
        why = "E == 0"
    if why is not None:
        _note_torch_route(why)
        return _composition(x, row, col, eterm, aggr, beta_c, eps, num_nodes)
    return _GenAggregate.apply(x, eterm, beta_t, row, col, aggr, beta_f, float(eps), num_nodes)
