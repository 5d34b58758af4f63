"""Sampled triple scoring for knowledge-graph embedding training: the score of each query row against the table rows an
index matrix names, with gradients for the queries and the table.

    sampled_scores(q, table, idx, kind, gamma=0.0, *, check=True) -> scores   float [B, K]       (autograd: q, table)
        q       [B, D]  float     prepared queries (cogdl_amd.kgrank.prepare_query)
        table   [N, D]  float     the entity table
        idx     [B, K]  int32 / int64 in [0, N): the candidates of each query (negative samples, or the positive tail)
        kind    "dot":  s[b, j] = SUM_k q[b,k] * table[idx[b,j],k]
                "l1":   s[b, j] = gamma - SUM_k |q[b,k] - table[idx[b,j],k]|
                "cl2":  s[b, j] = gamma - SUM_{k < D/2} sqrt((q[b,k] - t[k])^2 + (q[b,k+D/2] - t[k+D/2])^2),  t = table[idx[b,j]]
                        (D even: the halves are real and imaginary parts, as torch.chunk(.., 2) splits them)

The reference scores a batch by gathering a [B, K, D] copy of the table, broadcasting the query against it through three to
eight elementwise kernels and, backward, scattering [B K, D] gradient rows into the table with float atomics
(cogdl/models/emb/knowledge_base.py:52-101).  Here nothing of size [B, K, D] exists: forward and backward read each named row
once, the autograd node saves q, table and idx only.  float32 CUDA tensors run the HIP kernels (csrc/kgscore.hip), float32 CPU
tensors the OpenMP host twin; both follow csrc/kgscore_law.h -- per pair of rows 64 slot partials and a fixed butterfly,
grad_q summed over j in ascending order, grad_table over the occurrences of an entity in ascending flat position in chunks of
512 -- so scores and both gradients are equal bit for bit between the two and from run to run (no float atomics).  Backward
computes only the gradients that are asked for; the table's needs the inverted index of idx, built per call with one stable
torch.sort of the flat ids and a searchsorted on their device.  Backward is once_differentiable.

Any other floating dtype, D above 16384 and an empty B, K, N or D run the gather composition on torch (on the GPU it says so
once per reason with a TorchRouteWarning); its sums are torch's.  check=True validates idx in [0, N) with one flag read-back
before anything is gathered and raises BackendError; check=False skips the read-back: a position whose id is out of range
scores NaN and contributes to no gradient.  Mismatched shapes, dtypes or devices and odd D with cl2 raise.

Not for use under torch.cuda.graph capture (the validation reads a flag, the backward sorts and allocates).
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .kgrank import KINDS
from .ops import _ROUTE_NOTED, TorchRouteWarning

MAX_D = 16384  # cogdl_kgscore::kMaxD: the widest row the kernels hold in LDS


def _note_torch_route(why):
    if ("sampled_scores", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("sampled_scores", why))
    import warnings

    warnings.warn("cogdl_amd.operators.kgscore.sampled_scores: GPU tensors on the torch route (%s): the [B, K, D] gather "
                  "composition on torch's kernels; the HIP kernels cover float32 with B, K, N of at least 1 and D in 1 .. %d"
                  % (why, MAX_D), TorchRouteWarning, stacklevel=3)


def gather_composition(q, table, idx, kind, gamma=0.0):
    """The reference's arithmetic: gather [B, K, D], broadcast, reduce.  An id outside [0, N) scores NaN without a gradient."""
    b, k = idx.shape
    n = table.shape[0]
    if b == 0 or k == 0:
        return q.new_zeros((b, k)) + 0 * (q.sum() + table.sum())
    if n == 0:
        return q.new_full((b, k), float("nan")) + 0 * (q.sum() + table.sum())
    ids = idx.long()
    valid = (ids >= 0) & (ids < n)
    rows = table[ids.clamp(0, n - 1).reshape(-1)].view(b, k, table.shape[1])
    qb = q.unsqueeze(1)
    if kind == "dot":
        s = (qb * rows).sum(-1)
    elif kind == "l1":
        s = gamma - torch.norm(qb - rows, p=1, dim=2)
    else:
        re_q, im_q = torch.chunk(qb, 2, dim=2)
        re_t, im_t = torch.chunk(rows, 2, dim=2)
        s = gamma - torch.stack([re_q - re_t, im_q - im_t], dim=0).norm(dim=0).sum(dim=2)
    return torch.where(valid, s, s.new_full((), float("nan")))


def inverted_index(idx32, n):
    """-> (occ_ptr int32 [n + 1], occ_pos int32 [B K]): occ_pos[occ_ptr[e] : occ_ptr[e + 1]] are the flat positions of entity e
    in idx, ascending (one stable sort).  Ids below 0 sort in front of occ_ptr[0], ids of n and above behind occ_ptr[n]: they
    are in no list."""
    flat = idx32.reshape(-1)
    ids, pos = torch.sort(flat, stable=True)
    bounds = torch.arange(n + 1, dtype=torch.int32, device=flat.device)
    occ_ptr = torch.searchsorted(ids, bounds, out_int32=True)
    return occ_ptr.contiguous(), pos.to(torch.int32).contiguous()


class _SampledScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, table, idx32, kind, gamma):
        (b, d), n, k = q.shape, table.shape[0], idx32.shape[1]
        q, table = q.contiguous(), table.contiguous()
        scores = torch.empty((b, k), dtype=torch.float32, device=q.device)
        _lib.twin_call("kg_score", q.device, _lib.ptr(q), _lib.ptr(table), _lib.ptr(idx32), b, k, n, d, KINDS[kind], gamma,
                       _lib.ptr(scores))
        ctx.save_for_backward(q, table, idx32)
        ctx.kind = kind
        return scores

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, table, idx32 = ctx.saved_tensors
        (b, d), n, k = q.shape, table.shape[0], idx32.shape[1]
        dev, kind = q.device, KINDS[ctx.kind]
        g = g.contiguous()
        grad_q = grad_table = None
        if ctx.needs_input_grad[0]:
            grad_q = torch.empty_like(q)
            _lib.twin_call("kg_score_grad_q", dev, _lib.ptr(q), _lib.ptr(table), _lib.ptr(idx32), _lib.ptr(g), b, k, n, d, kind,
                           _lib.ptr(grad_q))
        if ctx.needs_input_grad[1]:
            occ_ptr, occ_pos = inverted_index(idx32, n)
            grad_table = torch.empty_like(table)  # (every row is written, zeros included)
            _lib.twin_call("kg_score_grad_table", dev, _lib.ptr(q), _lib.ptr(table), _lib.ptr(g), _lib.ptr(occ_ptr),
                           _lib.ptr(occ_pos), b, k, n, d, kind, _lib.ptr(grad_table))
        return grad_q, grad_table, None, None, None


def sampled_scores(q, table, idx, kind, gamma=0.0, *, check=True):
    """-> scores [B, K] with gradients for q and table; see the module docstring.  Not for use under torch.cuda.graph capture."""
    if kind not in KINDS:
        raise ValueError("sampled_scores: kind must be one of %s (got %r)" % (sorted(KINDS), kind))
    if not (torch.is_tensor(q) and torch.is_tensor(table) and torch.is_tensor(idx)):
        raise ValueError("sampled_scores: q, table and idx must be tensors")
    if q.dim() != 2 or table.dim() != 2 or q.shape[1] != table.shape[1]:
        raise ValueError("sampled_scores: q must be [B, D] and table [N, D] (got %s and %s)" % (tuple(q.shape), tuple(table.shape)))
    (b, d), n = q.shape, table.shape[0]
    if idx.dim() != 2 or idx.shape[0] != b or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError("sampled_scores: idx must be int32 / int64 [B, K] (got %s %s)" % (idx.dtype, tuple(idx.shape)))
    k = idx.shape[1]
    if kind == "cl2" and d % 2:
        raise ValueError("sampled_scores: kind 'cl2' needs an even D (got %d)" % d)
    if q.dtype != table.dtype or not q.dtype.is_floating_point:
        raise ValueError("sampled_scores: q and table must share a floating dtype (got %s and %s)" % (q.dtype, table.dtype))
    dev = q.device
    for t in (table, idx):
        if t.device != dev:
            raise _lib.BackendError("sampled_scores: tensors on different devices: %s vs %s" % (dev, t.device))
    if dev.type not in ("cuda", "cpu"):
        raise _lib.BackendError("sampled_scores: no implementation for device %s" % dev)
    if max(b, k, n, d) >= 2 ** 31 - 1 or b * k >= 2 ** 31 - 1:
        raise _lib.BackendError("sampled_scores: sizes beyond int32 indexing")
    if check and b and k:  # one flag, one read-back, before anything gathers
        if bool((idx.min() < 0) | (idx.max() >= n)):
            raise _lib.BackendError("sampled_scores: an idx entry outside [0, %d)" % n)
    gamma = float(gamma)
    why = None
    if q.dtype != torch.float32:
        why = "dtype %s" % q.dtype
    elif b == 0 or k == 0 or n == 0 or d == 0:
        why = "an empty operand: B %d, K %d, N %d, D %d" % (b, k, n, d)
    elif d > MAX_D and dev.type == "cuda":
        why = "D %d above %d" % (d, MAX_D)
    if why is not None:
        if dev.type == "cuda":
            _note_torch_route(why)
        return gather_composition(q, table, idx, kind, gamma)
    if idx.dtype != torch.int32:  # (ids beyond int32 are out of range of any table the kernels index: keep them so)
        idx = idx.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return _SampledScores.apply(q, table, idx.contiguous(), kind, gamma)
