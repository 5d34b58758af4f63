"""All-entity ranking for knowledge-graph link prediction: the rank of a target among all N candidates as a count.

    rank_all(q, table, target, kind, gamma=0.0, filt_ptr=None, filt_idx=None) -> counts   int32 [M, 3]
        q       [M, D]  float32   prepared queries (cogdl_amd.kgrank.prepare_query)
        table   [N, D]  float32   the candidate (entity) table
        target  [M]     int32 / int64 in [0, N)
        kind    "dot":  s(i, e) = SUM_k q[i,k] * table[e,k]
                "l1":   s(i, e) = gamma - SUM_k |q[i,k] - table[e,k]|
                "cl2":  s(i, e) = gamma - SUM_{k < D/2} sqrt((q[i,k] - table[e,k])^2 + (q[i,k+D/2] - table[e,k+D/2])^2)
                        (D even: the halves are real and imaginary parts, as torch.chunk(.., 2) splits them)
        filt_ptr [M + 1], filt_idx [filt_ptr[M]]  int32 / int64: per query, entity ids to leave out (any order, duplicates
                        allowed); the target itself is never left out even if listed
        counts[i] = (greater, equal_before, equal_after) over the candidates e != target[i] that are not left out:
                        s(i,e) > s(i,t);   s(i,e) == s(i,t) and e < t;   s(i,e) == s(i,t) and e > t
    ranks(counts, ties="stable")  -> 1-based ranks: stable 1 + greater + equal_before, optimistic 1 + greater, pessimistic
                        1 + greater + equal_before + equal_after (int64), mean 1 + greater + (equal_before + equal_after) / 2
                        (float64)

Ties are reported, not resolved: where scores are equal the position a sort gives the target is the sort's business
(torch.sort is not stable by default), and all that can be said of it is greater <= position <= greater + equal_before +
equal_after.  A NaN score compares false both ways and is counted nowhere: a NaN candidate is in none of the three counts,
and a query whose target scores NaN has all three counts 0.

The score of a pair of rows is csrc/kgrank_law.h's: one pass over k in ascending order, no split over k, the target's score
from the same operations as every candidate's.  float32 CUDA tensors run the HIP kernels (csrc/kgrank.hip: dot on the fp32
MFMA, l1 and cl2 on the VALU; nothing of size [M, N] or [M, N, D] exists), float32 CPU tensors the OpenMP host twin; both
return the same counts, equal from run to run.  The filter is a correction pass over the list entries; the lists are sorted
per query here (one torch sort on their device), which is where duplicates go.  Any other dtype and M, N or D of 0 run a
blocked torch composition (on the GPU it says so once per reason with a TorchRouteWarning); its sums are torch's, so its
counts need not equal the kernels' where scores are within rounding of the target's.  Ids outside [0, N), a non-monotone
filt_ptr, odd D with cl2 and mismatched shapes raise before anything is gathered (one flag is read back).  Forward only:
the outputs are integers.  Not for use under torch.cuda.graph capture (the validation reads a flag).
"""
import torch

from .. import _lib
from .ops import _ROUTE_NOTED, TorchRouteWarning

KINDS = {"dot": 0, "l1": 1, "cl2": 2}  # COGDL_HIP_KG_*
TIES = ("stable", "optimistic", "pessimistic", "mean")
_BLOCK_BYTES = 64 << 20


def _note_torch_route(why):
    if ("rank_all", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("rank_all", why))
    import warnings

    warnings.warn("cogdl_amd.operators.kgrank.rank_all: GPU tensors on the torch route (%s): the blocked composition on torch's "
                  "kernels; the HIP kernels cover float32 with M, N and D of at least 1" % why, TorchRouteWarning, stacklevel=3)


def slice_entities(m, n, d, kind):
    """The number of consecutive table rows one workgroup of the counting launch walks for these sizes."""
    return int(_lib.hip().cogdl_hip_kg_rank_slice_entities(int(m), int(n), int(d), KINDS[kind]))


def _scores(qb, table, kind, gamma):
    if kind == "dot":
        return qb @ table.t()
    if kind == "l1":
        return gamma - (qb.unsqueeze(1) - table.unsqueeze(0)).abs().sum(-1)
    h = table.shape[1] // 2
    re = qb[:, None, :h] - table[None, :, :h]
    im = qb[:, None, h:] - table[None, :, h:]
    return gamma - torch.sqrt(re * re + im * im).sum(-1)


def _composition(q, table, target, kind, gamma, filt_ptr, filt_idx):
    """Row blocks of the queries: scores [b, N], the three comparisons, the filter as a mask."""
    m, n, d = q.shape[0], table.shape[0], q.shape[1]
    dev = q.device
    counts = torch.zeros((m, 3), dtype=torch.int32, device=dev)
    if m == 0 or n == 0:
        return counts
    per_row = n * max(d, 1) * q.element_size() if kind != "dot" else n * q.element_size()
    block = max(1, min(m, _BLOCK_BYTES // max(per_row, 1)))
    ids = torch.arange(n, device=dev)
    owner = None
    if filt_ptr is not None and filt_idx.numel():
        owner = torch.repeat_interleave(torch.arange(m, device=dev), (filt_ptr[1:] - filt_ptr[:-1]).long(),
                                        output_size=filt_idx.numel())
    for lo in range(0, m, block):
        hi = min(m, lo + block)
        s = _scores(q[lo:hi], table, kind, gamma)
        t = target[lo:hi].long()
        st = s.gather(1, t.unsqueeze(1))
        keep = ids.unsqueeze(0) != t.unsqueeze(1)
        if owner is not None:
            sel = (owner >= lo) & (owner < hi)
            keep[owner[sel] - lo, filt_idx[sel].long()] = False
            keep[torch.arange(hi - lo, device=dev), t] = False
        eq = (s == st) & keep
        before = ids.unsqueeze(0) < t.unsqueeze(1)
        counts[lo:hi, 0] = ((s > st) & keep).sum(1)
        counts[lo:hi, 1] = (eq & before).sum(1)
        counts[lo:hi, 2] = (eq & ~before).sum(1)
    return counts


def _sorted_lists(filt_ptr, filt_idx, m, n):
    """Per query in ascending id order, int32 (what the C entry points take).  One sort of query * N + id."""
    lengths = (filt_ptr[1:] - filt_ptr[:-1]).long()
    owner = torch.repeat_interleave(torch.arange(m, device=filt_idx.device), lengths, output_size=filt_idx.numel())
    key = torch.sort(owner * n + filt_idx.long()).values
    return filt_ptr.to(torch.int32).contiguous(), (key - (key // n) * n).to(torch.int32).contiguous()


def rank_all(q, table, target, kind, gamma=0.0, filt_ptr=None, filt_idx=None):
    """-> counts int32 [M, 3] = (greater, equal_before, equal_after); see the module docstring."""
    if kind not in KINDS:
        raise ValueError("rank_all: kind must be one of %s (got %r)" % (sorted(KINDS), kind))
    if not (torch.is_tensor(q) and torch.is_tensor(table) and torch.is_tensor(target)):
        raise ValueError("rank_all: q, table and target must be tensors")
    if q.dim() != 2 or table.dim() != 2 or q.shape[1] != table.shape[1]:
        raise ValueError("rank_all: q must be [M, D] and table [N, D] (got %s and %s)" % (tuple(q.shape), tuple(table.shape)))
    (m, d), n = q.shape, table.shape[0]
    if target.dim() != 1 or target.numel() != m or target.dtype not in (torch.int32, torch.int64):
        raise ValueError("rank_all: target must be int32 / int64 [M] (got %s %s)" % (target.dtype, tuple(target.shape)))
    if kind == "cl2" and d % 2:
        raise ValueError("rank_all: kind 'cl2' needs an even D (got %d)" % d)
    if (filt_ptr is None) != (filt_idx is None):
        raise ValueError("rank_all: filt_ptr and filt_idx go together")
    if filt_ptr is not None:
        for name, t in (("filt_ptr", filt_ptr), ("filt_idx", filt_idx)):
            if not torch.is_tensor(t) or t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
                raise ValueError("rank_all: %s must be a 1-D int32 / int64 tensor" % name)
        if filt_ptr.numel() != m + 1:
            raise ValueError("rank_all: filt_ptr must have M + 1 = %d entries (got %d)" % (m + 1, filt_ptr.numel()))
    if q.dtype != table.dtype or not q.dtype.is_floating_point:
        raise ValueError("rank_all: q and table must share a floating dtype (got %s and %s)" % (q.dtype, table.dtype))
    dev = q.device
    for t in (table, target, filt_ptr, filt_idx):
        if t is not None and t.device != dev:
            raise _lib.BackendError("rank_all: tensors on different devices: %s vs %s" % (dev, t.device))
    if dev.type not in ("cuda", "cpu"):
        raise _lib.BackendError("rank_all: no implementation for device %s" % dev)
    if max(m, n, d, 0 if filt_idx is None else filt_idx.numel()) >= 2 ** 31 - 1:
        raise _lib.BackendError("rank_all: sizes beyond int32 indexing")
    # one flag, one read-back, before anything gathers
    bad = torch.zeros((), dtype=torch.bool, device=dev)
    if m:
        bad = bad | (target.min() < 0) | (target.max() >= n)
    if filt_ptr is not None:
        bad_ptr = (filt_ptr[0] != 0) | (filt_ptr[-1] != filt_idx.numel())
        if m:
            bad_ptr = bad_ptr | ((filt_ptr[1:] - filt_ptr[:-1]).min() < 0)
        bad = bad | bad_ptr
        if filt_idx.numel():
            bad = bad | (filt_idx.min() < 0) | (filt_idx.max() >= n)
    if bool(bad):
        raise _lib.BackendError("rank_all: a target or filt_idx entry outside [0, %d), or a filt_ptr that is not non-decreasing "
                                "from 0 to len(filt_idx)" % n)
    gamma = float(gamma)
    why = None
    if q.dtype != torch.float32:
        why = "dtype %s" % q.dtype
    elif m == 0 or n == 0 or d == 0:
        why = "an empty operand: M %d, N %d, D %d" % (m, n, d)
    if why is not None:
        if dev.type == "cuda":
            _note_torch_route(why)
        return _composition(q, table, target, kind, gamma, filt_ptr, filt_idx)
    q, table = q.contiguous(), table.contiguous()
    target = target.to(torch.int32).contiguous()
    fp = fi = None
    flen = 0
    if filt_ptr is not None and filt_idx.numel():
        fp, fi = _sorted_lists(filt_ptr, filt_idx, m, n)
        flen = fi.numel()
    counts = torch.empty((m, 3), dtype=torch.int32, device=dev)
    args = (_lib.ptr(q), _lib.ptr(table), _lib.ptr(target), m, n, d, KINDS[kind], gamma, _lib.ptr(fp), _lib.ptr(fi), flen,
            _lib.ptr(counts))
    if dev.type == "cuda":
        ws, ws_bytes = _lib.workspace("cogdl_hip_kg_rank_workspace_bytes", dev, m, n, d, KINDS[kind])
        _lib.twin_call("kg_rank", dev, *args, _lib.ptr(ws), ws_bytes)
    else:
        _lib.twin_call("kg_rank", dev, *args)
    return counts


def ranks(counts, ties="stable"):
    """1-based ranks from rank_all's counts: int64 [M], or float64 for ties="mean"."""
    if ties not in TIES:
        raise ValueError("ranks: ties must be one of %s (got %r)" % (TIES, ties))
    if counts.dim() != 2 or counts.shape[1] != 3:
        raise ValueError("ranks: counts must be [M, 3] (got %s)" % (tuple(counts.shape),))
    c = counts.long()
    if ties == "stable":
        return 1 + c[:, 0] + c[:, 1]
    if ties == "optimistic":
        return 1 + c[:, 0]
    if ties == "pessimistic":
        return 1 + c[:, 0] + c[:, 1] + c[:, 2]
    return 1 + c[:, 0].double() + (c[:, 1] + c[:, 2]).double() / 2
