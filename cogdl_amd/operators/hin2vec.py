"""HIN2Vec's two costs as operators: the training rows of typed walks, and the score of a batch with its gradients.

    hin_pairs(walks, node_type, hop, negative, seed=None, *, check=True) -> (x, y, key, label)     int64 [P] each
        walks      int64 [W, L], -1 from a walk's end on (L > hop)
        node_type  int32 / int64 [N] in [0, 64)
        hop        1 .. 8: a position i pairs with i + 1 .. i + hop where position i + hop still holds a node
        negative   rows with label 0 behind every positive: one side replaced by another node of its type
        key        the packed type sequence of walk[i .. i + j]; torch.unique(key, return_inverse=True) gives dense relation ids

    hin_scores(Wx, Wr, x, y, r) -> p   float32 [B]                                              (autograd: Wx, Wr)
        p[b] = sigmoid(SUM_k Wx[x_b, k] * Wx[y_b, k] * f(Wr[r_b, k])),  f(w) = s (1 - s),  s = sigmoid(clamp(w, -6, 6))

The reference builds the rows in interpreted Python -- a list append per walk position, hop and negative, a "-".join per
positive, a rejection loop over random.choice per negative -- and scores a batch through one-hot [B, N] x [N, d] products
(cogdl/models/emb/hin2vec.py:14-117).  The law of both operators is csrc/hin2vec_law.h.

hin_pairs: walks on the GPU run three steps on the current stream (csrc/hin2vec.hip: a count kernel that stages each walk
and its types in LDS once, the library's exclusive scan, an emit kernel); walks on the CPU run the OpenMP host twin.  It is
integer arithmetic under one law: for equal inputs and seed the two return the same arrays.  Rows are in slot order, a
positive first and its negatives behind it, and do not depend on launch geometry.  A replacement is uniform over the nodes
of the replaced node's type other than the node itself, without a rejection loop; a type that occurs with a single node
cannot be corrupted (the reference loops forever) and raises BackendError before anything is launched.  The number of rows
is read back once to size the outputs, together with the flags word: check=True raises BackendError for a node id outside
[0, N), a type outside [0, 64) and a -1 that is not in a suffix; with check=False what such a call returns is unspecified
(but nothing is indexed with a refused value).

hin_scores: float32 CUDA tensors with 1 <= d <= 16384 and B, N, R >= 1 run the HIP kernels: one wave per sample forward,
f(Wr[r]) in registers, a fixed butterfly; the autograd node saves the inputs and p, nothing of size [B, d].  Backward
(once_differentiable) builds the inverted index of the 2 B node occurrences and of the B relation occurrences with one
stable torch.sort + searchsorted each and sums every table row's occurrences in ascending position, in chunks of 512 that
run on workgroups of their own and are folded in ascending chunk order; rows without occurrences are written as zeros by
the same launch; only the requested gradients are computed; there are no float atomics, so two runs give bit-equal p and
gradients.  x_b == y_b is legal.  CPU tensors, other float dtypes and empty dimensions run the torch composition
(`composition`); on the GPU that route says so once per reason with a TorchRouteWarning.  expf is not bit-equal across two
libms, so the scorer has no host twin.  Ids outside their table raise BackendError (one flag read-back; check=False skips it:
such a sample scores NaN and contributes to no gradient).

Not for use under torch.cuda.graph capture: hin_pairs reads its size back, the backward of hin_scores sorts and allocates.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .kgscore import inverted_index
from .ops import _ROUTE_NOTED, TorchRouteWarning
from .walk import _seed

MAX_HOP, MAX_TYPES, MAX_D, CHUNK = 8, 64, 16384, 512  # cogdl_hin2vec::kMaxHop, kMaxTypes, kMaxD, kChunk

_FLAG_TEXT = ((1, "a walk entry is neither -1 nor a node id in [0, N)"), (2, "a node type lies outside [0, 64)"),
              (4, "a -1 is followed by a node: -1 must be a suffix of its walk"),
              (8, "a type's node list cannot give a replacement"))


def _raise_for_flags(flags):
    if flags:
        raise _lib.BackendError("hin_pairs: %s" % "; ".join(t for bit, t in _FLAG_TEXT if flags & bit))


def type_tables(node_type):
    """node_type int [N] in [0, 64) -> (type_ptr int32 [65], type_nodes int32 [N], rank int32 [N]): the node ids grouped by type
    (ascending inside a type: one stable sort) and each node's place in its group."""
    n = node_type.numel()
    types, nodes = torch.sort(node_type.long(), stable=True)
    counts = torch.bincount(types.clamp(0, MAX_TYPES - 1), minlength=MAX_TYPES)
    type_ptr = torch.zeros(MAX_TYPES + 1, dtype=torch.long, device=node_type.device)
    torch.cumsum(counts, 0, out=type_ptr[1:])
    rank = torch.empty(n, dtype=torch.long, device=node_type.device)
    rank[nodes] = torch.arange(n, device=node_type.device) - type_ptr[types.clamp(0, MAX_TYPES - 1)]
    return type_ptr.to(torch.int32), nodes.to(torch.int32).contiguous(), rank.to(torch.int32), counts


def hin_pairs(walks, node_type, hop, negative, seed=None, *, check=True):
    """-> (x, y, key, label), int64 [P] each on the device of `walks`; see the module docstring."""
    if not torch.is_tensor(walks) or walks.dim() != 2 or walks.dtype != torch.int64:
        raise ValueError("hin_pairs: walks must be an int64 [W, L] tensor")
    if not torch.is_tensor(node_type) or node_type.dim() != 1 or node_type.dtype not in (torch.int32, torch.int64):
        raise ValueError("hin_pairs: node_type must be an int32 / int64 [N] tensor")
    hop, negative = int(hop), int(negative)
    (w, length), n, dev = walks.shape, node_type.numel(), walks.device
    if not 1 <= hop <= MAX_HOP:
        raise ValueError("hin_pairs: hop must be in [1, %d] (got %d)" % (MAX_HOP, hop))
    if length <= hop:
        raise ValueError("hin_pairs: walks of length %d are not longer than hop %d" % (length, hop))
    if negative < 0:
        raise ValueError("hin_pairs: negative must not be negative (got %d)" % negative)
    if node_type.device != dev:
        raise _lib.BackendError("hin_pairs: tensors on different devices: %s vs %s" % (dev, node_type.device))
    if dev.type not in ("cuda", "cpu"):
        raise _lib.BackendError("hin_pairs: no implementation for device %s" % dev)
    if n >= 2 ** 31 - 1:
        raise _lib.BackendError("hin_pairs: node ids beyond int32")
    seed = _seed(seed)
    empty = tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(4))
    if w == 0:
        return empty
    walks = walks.contiguous()
    if check and n and bool((node_type.min() < 0) | (node_type.max() >= MAX_TYPES)):
        _raise_for_flags(2)
    type32 = node_type.to(torch.int32).contiguous()
    type_ptr, type_nodes, rank, counts = type_tables(node_type)
    if negative and bool((counts == 1).any()):  # (the tiny read-back: the reference loops forever here)
        raise _lib.BackendError("hin_pairs: a node type occurs with a single node: it has no other node to be replaced by")
    words = _lib.hip().cogdl_hip_hin_pairs_scratch_words(w) if dev.type == "cuda" else 0
    offsets = torch.empty(w + 1, dtype=torch.int64, device=dev)
    scratch = torch.empty(words, dtype=torch.int64, device=dev) if words else None
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.twin_call("hin_pairs_count", dev, _lib.ptr(walks), w, length, hop, _lib.ptr(type32), n, _lib.ptr(offsets),
                   _lib.ptr(scratch), _lib.ptr(flags))
    total, raised = torch.stack([offsets[w], flags[0].long()]).tolist()  # the one read-back
    if check:
        _raise_for_flags(raised)
    if total == 0:
        return empty
    x, y, key, label = (torch.empty(total * (1 + negative), dtype=torch.int64, device=dev) for _ in range(4))
    _lib.twin_call("hin_pairs_emit", dev, _lib.ptr(walks), w, length, hop, negative, _lib.ptr(type32), _lib.ptr(type_ptr),
                   _lib.ptr(type_nodes), _lib.ptr(rank), n, seed, _lib.ptr(offsets), total, _lib.ptr(x), _lib.ptr(y),
                   _lib.ptr(key), _lib.ptr(label), _lib.ptr(flags))
    return x, y, key, label


def regularise(w):
    """f(w) = s (1 - s), s = sigmoid(clamp(w, -6, 6)): the reference's `regulartion`."""
    s = torch.sigmoid(torch.clamp(w, -6.0, 6.0))
    return s * (1 - s)


def composition(Wx, Wr, x, y, r):
    """The score as a torch gather composition (the alternative route, and the tests' reference in float64)."""
    if Wx.shape[0] == 0 or Wr.shape[0] == 0:
        return Wx.new_full((x.numel(),), float("nan")) + 0 * (Wx.sum() + Wr.sum())
    return torch.sigmoid((Wx[x.long()] * Wx[y.long()] * regularise(Wr[r.long()])).sum(1))


def _note_torch_route(why):
    if ("hin_scores", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("hin_scores", why))
    import warnings

    warnings.warn("cogdl_amd.operators.hin2vec.hin_scores: GPU tensors on the torch route (%s): the gather composition on "
                  "torch's kernels; the HIP kernels cover float32 with B, N, R of at least 1 and d in 1 .. %d" % (why, MAX_D),
                  TorchRouteWarning, stacklevel=3)


def _chunk_ptr(occ_ptr):
    """occ_ptr int32 [rows + 1] -> int32 [rows + 1]: the running number of 512-chunks, every row counting at least one."""
    cnt = (occ_ptr[1:] - occ_ptr[:-1]).long()
    out = torch.zeros(occ_ptr.numel(), dtype=torch.long, device=occ_ptr.device)
    torch.cumsum(((cnt + (CHUNK - 1)) // CHUNK).clamp_(min=1), 0, out=out[1:])
    return out.to(torch.int32)


class _HinScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Wx, Wr, x, y, r):
        Wx, Wr = Wx.contiguous(), Wr.contiguous()
        (n, d), rel, b = Wx.shape, Wr.shape[0], x.numel()
        p = torch.empty(b, dtype=torch.float32, device=Wx.device)
        with _lib.on_device(Wx.device):
            rc = _lib.hip().cogdl_hip_hin_score(_lib.ptr(Wx), _lib.ptr(Wr), _lib.ptr(x), _lib.ptr(y), _lib.ptr(r), b, n, rel, d,
                                                _lib.ptr(p), _lib.stream_of(Wx))
        _lib.check(rc, "hin_score")
        ctx.save_for_backward(Wx, Wr, x, y, r, p)
        return p

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        Wx, Wr, x, y, r, p = ctx.saved_tensors
        (n, d), rel, b = Wx.shape, Wr.shape[0], x.numel()
        g = g.contiguous()
        grads = [None, None]
        for relation, (table, ids) in enumerate(((Wx, None), (Wr, r))):
            if not ctx.needs_input_grad[relation]:
                continue
            ids = torch.cat([x, y]) if ids is None else ids
            rows = table.shape[0]
            occ_ptr, occ_pos = inverted_index(ids, rows)
            chunk_ptr = _chunk_ptr(occ_ptr)
            slots = ids.numel() // CHUNK
            grad = torch.empty_like(table)  # (every row is written, zeros included)
            partials = torch.empty((slots, d), dtype=torch.float32, device=table.device) if slots else None
            with _lib.on_device(table.device):
                rc = _lib.hip().cogdl_hip_hin_score_grad(_lib.ptr(Wx), _lib.ptr(Wr), _lib.ptr(x), _lib.ptr(y), _lib.ptr(r),
                                                         _lib.ptr(p), _lib.ptr(g), _lib.ptr(occ_ptr), _lib.ptr(occ_pos),
                                                         _lib.ptr(chunk_ptr), b, n, rel, d, relation, _lib.ptr(grad),
                                                         _lib.ptr(partials), slots, _lib.stream_of(table))
            _lib.check(rc, "hin_score_grad")
            grads[relation] = grad
        return grads[0], grads[1], None, None, None


def hin_scores(Wx, Wr, x, y, r, *, check=True):
    """-> p float32 [B] with gradients for Wx and Wr; see the module docstring.  Not for use under torch.cuda.graph capture."""
    if not all(torch.is_tensor(t) for t in (Wx, Wr, x, y, r)):
        raise ValueError("hin_scores: Wx, Wr, x, y and r must be tensors")
    if Wx.dim() != 2 or Wr.dim() != 2 or Wx.shape[1] != Wr.shape[1]:
        raise ValueError("hin_scores: Wx must be [N, d] and Wr [R, d] (got %s and %s)" % (tuple(Wx.shape), tuple(Wr.shape)))
    if Wx.dtype != Wr.dtype or not Wx.dtype.is_floating_point:
        raise ValueError("hin_scores: Wx and Wr must share a floating dtype (got %s and %s)" % (Wx.dtype, Wr.dtype))
    b = x.numel()
    for name, t in (("x", x), ("y", y), ("r", r)):
        if t.dim() != 1 or t.numel() != b or t.dtype not in (torch.int32, torch.int64):
            raise ValueError("hin_scores: %s must be an int32 / int64 [B] tensor" % name)
    dev = Wx.device
    for t in (Wr, x, y, r):
        if t.device != dev:
            raise _lib.BackendError("hin_scores: tensors on different devices: %s vs %s" % (dev, t.device))
    if dev.type not in ("cuda", "cpu"):
        raise _lib.BackendError("hin_scores: no implementation for device %s" % dev)
    (n, d), rel = Wx.shape, Wr.shape[0]
    if max(b, n, rel) >= 2 ** 30 - 1:
        raise _lib.BackendError("hin_scores: sizes beyond int32 indexing")
    if check and b:  # one flag, one read-back, before anything gathers
        nodes = torch.cat([x, y])
        if bool((nodes.min() < 0) | (nodes.max() >= n) | (r.min() < 0) | (r.max() >= rel)):
            raise _lib.BackendError("hin_scores: an id outside its table (x, y in [0, %d), r in [0, %d))" % (n, rel))
    why = None
    if dev.type == "cpu":
        why = "cpu"
    elif Wx.dtype != torch.float32:
        why = "dtype %s" % Wx.dtype
    elif b == 0 or n == 0 or rel == 0 or d == 0:
        why = "an empty operand: B %d, N %d, R %d, d %d" % (b, n, rel, d)
    elif d > MAX_D:
        why = "d %d above %d" % (d, MAX_D)
    if why is not None:
        if dev.type == "cuda":
            _note_torch_route(why)
        return composition(Wx, Wr, x, y, r)
    ids = [t.clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous() if t.dtype != torch.int32 else t.contiguous() for t in (x, y, r)]
    return _HinScores.apply(Wx, Wr, *ids)
