"""The multiplex (typed-edge) attention embedding of GATNE as one operator: GATNEModel.forward (cogdl/models/emb/gatne.py:221-241)
with the neighbour rows looked up through `inputs`.

    multiplex_embed(node_emb, type_emb, trans_w, att_w1, att_w2, neigh, inputs, types, *, check=True) -> out [B, D]
        node_emb [N, D]      float   base embeddings                              (autograd)
        type_emb [N, T, U]   float   one U-vector per node and edge type          (autograd)
        trans_w  [T, U, D]   float   type-specific projection                     (autograd)
        att_w1   [T, U, A]   float   attention, first layer                       (autograd)
        att_w2   [T, A]      float   attention, second layer                      (autograd)
        neigh    [N, T, S]   int32 / int64 in [0, N): S sampled neighbours per node and type
        inputs   [B]         int32 / int64 in [0, N)
        types    [B]         int32 / int64 in [0, T)
    For sample b, x = inputs[b], t = types[b]:
        c[i, :] = SUM_s type_emb[neigh[x, i, s], i, :]        h = tanh(c att_w1[t])        e = h att_w2[t]
        att = softmax_i(e)        m = att c        y = node_emb[x] + m trans_w[t]        out[b] = y / max(||y||_2, 1e-12)
    B == 1 and T == 1 are served (the reference's module raises for both: a squeeze()).

The reference evaluates type_emb[neigh[inputs]], a [B, T, S, T, U] gather of which it keeps the diagonal, runs about fifteen small
kernels on it, saves all of it for autograd and scatters [B, T, S, T, U] gradient rows into the table with float atomics.  Here
float32 CUDA tensors run csrc/multiplex.hip: the forward is one launch (one wave per sample), nothing of size [B, T, S, U] exists,
and the autograd node saves c [B, T, U], h [B, T, A], att [B, T], m [B, U], the norm [B] and out.  Backward is a per-sample kernel
(g_y, g_c, g_pre, g_e) and up to three list kernels: the weight gradients sum the samples of each type in ascending b, grad
node_emb the occurrences of a node in inputs in ascending b, grad type_emb the neighbour slots that name (node, type) in ascending
b S + s -- all through one inverted index (operators/kgscore.py: inverted_index, one stable sort per call), in chunks of 128 as
csrc/multiplex_law.h states.  No float atomics: results are equal bit for bit from run to run and do not depend on the batch a
sample sits in.  Every element of every gradient is written; a type absent from the batch and a node nothing refers to get exact
+0.  Backward computes only the gradients that are asked for and is once_differentiable.

Where y == 0 the output is exactly 0 and the gradient is torch's: g / 1e-12 (clamp_min passes nothing to the norm there).

Routes.  CPU tensors, other floating dtypes, empty operands and shapes beyond the kernels' limits (T <= 16, S, U, A <= 64,
D <= 1024) run `composition`, the reference's arithmetic on torch; on the GPU that route says so once per reason with a
TorchRouteWarning.  There is no host twin: tanh and exp are not bit-equal across two libms.

check=True validates inputs, types and neigh with one flag read-back before anything is gathered and raises BackendError;
check=False skips the read-back: a sample whose input, type or any of its T S neighbour ids is out of range gives a NaN row and
contributes to no gradient.  No id is followed unchecked on either route.  Mismatched shapes and dtypes raise ValueError, tensors
on different devices BackendError.

Not for use under torch.cuda.graph capture (the validation reads a flag, the backward sorts and allocates).
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib

# (operators/ops.py and operators/kgscore.py load libcogdl_hip.so when they are imported: the GPU routes import them where they
# run, so that CPU tensors never load the library)
MAX_T, MAX_S, MAX_U, MAX_A, MAX_D = 16, 64, 64, 64, 1024  # cogdl_multiplex::kMax*: what one wave holds
EPS = 1e-12


def _note_torch_route(why):
    from .ops import _ROUTE_NOTED, TorchRouteWarning

    if ("multiplex_embed", why) in _ROUTE_NOTED:
        return
    _ROUTE_NOTED.add(("multiplex_embed", why))
    import warnings

    warnings.warn("cogdl_amd.operators.multiplex.multiplex_embed: GPU tensors on the torch route (%s): the [B, T, S, T, U] gather "
                  "composition on torch's kernels; the HIP kernels cover float32 with T in 1 .. %d, S, U, A in 1 .. %d, "
                  "D in 1 .. %d and B, N of at least 1" % (why, MAX_T, MAX_S, MAX_D), TorchRouteWarning, stacklevel=3)


def composition(node_emb, type_emb, trans_w, att_w1, att_w2, neigh, inputs, types):
    """The reference's arithmetic: the [B, T, S, T, U] gather, its diagonal, matmuls, softmax, normalize.  A sample with an id
    outside its range gives a NaN row without a gradient."""
    (n, t_count, u_dim), d, b = type_emb.shape, node_emb.shape[1], inputs.shape[0]
    floats = (node_emb, type_emb, trans_w, att_w1, att_w2)
    if b == 0 or d == 0:
        return node_emb.new_zeros((b, d)) + 0 * sum(f.sum() for f in floats)
    if n == 0 or t_count == 0:
        return node_emb.new_full((b, d), float("nan")) + 0 * sum(f.sum() for f in floats)
    x, t = inputs.long(), types.long()
    valid = (x >= 0) & (x < n) & (t >= 0) & (t < t_count)
    x, t = x.clamp(0, n - 1), t.clamp(0, t_count - 1)
    nb = neigh[x].long()  # [B, T, S]
    if nb.shape[2]:
        valid = valid & ((nb >= 0) & (nb < n)).all(2).all(1)
    nb = nb.clamp(0, n - 1)
    # (index_select, not table[ids]: the same gather, and on the CPU its backward adds rows one after the other, so a CPU run
    # repeats bit for bit)
    block = type_emb.index_select(0, nb.reshape(-1)).view(tuple(nb.shape) + (t_count, u_dim))  # [B, T, S, T, U]
    c = torch.cat([block[:, i, :, i, :].unsqueeze(1) for i in range(t_count)], dim=1).sum(dim=2)  # [B, T, U]
    h = torch.tanh(torch.matmul(c, att_w1.index_select(0, t)))  # [B, T, A]
    e = torch.matmul(h, att_w2.index_select(0, t).unsqueeze(2)).squeeze(2)  # [B, T]
    att = torch.softmax(e, dim=1).unsqueeze(1)  # [B, 1, T]
    m = torch.matmul(att, c)  # [B, 1, U]
    y = node_emb.index_select(0, x) + torch.matmul(m, trans_w.index_select(0, t)).squeeze(1)
    out = torch.nn.functional.normalize(y, dim=1, eps=EPS)
    return torch.where(valid.unsqueeze(1), out, out.new_full((), float("nan")))


class _MultiplexEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, node_emb, type_emb, trans_w, att_w1, att_w2, neigh32, inputs32, types32, checked):
        node_emb, type_emb = node_emb.contiguous(), type_emb.contiguous()
        trans_w, att_w1, att_w2 = trans_w.contiguous(), att_w1.contiguous(), att_w2.contiguous()
        (n, t, u), d, a, s, b = type_emb.shape, node_emb.shape[1], att_w1.shape[2], neigh32.shape[2], inputs32.shape[0]
        dev = node_emb.device
        f32 = dict(dtype=torch.float32, device=dev)
        c, h = torch.empty((b, t, u), **f32), torch.empty((b, t, a), **f32)
        att, m, nrm = torch.empty((b, t), **f32), torch.empty((b, u), **f32), torch.empty((b,), **f32)
        out = torch.empty((b, d), **f32)
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_multiplex_fwd(_lib.ptr(node_emb), _lib.ptr(type_emb), _lib.ptr(trans_w), _lib.ptr(att_w1),
                                                    _lib.ptr(att_w2), _lib.ptr(neigh32), _lib.ptr(inputs32), _lib.ptr(types32), b, n, t,
                                                    s, u, a, d, _lib.ptr(c), _lib.ptr(h), _lib.ptr(att), _lib.ptr(m), _lib.ptr(nrm),
                                                    _lib.ptr(out), _lib.stream_of(out))
        _lib.check(rc, "multiplex_fwd")
        ctx.save_for_backward(trans_w, att_w1, att_w2, neigh32, inputs32, types32, c, h, att, m, nrm, out)
        ctx.sizes, ctx.checked = (b, n, t, s, u, a, d), checked
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        trans_w, att_w1, att_w2, neigh32, inputs32, types32, c, h, att, m, nrm, out = ctx.saved_tensors
        b, n, t, s, u, a, d = ctx.sizes
        need_node, need_type, need_trans, need_w1, need_w2 = ctx.needs_input_grad[:5]
        if not (need_node or need_type or need_trans or need_w1 or need_w2):
            return (None,) * 9
        if g.dtype != torch.float32:
            raise _lib.BackendError("multiplex_embed backward: grad must be float32 (got %s)" % g.dtype)
        from .kgscore import inverted_index

        dev, lib = out.device, _lib.hip()
        g = g.contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        g_y, g_c = torch.empty((b, d), **f32), torch.empty((b, t, u), **f32)
        g_pre, g_e = torch.empty((b, t, a), **f32), torch.empty((b, t), **f32)
        stream = _lib.stream_of(out)
        with _lib.on_device(dev):
            rc = lib.cogdl_hip_multiplex_bwd_sample(_lib.ptr(trans_w), _lib.ptr(att_w1), _lib.ptr(att_w2), _lib.ptr(types32),
                                                    _lib.ptr(g), _lib.ptr(out), _lib.ptr(nrm), _lib.ptr(c), _lib.ptr(h),
                                                    _lib.ptr(att), b, t, u, a, d, _lib.ptr(g_y), _lib.ptr(g_c), _lib.ptr(g_pre),
                                                    _lib.ptr(g_e), stream)
        _lib.check(rc, "multiplex_bwd_sample")
        # One inverted index for every list that is needed.  Keys: n T + i for the neighbour slots (position (b T + i) S + s),
        # N T + inputs[b], N T + N + types[b]; a sample the forward refused (nrm < 0) is keyed -1: it is in no list.
        refused = None if ctx.checked else nrm < 0
        parts, base = [], {}
        pos = 0
        if need_type:
            x = inputs32.long() if ctx.checked else inputs32.long().clamp(0, n - 1)
            keys = neigh32[x] * t + torch.arange(t, dtype=torch.int32, device=dev).view(1, t, 1)
            if refused is not None:
                keys = torch.where(refused.view(b, 1, 1), keys.new_full((), -1), keys)
            parts.append(keys.reshape(-1))
            base["type"], pos = pos, pos + b * t * s
        if need_node:
            keys = inputs32 + n * t
            parts.append(keys if refused is None else torch.where(refused, keys.new_full((), -1), keys))
            base["node"], pos = pos, pos + b
        if need_trans or need_w1 or need_w2:
            keys = types32 + (n * t + n)
            parts.append(keys if refused is None else torch.where(refused, keys.new_full((), -1), keys))
            base["weights"], pos = pos, pos + b
        occ_ptr, occ_pos = inverted_index(parts[0] if len(parts) == 1 else torch.cat(parts), n * t + n + t)
        ptr0 = occ_ptr.data_ptr()
        g_node = g_type = g_trans = g_w1 = g_w2 = None
        with _lib.on_device(dev):
            if need_type:
                g_type = torch.empty((n, t, u), **f32)
                rc = lib.cogdl_hip_multiplex_bwd_type(_lib.ptr(g_c), ptr0, _lib.ptr(occ_pos), base["type"], pos, b, n, t, s, u,
                                                      _lib.ptr(g_type), stream)
                _lib.check(rc, "multiplex_bwd_type")
            if need_node:
                g_node = torch.empty((n, d), **f32)
                rc = lib.cogdl_hip_multiplex_bwd_node(_lib.ptr(g_y), ptr0 + 4 * n * t, _lib.ptr(occ_pos), base["node"], pos, b, n, d,
                                                      _lib.ptr(g_node), stream)
                _lib.check(rc, "multiplex_bwd_node")
            if need_trans or need_w1 or need_w2:
                g_trans = torch.empty_like(trans_w) if need_trans else None
                g_w1 = torch.empty_like(att_w1) if need_w1 else None
                g_w2 = torch.empty_like(att_w2) if need_w2 else None
                rc = lib.cogdl_hip_multiplex_bwd_weights(_lib.ptr(m), _lib.ptr(g_y), _lib.ptr(c), _lib.ptr(g_pre), _lib.ptr(g_e),
                                                         _lib.ptr(h), ptr0 + 4 * (n * t + n), _lib.ptr(occ_pos), base["weights"],
                                                         pos, b, t, u, a, d, _lib.ptr(g_trans), _lib.ptr(g_w1), _lib.ptr(g_w2),
                                                         stream)
                _lib.check(rc, "multiplex_bwd_weights")
        return g_node, g_type, g_trans, g_w1, g_w2, None, None, None, None


def _ids32(t):
    """ids as contiguous int32 (ids beyond int32 are out of range of any table the kernels index: keep them so)"""
    if t.dtype != torch.int32:
        t = t.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return t.contiguous()


def multiplex_embed(node_emb, type_emb, trans_w, att_w1, att_w2, neigh, inputs, types, *, check=True):
    """-> out [B, D] with gradients for the five float operands; see the module docstring.  Not for use under
    torch.cuda.graph capture."""
    floats, ints = (node_emb, type_emb, trans_w, att_w1, att_w2), (neigh, inputs, types)
    if not all(torch.is_tensor(x) for x in floats + ints):
        raise ValueError("multiplex_embed: every operand must be a tensor")
    if node_emb.dim() != 2 or type_emb.dim() != 3 or trans_w.dim() != 3 or att_w1.dim() != 3 or att_w2.dim() != 2:
        raise ValueError("multiplex_embed: node_emb [N, D], type_emb [N, T, U], trans_w [T, U, D], att_w1 [T, U, A], att_w2 [T, A] "
                         "(got %s)" % ", ".join(str(tuple(x.shape)) for x in floats))
    (n, d), (_, t, u), a = node_emb.shape, type_emb.shape, att_w1.shape[2]
    if type_emb.shape[0] != n or tuple(trans_w.shape) != (t, u, d) or tuple(att_w1.shape[:2]) != (t, u) or \
            tuple(att_w2.shape) != (t, a):
        raise ValueError("multiplex_embed: node_emb [N, D], type_emb [N, T, U], trans_w [T, U, D], att_w1 [T, U, A], att_w2 [T, A] "
                         "(got %s)" % ", ".join(str(tuple(x.shape)) for x in floats))
    if neigh.dim() != 3 or tuple(neigh.shape[:2]) != (n, t) or neigh.dtype not in (torch.int32, torch.int64):
        raise ValueError("multiplex_embed: neigh must be int32 / int64 [N, T, S] (got %s %s)" % (neigh.dtype, tuple(neigh.shape)))
    s = neigh.shape[2]
    if inputs.dim() != 1 or types.dim() != 1 or inputs.shape != types.shape:
        raise ValueError("multiplex_embed: inputs and types must be [B] (got %s and %s)" % (tuple(inputs.shape), tuple(types.shape)))
    for x in (inputs, types):
        if x.dtype not in (torch.int32, torch.int64):
            raise ValueError("multiplex_embed: inputs and types must be int32 / int64 (got %s)" % x.dtype)
    b = inputs.shape[0]
    if not node_emb.dtype.is_floating_point or any(x.dtype != node_emb.dtype for x in floats):
        raise ValueError("multiplex_embed: the five float operands must share a floating dtype (got %s)"
                         % ", ".join(str(x.dtype) for x in floats))
    dev = node_emb.device
    for x in floats[1:] + ints:
        if x.device != dev:
            raise _lib.BackendError("multiplex_embed: tensors on different devices: %s vs %s" % (dev, x.device))
    if dev.type not in ("cuda", "cpu"):
        raise _lib.BackendError("multiplex_embed: no implementation for device %s" % dev)
    if check and b:  # one flag, one read-back, before anything gathers
        bad = (inputs.min() < 0) | (inputs.max() >= n) | (types.min() < 0) | (types.max() >= t)
        if neigh.numel():
            bad = bad | (neigh.min() < 0) | (neigh.max() >= n)
        if bool(bad):
            raise _lib.BackendError("multiplex_embed: an id outside its range (inputs and neigh in [0, %d), types in [0, %d))" % (n, t))
    if dev.type == "cpu":
        return composition(node_emb, type_emb, trans_w, att_w1, att_w2, neigh, inputs, types)
    why = None
    if node_emb.dtype != torch.float32:
        why = "dtype %s" % node_emb.dtype
    elif min(b, n, t, s, u, a, d) == 0:
        why = "an empty operand: B %d, N %d, T %d, S %d, U %d, A %d, D %d" % (b, n, t, s, u, a, d)
    elif t > MAX_T or s > MAX_S or u > MAX_U or a > MAX_A or d > MAX_D:
        why = "T %d, S %d, U %d, A %d, D %d beyond %d, %d, %d, %d, %d" % (t, s, u, a, d, MAX_T, MAX_S, MAX_U, MAX_A, MAX_D)
    elif b * t * s + 2 * b >= 2 ** 31 - 1 or n * t + n + t >= 2 ** 31 - 1:
        why = "sizes beyond int32 indexing"
    if why is not None:
        _note_torch_route(why)
        return composition(node_emb, type_emb, trans_w, att_w1, att_w2, neigh, inputs, types)
    return _MultiplexEmbed.apply(node_emb, type_emb, trans_w, att_w1, att_w2, _ids32(neigh), _ids32(inputs), _ids32(types),
                                 bool(check))
