"""Activation compression: what a layer keeps for its backward pass, in 1 / 2 / 4 / 8 bits per element, one bit per element,
or not at all (the ActNN family of the reference: cogdl/operators/linear.py, operators/spmm.py:89-133, layers/act*_layer.py).

    quantize(x, bits=2, group=256, seed=None, call=None) -> Quantized(codes, meta, bits, group, numel, dtype)
    dequantize(q, shape)                                  -> tensor of q.dtype
    relu_packed(x)                                        torch.relu; the backward reads a mask of one bit per element
    dropout_regen(x, p, training=True)                    dropout; the backward regenerates the mask from (seed, call, p)
    linear_q(x, weight, bias=None, bits=None, group=None) F.linear; the input is saved quantised

The law is csrc/actq_law.h: the tensor is quantised as its row-major flattening in groups of `group` elements (64, 128 or 256),
each with one float32 (min, step) pair; the code of an element is rounded stochastically with a Philox draw selected by
(seed, call, element index); |dequantised - x| <= step up to float rounding (error_bound below is the header's formula), and
the expectation is x.  A group that holds a NaN or an infinity, or whose range overflows float32, dequantises to NaN.  CUDA
tensors run the HIP kernels (csrc/actq.hip), CPU tensors the OpenMP host twin; the bytes are equal.  float16 / bfloat16 inputs
are converted to float32 before quantising and back after dequantising.  A contiguous view that starts mid-allocation is read
where it is (the kernels take 4-byte lanes for it; same bytes).

Seeds.  With seed=None the key is torch.initial_seed() and `call` comes from a per-process counter that restarts whenever
initial_seed changes: torch.manual_seed(s) with a new s reproduces a run (reset_draws() restarts it for the same s).  One
counter serves the quantiser and the dropout, so no two uses share a draw.  A captured graph would replay one draw: do not
capture a training step that uses these operators.
"""
import collections

import torch

from .. import _lib

BITS = (1, 2, 4, 8)
GROUPS = (64, 128, 256)
_MASK64 = 2 ** 64 - 1
_FLOATS = (torch.float32, torch.float16, torch.bfloat16)

Quantized = collections.namedtuple("Quantized", "codes meta bits group numel dtype")

_DRAWS = {"seed": None, "call": 0}


def reset_draws():
    """Restart the per-process call counter (as a change of torch.initial_seed() does)."""
    _DRAWS["seed"], _DRAWS["call"] = None, 0


def next_draw():
    """(seed, call) of the next use: seed = torch.initial_seed(), call = how many uses came before under that seed."""
    seed = torch.initial_seed() & _MASK64
    if seed != _DRAWS["seed"]:
        _DRAWS["seed"], _DRAWS["call"] = seed, 0
    call = _DRAWS["call"]
    _DRAWS["call"] = call + 1
    return seed, call


def _draw(seed, call):
    if seed is None:
        return next_draw()
    return int(seed) & _MASK64, (0 if call is None else int(call)) & _MASK64


def _device_of(t, what):
    if t.device.type not in ("cuda", "cpu"):
        raise _lib.BackendError("%s: no implementation for device %s" % (what, t.device))
    return t.device


def _f32(x, what):
    if not torch.is_tensor(x) or x.dtype not in _FLOATS:
        raise _lib.BackendError("%s: a float32 / float16 / bfloat16 tensor is needed (got %s)"
                                % (what, getattr(x, "dtype", type(x))))
    x = x.detach()
    return (x if x.dtype == torch.float32 else x.float()).contiguous()


def code_words(n, bits):
    return (n * bits + 31) // 32


def error_bound(mn, step, bits):
    """csrc/actq_law.h's bound of |dequantised - x| for the elements of a finite group, from its stored (mn, step), in
    float64: step (1 + 16 L U) + 2 U max(|mn|, |mn + L step|) + 2^-119 with L = 2^bits - 1, U = 2^-24."""
    L, U = float(2 ** bits - 1), 2.0 ** -24
    mn, step = mn.double(), step.double()
    return step * (1.0 + 16.0 * L * U) + 2.0 * U * torch.maximum(mn.abs(), (mn + L * step).abs()) + 2.0 ** -119


def quantize(x, bits=2, group=256, seed=None, call=None):
    """-> Quantized: codes int32 [ceil(n bits / 32)] (the law's uint32 words), meta float32 [ceil(n / group), 2]."""
    bits, group = int(bits), int(group)
    if bits not in BITS or group not in GROUPS:
        raise ValueError("quantize: bits must be one of %s and group one of %s (got %d, %d)" % (BITS, GROUPS, bits, group))
    dev = _device_of(x, "quantize")
    xf = _f32(x, "quantize")
    n = xf.numel()
    seed, call = _draw(seed, call)
    codes = torch.empty(code_words(n, bits), dtype=torch.int32, device=dev)
    meta = torch.empty(((n + group - 1) // group, 2), dtype=torch.float32, device=dev)
    if n:
        _lib.twin_call("actq_quantize", dev, _lib.ptr(xf), n, bits, group, seed, call, _lib.ptr(codes), _lib.ptr(meta))
    return Quantized(codes, meta, bits, group, n, x.dtype)


def dequantize(q, shape):
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    if n != q.numel:
        raise ValueError("dequantize: shape %s does not hold %d elements" % (shape, q.numel))
    dev = q.codes.device
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    if n:
        _lib.twin_call("actq_dequantize", dev, _lib.ptr(q.codes), _lib.ptr(q.meta), n, q.bits, q.group, _lib.ptr(out))
    return out if q.dtype == torch.float32 else out.to(q.dtype)


def relu_mask(x):
    """(relu(x) float32, mask int64 [ceil(n / 64)]) for a float32 tensor; no autograd."""
    dev = _device_of(x, "relu_mask")
    xf = _f32(x, "relu_mask")
    n = xf.numel()
    y = torch.empty_like(xf)
    mask = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    if n:
        _lib.twin_call("relu_mask", dev, _lib.ptr(xf), n, _lib.ptr(y), _lib.ptr(mask))
    return y, mask


def mask_apply(g, mask):
    dev = _device_of(g, "mask_apply")
    gf = _f32(g, "mask_apply")
    n = gf.numel()
    if mask.dtype != torch.int64 or mask.numel() != (n + 63) // 64 or mask.device != dev or not mask.is_contiguous():
        raise _lib.BackendError("mask_apply: the mask must be a contiguous int64 [%d] tensor on %s" % ((n + 63) // 64, dev))
    out = torch.empty_like(gf)
    if n:
        _lib.twin_call("mask_apply", dev, _lib.ptr(gf), _lib.ptr(mask), n, _lib.ptr(out))
    return out


def drop_params(p):
    """(thresh, scale) of csrc/philox.h's drop_params: thresh = round(p 65536) in [0, 65536], scale = 65536 / (65536 - thresh)."""
    t = min(max(float(p) * 65536.0, 0.0), 65536.0)
    thresh = int(t + 0.5)
    return thresh, (0.0 if thresh >= 65536 else 65536.0 / (65536 - thresh))


def drop_apply(x, seed, call, thresh, scale):
    """keep(seed, call, i) ? x[i] * scale : 0 as a new float32 tensor; no autograd.  Forward and backward of the dropout."""
    dev = _device_of(x, "drop_apply")
    xf = _f32(x, "drop_apply")
    n = xf.numel()
    y = torch.empty_like(xf)
    if n:
        _lib.twin_call("drop_apply", dev, _lib.ptr(xf), n, int(seed) & _MASK64, int(call) & _MASK64, int(thresh), float(scale),
                       _lib.ptr(y))
    return y


class _ReluPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y, mask = relu_mask(x)
        ctx.save_for_backward(mask)
        return y if x.dtype == torch.float32 else y.to(x.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        (mask,) = ctx.saved_tensors
        g = mask_apply(grad_out, mask)
        return g if grad_out.dtype == torch.float32 else g.to(grad_out.dtype)


def relu_packed(x):
    return _ReluPacked.apply(x)


class _DropoutRegen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, thresh, scale, seed, call):
        ctx.draw = (seed, call, thresh, scale)
        y = drop_apply(x, seed, call, thresh, scale)
        return y if x.dtype == torch.float32 else y.to(x.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        g = drop_apply(grad_out, *ctx.draw)
        return (g if grad_out.dtype == torch.float32 else g.to(grad_out.dtype)), None, None, None, None


def dropout_regen(x, p=0.5, training=True, seed=None, call=None):
    if not training:
        return x
    thresh, scale = drop_params(p)
    seed, call = _draw(seed, call)
    return _DropoutRegen.apply(x, thresh, scale, seed, call)


def _wgrad_kernel_serves(x, grad_out):
    from .. import linear as _linear

    return (torch.nn.functional.linear is _linear.linear and x.is_cuda and x.dtype == torch.float32
            and grad_out.dtype == torch.float32 and x.shape[0] >= _linear.MIN_ROWS
            and max(x.shape[1], grad_out.shape[1]) <= _linear.MAX_FEATURES)


class _LinearQ(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bits, group):
        ctx.q = quantize(x, bits, group) if ctx.needs_input_grad[1] else None
        ctx.x_shape = tuple(x.shape)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(weight)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, grad_out):
        (weight,) = ctx.saved_tensors
        g = grad_out.reshape(-1, grad_out.shape[-1])
        grad_x = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_x = g.mm(weight.to(g.dtype)).reshape(ctx.x_shape)
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            x_hat = dequantize(ctx.q, ctx.x_shape).reshape(-1, ctx.x_shape[-1])  # transient: freed when this function returns
            ctx.q = None
            if _wgrad_kernel_serves(x_hat, g):
                from .. import linear as _linear

                grad_w, grad_b = _linear.linear_wgrad(x_hat, g.contiguous(), want_bias=need_b)
            else:
                grad_w = g.t().mm(x_hat.to(g.dtype))
            grad_w = grad_w.to(weight.dtype)
        if need_b and grad_b is None:
            grad_b = g.sum(0)
        return grad_x, grad_w, grad_b, None, None


def linear_q(x, weight, bias=None, bits=None, group=None):
    """F.linear(x, weight, bias) whose backward reads x from its quantised copy (bits / group: actnn_compat's config when
    None).  grad_input = g W is exact; grad_weight = g^T x_hat carries the quantisation noise (zero mean)."""
    if bits is None or group is None:
        from .. import actnn_compat

        bits = actnn_compat.config.bits if bits is None else bits
        group = actnn_compat.config.group_size if group is None else group
    return _LinearQ.apply(x, weight, bias, int(bits), int(group))
