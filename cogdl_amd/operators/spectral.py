"""Polynomial graph filters on the graph's device: the spectral propagation of ProNE and the heat-kernel / PPR / Gaussian
filters around it (cogdl/utils/prone_utils.py:26-176), which the reference runs as scipy float64 products on the host.

    filter_step(rowptr, colind, val, x, *, a, b, z1, c1, z2, c2, dst_scale, acc, d, out) -> out
    bessel_i(n, s)                                                                       -> I_n(s), Python float
    spectral_filter(kind, rowptr, colind, emb, **params)                                 -> float32 [N, F]

filter_step is ONE launch (cogdl_hip_csr_filter_step, csrc/polyfilter.hip; the OpenMP twin in libcogdl_host.so for CPU
tensors, and libcogdl_hip.so is then not loaded):

    t = A x  (csr_spmm's sum);  y = a * (dst_scale * t) + b * x + c1 * z1 + c2 * z2;  out = y;  acc += d * y

with every product and sum a separately rounded float32 operation in that order, absent operands skipped.  The four
filters are loops of it over three rotating [N, F] buffers plus the running sum `conv` as acc (DESIGN.md has the table of
coefficients).  The reference assembles its operator M = (1 - mu) I - D^-1 (A + I) as one float64 sparse matrix; here the
diagonal term is the step's b * x and the normalisation its dst_scale, in float32: the same numbers up to float32 rounding.
The "sc" filter (SignalRescaling) is not served.
"""
import torch

from .. import _lib

__all__ = ["filter_step", "bessel_i", "spectral_filter", "KINDS"]

KINDS = ("prone", "gaussian", "heat", "ppr")


def _dense(name, t, shape, dev):
    if not torch.is_tensor(t):
        raise _lib.BackendError("filter_step: %s must be a tensor" % name)
    if t.requires_grad:
        raise _lib.BackendError("filter_step: %s requires grad; the filter step has no backward" % name)
    if t.dtype != torch.float32:
        raise _lib.BackendError("filter_step: %s must be float32 (got %s)" % (name, t.dtype))
    if t.device != dev:
        raise _lib.BackendError("filter_step: %s is on %s, x on %s" % (name, t.device, dev))
    if tuple(t.shape) != tuple(shape):
        raise _lib.BackendError("filter_step: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    if not t.is_contiguous():
        raise _lib.BackendError("filter_step: %s must be contiguous" % name)
    return t


def _same(p, q):
    return p is not None and q is not None and p.data_ptr() == q.data_ptr()


def _overlap(p, q):
    if p is None or q is None or p.numel() == 0:
        return False
    a, b, nbytes = p.data_ptr(), q.data_ptr(), p.numel() * 4
    return a < b + nbytes and b < a + nbytes


def filter_step(rowptr, colind, val, x, *, a, b=0.0, z1=None, c1=0.0, z2=None, c2=0.0, dst_scale=None, acc=None, d=0.0,
                out=None):
    """One filter step (module docstring) on a square CSR structure: rowptr int32 [N + 1], colind int32 [nnz], val float32
    [nnz] or None (unweighted), x / z1 / z2 / acc / out float32 [N, F] contiguous, dst_scale float32 [N], scalars Python
    floats.  `out` may be z1 or z2 (None: a new tensor); out must not be x or acc, acc must not be x.  acc is updated in
    place.  No autograd: a tensor that requires grad raises BackendError.  -> out."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise _lib.BackendError("filter_step: x must be a 2-D tensor")
    dev, (n, k) = x.device, x.shape
    for name, t in (("rowptr", rowptr), ("colind", colind)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.device != dev or not t.is_contiguous():
            raise _lib.BackendError("filter_step: %s must be a contiguous 1-D int32 tensor on x's device" % name)
    if rowptr.numel() != n + 1:
        raise _lib.BackendError("filter_step: a square structure: rowptr has %d entries for %d rows of x" % (rowptr.numel(), n))
    nnz = colind.numel()
    x = _dense("x", x, (n, k), dev)
    if val is not None:
        val = _dense("val", val, (nnz,), dev)
    if dst_scale is not None:
        dst_scale = _dense("dst_scale", dst_scale, (n,), dev)
    z1 = None if z1 is None else _dense("z1", z1, (n, k), dev)
    z2 = None if z2 is None else _dense("z2", z2, (n, k), dev)
    acc = None if acc is None else _dense("acc", acc, (n, k), dev)
    out = torch.empty_like(x) if out is None else _dense("out", out, (n, k), dev)
    if _overlap(out, x) or _overlap(acc, x) or _overlap(out, acc):
        raise _lib.BackendError("filter_step: out must not be x or acc, and acc must not be x")
    for name, z in (("z1", z1), ("z2", z2)):
        for wname, w in (("out", out), ("acc", acc)):
            if _overlap(w, z) and not _same(w, z):
                raise _lib.BackendError("filter_step: %s overlaps %s without being it" % (name, wname))
    args = (_lib.ptr(rowptr), _lib.ptr(colind), _lib.ptr(val), _lib.ptr(x), _lib.ptr(out), n, k, nnz, 0, float(a), float(b),
            _lib.ptr(z1), float(c1), _lib.ptr(z2), float(c2), _lib.ptr(dst_scale), _lib.ptr(acc), float(d))
    if dev.type == "cuda":
        ws, ws_bytes = _lib.workspace("cogdl_hip_csr_spmm_workspace_bytes", dev, nnz, k, 0)
        args = args + (_lib.ptr(ws), ws_bytes)
    _lib.twin_call("csr_filter_step", dev, *args)
    return out


def bessel_i(n, s):
    """The modified Bessel function of the first kind I_n(s) for an integer order n >= 0, by its power series
    sum_m (s / 2)^(2 m + n) / (m! (m + n)!) in Python float64 (every term has one sign: no cancellation) -- what
    scipy.special.iv(n, s) returns to ~1e-15 relative for the arguments a filter uses (|s| up to tens)."""
    n, s = int(n), float(s)
    if n < 0:
        raise ValueError("bessel_i: the order must be >= 0 (got %d)" % n)
    h = s / 2.0
    term = 1.0
    for j in range(1, n + 1):
        term = term * h / j  # (s / 2)^n / n!
    total, m = term, 0
    while True:
        m += 1
        term = term * (h * h) / (m * (m + n))
        total += term
        if abs(term) <= 1e-17 * abs(total) or m > 500:
            return total


def _rows_of(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), (rowptr[1:] - rowptr[:-1]).long())


def with_self_loops(rowptr, colind):
    """The structure of A + I for a simple adjacency without self loops, by the library's graph-build helpers
    (add_remaining_self_loops, coo2csr_index) -> (rowptr int32 [N + 1], colind int32, 1 / (deg + 1) float32 [N])."""
    from ..graph_build import add_remaining_self_loops, coo2csr_index

    n = rowptr.numel() - 1
    (row, col), _ = add_remaining_self_loops((_rows_of(rowptr), colind.long()), None, 1, n)
    ptr64, perm = coo2csr_index(row, col, n)
    deg1 = (ptr64[1:] - ptr64[:-1]).float()
    return ptr64.int().contiguous(), col[perm].int().contiguous(), (1.0 / deg1).contiguous()


def _structure(name, rowptr, colind, emb):
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.dtype != torch.float32:
        raise _lib.BackendError("%s: emb must be a 2-D float32 tensor" % name)
    if emb.requires_grad:
        raise _lib.BackendError("%s: emb requires grad; the filters have no backward" % name)
    rowptr, colind = _lib.csr_structure(rowptr, colind)
    if rowptr.device != emb.device or colind.device != emb.device:
        raise _lib.BackendError("%s: the structure and emb are on different devices" % name)
    if rowptr.numel() != emb.shape[0] + 1:
        raise _lib.BackendError("%s: rowptr has %d entries for %d rows of emb" % (name, rowptr.numel(), emb.shape[0]))
    return rowptr, colind, emb.contiguous()


def _product(rowptr, colind, x):
    """A x with the unnormalised, unweighted structure: csrspmm on the GPU, the host SpMM on the CPU."""
    if x.device.type == "cuda":
        from .spmm import csrspmm

        return csrspmm(rowptr, colind, x, None)
    out = torch.empty_like(x)
    rc = _lib.host().cogdl_host_csr_spmm_f32(_lib.ptr(rowptr), _lib.ptr(colind), None, _lib.ptr(x), _lib.ptr(out),
                                             rowptr.numel() - 1, x.shape[1], torch.get_num_threads())
    _lib.check_host(rc, "csr_spmm_cpu")
    return out


def _chebyshev_gaussian(rp, ci, scale, emb, order, mu, s):
    """conv of ProNE.__call__ / Gaussian.prop (prone_utils.py:59-91, 142-176) with M = (1 - mu) I - D^-1 (A + I):
    Lx1 = 0.5 M M emb - emb, Lx_{i+1} = M M Lx_i - 2 Lx_i - Lx_{i-1}, conv = I_0 emb + sum_i (-1)^i 2 I_i(s) Lx_i."""
    m = dict(dst_scale=scale, b=1.0 - mu)
    conv = emb * bessel_i(0, s)
    u = filter_step(rp, ci, None, emb, a=-1.0, **m)
    # 0.5 * (M u) - emb
    lx1 = filter_step(rp, ci, None, u, a=-0.5, dst_scale=scale, b=0.5 * (1.0 - mu), z1=emb, c1=-1.0, acc=conv, d=-2.0 * bessel_i(1, s))
    lx0 = emb
    for i in range(2, order):
        filter_step(rp, ci, None, lx1, a=-1.0, out=u, **m)
        # (M u - 2 Lx1) - Lx0, written over Lx0 (out is z2) once Lx0 is a buffer of ours: u and two more rotate
        sign = 1.0 if i % 2 == 0 else -1.0
        lx2 = filter_step(rp, ci, None, u, a=-1.0, z1=lx1, c1=-2.0, z2=lx0, c2=-1.0, acc=conv, d=sign * 2.0 * bessel_i(i, s),
                          out=None if lx0 is emb else lx0, **m)
        lx0, lx1 = lx1, lx2
    return conv


def spectral_filter(kind, rowptr, colind, emb, **params):
    """A filter of cogdl/utils/prone_utils.py applied to emb [N, F] float32 on the simple adjacency (rowptr, colind: int32
    CSR without self loops, unit weights) -> float32 [N, F] on emb's device.  Defaults are the reference's:
        "prone"     order=10, mu=0.1, s=0.5    ProNE.__call__ (142-176): A' (emb - conv) with A' = A + I, order 1 returns emb
        "gaussian"  mu=0.5, theta=1.0, k=3     Gaussian.prop (59-91), rescale=False
        "heat"      t=0.2, k=5                 HeatKernelApproximation.chebyshev (39-53)
        "ppr"       alpha=0.5, k=10            PPR.prop (94-113), on A without self loops
    Every [N, F] pass but the first scaling of conv and ProNE's final subtraction is a filter_step."""
    if kind not in KINDS:
        raise ValueError("spectral_filter: kind must be one of %s (got %r)" % (KINDS, kind))
    defaults = {"prone": dict(order=10, mu=0.1, s=0.5), "gaussian": dict(mu=0.5, theta=1.0, k=3),
                "heat": dict(t=0.2, k=5), "ppr": dict(alpha=0.5, k=10)}[kind]
    unknown = set(params) - set(defaults)
    if unknown:
        raise ValueError("spectral_filter(%r): unknown parameters %s" % (kind, sorted(unknown)))
    p = dict(defaults, **params)
    rowptr, colind, emb = _structure("spectral_filter", rowptr, colind, emb)
    with torch.no_grad():
        if kind == "ppr":
            alpha, k = float(p["alpha"]), int(p["k"])
            deg = (rowptr[1:] - rowptr[:-1]).float()
            scale = torch.where(deg > 0, 1.0 / deg.clamp_min(1.0), torch.zeros_like(deg)).contiguous()
            conv = emb * alpha
            lx, other = emb, None
            for _ in range(1, k):
                nxt = filter_step(rowptr, colind, None, lx, a=1.0 - alpha, dst_scale=scale, acc=conv, d=1.0, out=other)
                other = lx if lx is not emb else None
                lx = nxt
            return conv
        if kind == "prone" and int(p["order"]) == 1:
            return emb.clone()
        rp, ci, scale = with_self_loops(rowptr, colind)
        if kind == "heat":
            t, k = float(p["t"]), int(p["k"])
            conv = emb * bessel_i(0, t)
            lx1 = filter_step(rp, ci, None, emb, a=-1.0, dst_scale=scale, b=1.0, acc=conv, d=-2.0 * bessel_i(1, t))
            lx0 = emb
            for i in range(2, k):
                # 2 L Lx1 - Lx0, written over Lx0 (out is z1) once Lx0 is a buffer of ours
                dst = None if lx0 is emb else lx0
                lx2 = filter_step(rp, ci, None, lx1, a=-2.0, dst_scale=scale, b=2.0, z1=lx0, c1=-1.0, acc=conv,
                                  d=(1.0 if i % 2 == 0 else -1.0) * 2.0 * bessel_i(i, t), out=dst)
                lx0, lx1 = lx1, lx2
            return conv
        if kind == "gaussian":
            return _chebyshev_gaussian(rp, ci, scale, emb, int(p["k"]), float(p["mu"]), float(p["theta"]))
        conv = _chebyshev_gaussian(rp, ci, scale, emb, int(p["order"]), float(p["mu"]), float(p["s"]))
        return _product(rp, ci, emb - conv)
