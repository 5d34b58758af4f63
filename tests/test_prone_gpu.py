"""The fused filter step on the GPU (cogdl_hip_csr_filter_step): bit for bit the composition of csrspmm and torch's
separately rounded elementwise kernels on both graphs, every width and every operand subset, long rows included; bit for
bit the host twin wherever a row has at most the long-row threshold of edges, and within the float32 bound of a float64
oracle above it; the four filters against the reference's recorded results; repeatable, stream-correct; and the stages
of embedding.prone against the same stages on the CPU."""
import functools

import numpy as np
import pytest
import torch

import _prone_cases as cases
from cogdl_amd import _lib, embedding
from cogdl_amd.operators.spectral import bessel_i, filter_step, spectral_filter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL = dict((k, True) for k in ("b", "z1", "z2", "dst_scale", "acc", "val"))


def T(a, dev=DEV):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


@functools.lru_cache(None)
def structure(graph):
    rowptr, colind = cases.GRAPHS[graph]()
    return T(rowptr), T(colind)


def tensors(ops, dev=DEV):
    return dict((k, T(ops[k], dev)) for k in ("x", "z1", "z2", "acc", "val", "dst_scale"))


def step_kwargs(ops, t, subset):
    kw = dict(a=ops["a"], b=ops["b"] if subset["b"] else 0.0)
    if subset["z1"]:
        kw.update(z1=t["z1"], c1=ops["c1"])
    if subset["z2"]:
        kw.update(z2=t["z2"], c2=ops["c2"])
    if subset["dst_scale"]:
        kw.update(dst_scale=t["dst_scale"])
    if subset["acc"]:
        kw.update(acc=t["acc"], d=ops["d"])
    return kw


def composition(rp, ci, ops, t, subset):
    """csrspmm, then torch's elementwise kernels in the stated order: every product and sum its own rounded kernel."""
    from cogdl_amd.operators.spmm import csrspmm

    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)
    s = csrspmm(rp, ci, t["x"], t["val"] if subset["val"] else None)
    if subset["dst_scale"]:
        s = t["dst_scale"].unsqueeze(1) * s
    y = f32(ops["a"]) * s
    if subset["b"]:
        y = y + f32(ops["b"]) * t["x"]
    if subset["z1"]:
        y = y + f32(ops["c1"]) * t["z1"]
    if subset["z2"]:
        y = y + f32(ops["c2"]) * t["z2"]
    acc = t["acc"] + f32(ops["d"]) * y if subset["acc"] else None
    return y, acc


@pytest.mark.parametrize("f", cases.WIDTHS)
@pytest.mark.parametrize("graph", sorted(cases.GRAPHS))
def test_fused_step_equals_csrspmm_plus_elementwise_bit_for_bit(graph, f):
    rowptr, colind = cases.GRAPHS[graph]()
    rp, ci = structure(graph)
    ops = cases.step_operands(rowptr, colind, f)
    t = tensors(ops)
    for subset in cases.SUBSETS:
        want_out, want_acc = composition(rp, ci, ops, t, subset)
        acc0 = t["acc"].clone()
        kw = step_kwargs(ops, dict(t, acc=acc0), subset)
        out = filter_step(rp, ci, t["val"] if subset["val"] else None, t["x"], **kw)
        assert torch.equal(out, want_out), (subset, float((out - want_out).abs().max()))
        if subset["acc"]:
            assert torch.equal(acc0, want_acc), subset


@pytest.mark.parametrize("f", [8, 128, 200])
def test_out_may_be_z1_or_z2(f):
    rowptr, colind = cases.hub()
    rp, ci = structure("hub")
    ops = cases.step_operands(rowptr, colind, f, seed=2)
    t = tensors(ops)
    want = filter_step(rp, ci, t["val"], t["x"], **step_kwargs(ops, dict(t, acc=t["acc"].clone()), FULL))
    for alias in ("z1", "z2"):
        mine = dict(t, acc=t["acc"].clone())
        mine[alias] = t[alias].clone()
        out = filter_step(rp, ci, t["val"], t["x"], out=mine[alias], **step_kwargs(ops, mine, FULL))
        assert out is mine[alias] and torch.equal(out, want)


def test_aliasing_and_dtype_refusals_of_the_abi():
    rp, ci = structure("ragged")
    x = torch.randn(300, 8, device=DEV)
    other = torch.randn_like(x)
    for kw in (dict(out=x), dict(acc=x, d=1.0), dict(acc=other, d=1.0, out=other)):
        with pytest.raises(_lib.BackendError):
            filter_step(rp, ci, None, x, a=1.0, **kw)
    for kw in (dict(z1=other.cpu(), c1=1.0), dict(dst_scale=torch.ones(300)), dict(acc=other.cpu(), d=1.0)):
        with pytest.raises(_lib.BackendError):  # an operand on another device
            filter_step(rp, ci, None, x, a=1.0, **kw)
    lib = _lib.hip()
    call = lambda o, acc=None, dtype=0, n=300, k=8: lib.cogdl_hip_csr_filter_step(
        _lib.ptr(rp), _lib.ptr(ci), None, _lib.ptr(x), _lib.ptr(o), n, k, ci.numel(), dtype, 1.0, 0.0, None, 0.0, None, 0.0, None,
        _lib.ptr(acc), 0.0, None, 0, _lib.stream_of(x))
    assert call(x) == 1 and call(other, acc=x) == 1 and call(other, acc=other) == 1  # COGDL_HIP_EINVAL
    assert call(other, dtype=1) == 7                                                  # COGDL_HIP_EUNSUPPORTED
    assert call(other, n=0) == 0 and call(other, k=0) == 0 and call(other, n=-1) == 1
    assert call(other) == 0                                                           # no workspace: sequential rows
    torch.cuda.synchronize()


@pytest.mark.parametrize("f", cases.WIDTHS)
def test_gpu_equals_host_twin_on_ragged(f):
    rowptr, colind = cases.ragged()
    assert np.diff(rowptr).max() == cases.LONG + 1 and _lib.hip().cogdl_hip_long_row_threshold(colind.size) == cases.LONG
    ops = cases.step_operands(rowptr, colind, f, seed=3)
    gpu, cpu = tensors(ops), tensors(ops, "cpu")
    out = filter_step(*structure("ragged"), gpu["val"], gpu["x"], **step_kwargs(ops, gpu, FULL))
    ref = filter_step(T(rowptr, "cpu"), T(colind, "cpu"), cpu["val"], cpu["x"], **step_kwargs(ops, cpu, FULL))
    short = torch.from_numpy(np.diff(rowptr) <= cases.LONG)
    assert torch.equal(out.cpu()[short], ref[short]) and torch.equal(gpu["acc"].cpu()[short], cpu["acc"][short])
    check_long_rows(rowptr, colind, ops, out.cpu().numpy(), gpu["acc"].cpu().numpy())


def check_long_rows(rowptr, colind, ops, out, acc):
    """Rows above the threshold: re-associated sums.  Against the float64 oracle they may lose what the sequential float32
    loop loses four times over, plus eight roundings of the row's largest value."""
    long_rows = np.nonzero(np.diff(rowptr) > cases.LONG)[0]
    assert long_rows.size
    # (only the long rows are evaluated: a CSR of those rows alone, the dense operands sliced alike)
    sub_ptr = np.concatenate([[0], np.cumsum(np.diff(rowptr)[long_rows])]).astype(np.int64)
    sub_col = np.concatenate([colind[rowptr[i]:rowptr[i + 1]] for i in long_rows])
    sub_val = np.concatenate([ops["val"][rowptr[i]:rowptr[i + 1]] for i in long_rows])

    def rows_only(dtype):
        n, f = ops["x"].shape
        outs, accs = [], []
        for j, i in enumerate(long_rows):
            xs = ops["x"].astype(dtype)
            t = np.zeros(f, dtype=dtype)
            for e in range(sub_ptr[j], sub_ptr[j + 1]):
                t = t + dtype(sub_val[e]) * xs[sub_col[e]]
            c = lambda v: dtype(np.float32(v))
            y = c(ops["a"]) * (dtype(ops["dst_scale"][i]) * t)
            y = y + c(ops["b"]) * xs[i]
            y = y + c(ops["c1"]) * ops["z1"][i].astype(dtype)
            y = y + c(ops["c2"]) * ops["z2"][i].astype(dtype)
            outs.append(y)
            accs.append(ops["acc"][i].astype(dtype) + c(ops["d"]) * y)
        return np.stack(outs), np.stack(accs)

    o64, a64 = rows_only(np.float64)
    o32, a32 = rows_only(np.float32)
    for name, got, w64, w32 in (("out", out[long_rows], o64, o32), ("acc", acc[long_rows], a64, a32)):
        err_new = float(np.abs(got.astype(np.float64) - w64).max())
        err_ref = float(np.abs(w32.astype(np.float64) - w64).max())
        print("long rows %s: err_new %.3e err_ref %.3e" % (name, err_new, err_ref))
        assert err_new <= cases.bound(err_ref, w64)


@pytest.mark.parametrize("f", [3, 64, 128])
def test_gpu_equals_host_twin_on_hub_short_rows_and_bounds_the_long_ones(f):
    rowptr, colind = cases.hub()
    ops = cases.step_operands(rowptr, colind, f, seed=4)
    gpu, cpu = tensors(ops), tensors(ops, "cpu")
    out = filter_step(*structure("hub"), gpu["val"], gpu["x"], **step_kwargs(ops, gpu, FULL))
    ref = filter_step(T(rowptr, "cpu"), T(colind, "cpu"), cpu["val"], cpu["x"], **step_kwargs(ops, cpu, FULL))
    short = torch.from_numpy(np.diff(rowptr) <= cases.LONG)
    assert int((~short).sum()) >= 2 and np.diff(rowptr).max() > 10 * cases.LONG  # several chunks per long row
    assert torch.equal(out.cpu()[short], ref[short]) and torch.equal(gpu["acc"].cpu()[short], cpu["acc"][short])
    check_long_rows(rowptr, colind, ops, out.cpu().numpy(), gpu["acc"].cpu().numpy())


@pytest.mark.parametrize("graph", sorted(cases.GRAPHS))
@pytest.mark.parametrize("kind", cases.KINDS)
def test_filters_match_the_reference_within_the_float32_bound(graph, kind):
    pytest.importorskip("sklearn")
    rowptr, colind = cases.GRAPHS[graph]()
    gold = cases.load("filters_" + graph)
    rp, ci = structure(graph)
    emb = torch.from_numpy(gold["a"]).float().to(DEV)
    first = spectral_filter(kind, rp, ci, emb)
    out = first.cpu().numpy().astype(np.float64)
    err_new = float(np.abs(out - gold[kind]).max())
    err_ref = float(np.abs(cases.restate_f32(kind, rowptr, colind, gold["a"], bessel_i).astype(np.float64) - gold[kind]).max())
    print("%s %s: err_new %.3e err_ref %.3e max|golden| %.3f" % (graph, kind, err_new, err_ref, np.abs(gold[kind]).max()))
    assert err_new <= cases.bound(err_ref, gold[kind])
    assert torch.equal(spectral_filter(kind, rp, ci, emb), first)  # equal from run to run


def test_side_stream_gives_the_same_bytes():
    rowptr, colind = cases.hub()
    rp, ci = structure("hub")
    ops = cases.step_operands(rowptr, colind, 128, seed=5)
    t = tensors(ops)
    want_acc = t["acc"].clone()
    want = filter_step(rp, ci, t["val"], t["x"], **step_kwargs(ops, dict(t, acc=want_acc), FULL))
    emb = torch.randn(rowptr.size - 1, 33, device=DEV)
    want_filter = spectral_filter("prone", rp, ci, emb, order=4)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        acc = t["acc"].clone()
        out = filter_step(rp, ci, t["val"], t["x"], **step_kwargs(ops, dict(t, acc=acc), FULL))
        got_filter = spectral_filter("prone", rp, ci, emb, order=4)
    side.synchronize()
    assert torch.equal(out, want) and torch.equal(acc, want_acc) and torch.equal(got_filter, want_filter)


def test_prone_stages_agree_with_the_cpu():
    rowptr, colind = cases.hub()
    ip, ix = T(rowptr, "cpu").long(), T(colind, "cpu").long()
    # (a) the pre-factorisation matrix: float32 column sums in one order on both sides, float64 elementwise, one rounding
    rp_c, ci_c, val_c = embedding.prone_prefactorization(ip, ix)
    rp_g, ci_g, val_g = embedding.prone_prefactorization(ip.to(DEV), ix.to(DEV))
    assert torch.equal(rp_g.cpu(), rp_c) and torch.equal(ci_g.cpu(), ci_c)
    top = float(val_c.abs().max())
    assert float((val_g.cpu() - val_c).abs().max()) <= 8 * cases.EPS * top
    # (c) the propagation of one input: each side within the filters' bound of the float64 computation
    pytest.importorskip("sklearn")
    feat = torch.randn(rowptr.size - 1, 16, generator=torch.Generator().manual_seed(0))
    feat = feat / feat.norm(dim=1, keepdim=True)
    params = dict(order=5, mu=0.2, s=0.5)
    prop_c = spectral_filter("prone", rp_c, ci_c, feat, **params)
    prop_g = spectral_filter("prone", rp_g, ci_g, feat.to(DEV), **params)
    truth = cases.restate_f32("prone", rowptr, colind, feat.numpy().astype(np.float64), bessel_i, dtype=np.float64, **params)
    err_ref = float(np.abs(cases.restate_f32("prone", rowptr, colind, feat.numpy(), bessel_i, **params).astype(np.float64) - truth).max())
    for name, prop in (("cpu", prop_c), ("gpu", prop_g.cpu())):
        err_new = float(np.abs(prop.numpy().astype(np.float64) - truth).max())
        print("propagation on %s: err_new %.3e err_ref %.3e" % (name, err_new, err_ref))
        assert err_new <= cases.bound(err_ref, truth)
    # (d) the dense embedding of one input: cosines within four times the float32 SVD's deviation from float64
    x = prop_c
    u64, s64, _ = np.linalg.svd(x.numpy().astype(np.float64), full_matrices=False)
    e64 = u64 * np.sqrt(s64)
    e64 = e64 / np.maximum(np.linalg.norm(e64, axis=1, keepdims=True), 1e-300)
    u32, s32, _ = np.linalg.svd(x.numpy(), full_matrices=False)
    e32 = (u32 * np.sqrt(s32)).astype(np.float64)
    e32 = e32 / np.maximum(np.linalg.norm(e32, axis=1, keepdims=True), 1e-300)
    rows = slice(0, 400)
    deviation = float(np.abs(cases.cosine(e32[rows]) - cases.cosine(e64[rows])).max())
    for dev in ("cpu", DEV):
        e = embedding.dense_embedding(x.to(dev)).cpu().numpy().astype(np.float64)
        err = float(np.abs(cases.cosine(e[rows]) - cases.cosine(e64[rows])).max())
        print("dense embedding on %s: err %.3e, float32 SVD deviation %.3e" % (dev, err, deviation))
        assert err <= 4 * deviation
    # the whole pipeline runs on the GPU and repeats itself
    a = embedding.prone((ip.to(DEV), ix.to(DEV)), dim=16, step=5, seed=7)
    b = embedding.prone((ip.to(DEV), ix.to(DEV)), dim=16, step=5, seed=7)
    assert a.is_cuda and a.shape == (rowptr.size - 1, 16) and torch.isfinite(a).all() and torch.equal(a, b)
