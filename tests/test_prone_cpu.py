"""The polynomial filter step's host twin, the Bessel series, the four filters and the ProNE stages on the CPU: the twin
against a literal float32 loop bit for bit, the argument checks, and the recorded results of the reference's own functions
(tests/golden/prone, tests/golden/make_golden_prone.py) within the bound of tests/_prone_cases.py."""
import numpy as np
import pytest
import torch

import _prone_cases as cases
from cogdl_amd import _lib, embedding
from cogdl_amd.operators import spectral
from cogdl_amd.operators.spectral import bessel_i, filter_step, spectral_filter


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy())


def run_step(rowptr, colind, ops, subset, alias=None):
    """filter_step on CPU tensors for an operand subset -> (out, acc) as numpy; alias = "z1" / "z2": out is that tensor."""
    t = dict((k, T(ops[k])) for k in ("x", "z1", "z2", "acc", "val", "dst_scale"))
    kw = dict(a=ops["a"], b=ops["b"] if subset["b"] else 0.0)
    if subset["z1"]:
        kw.update(z1=t["z1"], c1=ops["c1"])
    if subset["z2"]:
        kw.update(z2=t["z2"], c2=ops["c2"])
    if subset["dst_scale"]:
        kw.update(dst_scale=t["dst_scale"])
    if subset["acc"]:
        kw.update(acc=t["acc"], d=ops["d"])
    if alias:
        kw["out"] = t[alias]
    out = filter_step(T(rowptr), T(colind), t["val"] if subset["val"] else None, t["x"], **kw)
    if alias:
        assert out is t[alias]
    return out.numpy(), (t["acc"].numpy() if subset["acc"] else None)


def literal(rowptr, colind, ops, subset, dtype=np.float32):
    pick = lambda k: ops[k] if subset[k] else None
    return cases.step_literal(rowptr, colind, pick("val"), ops["x"], ops["a"], ops["b"] if subset["b"] else 0.0, pick("z1"),
                              ops["c1"], pick("z2"), ops["c2"], pick("dst_scale"), pick("acc"), ops["d"], dtype=dtype)


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("f", [3, 33])
def test_twin_equals_the_literal_loop_for_every_operand_subset(f):
    rowptr, colind = cases.ragged()  # degrees 0, 1, 63 .. 129: the zero-edge row gets its epilogue too
    ops = cases.step_operands(rowptr, colind, f)
    for subset in cases.SUBSETS:
        out, acc = run_step(rowptr, colind, ops, subset)
        want_out, want_acc = literal(rowptr, colind, ops, subset)
        assert same_bits(out, want_out), subset
        if subset["acc"]:
            assert same_bits(acc, want_acc), subset
    assert np.diff(rowptr)[0] == 0


@pytest.mark.parametrize("f", cases.WIDTHS)
def test_twin_all_operands_every_width_and_out_aliases(f):
    rowptr, colind = cases.ragged()
    ops = cases.step_operands(rowptr, colind, f, seed=1)
    full = dict((k, True) for k in ("b", "z1", "z2", "dst_scale", "acc", "val"))
    want_out, want_acc = literal(rowptr, colind, ops, full)
    for alias in (None, "z1", "z2"):
        out, acc = run_step(rowptr, colind, ops, full, alias=alias)
        assert same_bits(out, want_out) and same_bits(acc, want_acc), alias


def test_twin_skips_absent_terms_instead_of_multiplying_by_zero():
    rowptr, colind = cases.ragged()
    ops = cases.step_operands(rowptr, colind, 8)
    ops["x"][5, :] = np.inf  # b == 0: x[i, :] is not read for row i's own term (0 * inf would be nan)
    none = dict((k, False) for k in ("b", "z1", "z2", "dst_scale", "acc", "val"))
    out, _ = run_step(rowptr, colind, ops, none)
    assert not np.isin(5, colind[rowptr[5]:rowptr[6]]) and np.isfinite(out[5]).all()
    want, _ = literal(rowptr, colind, ops, none)
    assert np.array_equal(out, want, equal_nan=True)


def test_twin_sums_rows_of_any_length_in_csr_order():
    rowptr, colind = cases.hub()
    ops = cases.step_operands(rowptr, colind, 8)
    full = dict((k, True) for k in ("b", "z1", "z2", "dst_scale", "acc", "val"))
    out, acc = run_step(rowptr, colind, ops, full)
    want_out, want_acc = literal(rowptr, colind, ops, full)
    assert same_bits(out, want_out) and same_bits(acc, want_acc)  # the host sum is sequential at any length


def _operands(n=6, f=4):
    rowptr = torch.tensor([0, 1, 2, 3, 4, 5, 6], dtype=torch.int32)
    colind = torch.tensor([1, 2, 3, 4, 5, 0], dtype=torch.int32)
    return rowptr, colind, torch.randn(n, f)


def test_aliasing_violations_raise():
    rowptr, colind, x = _operands()
    other = torch.randn_like(x)
    with pytest.raises(_lib.BackendError):
        filter_step(rowptr, colind, None, x, a=1.0, out=x)
    with pytest.raises(_lib.BackendError):
        filter_step(rowptr, colind, None, x, a=1.0, acc=x, d=1.0)
    with pytest.raises(_lib.BackendError):
        filter_step(rowptr, colind, None, x, a=1.0, acc=other, d=1.0, out=other)
    big = torch.randn(x.numel() + 4)
    shifted, base = big[4:].view_as(x), big[:x.numel()].view_as(x)
    with pytest.raises(_lib.BackendError):  # a z that overlaps out without being it
        filter_step(rowptr, colind, None, x, a=1.0, z1=shifted, c1=1.0, out=base)
    before = x.clone()
    filter_step(rowptr, colind, None, x, a=1.0, z1=other, c1=1.0, out=other)  # out is z1: allowed
    assert torch.equal(x, before)


def test_the_abi_itself_refuses_aliasing_and_bad_sizes():
    rowptr, colind, x = _operands()
    out = torch.empty_like(x)
    lib = _lib.host()
    call = lambda o, acc=None, n=6, k=4, dtype=0: lib.cogdl_host_csr_filter_step(
        _lib.ptr(rowptr), _lib.ptr(colind), None, _lib.ptr(x), _lib.ptr(o), n, k, 6, dtype, 1.0, 0.0, None, 0.0, None, 0.0, None,
        _lib.ptr(acc), 0.0)
    assert call(out) == 0
    assert call(x) == 1 and call(out, acc=x) == 1 and call(out, acc=out) == 1
    assert call(out, n=-1) == 1 and call(out, dtype=1) == 1
    assert call(out, n=0) == 0 and call(out, k=0) == 0
    bad = colind.clone()
    bad[2] = 6
    rc = lib.cogdl_host_csr_filter_step(_lib.ptr(rowptr), _lib.ptr(bad), None, _lib.ptr(x), _lib.ptr(out), 6, 4, 6, 0, 1.0, 0.0,
                                        None, 0.0, None, 0.0, None, None, 0.0)
    assert rc == 2  # COGDL_HOST_ERANGE: nothing read out of bounds


@pytest.mark.parametrize("case", ["x dtype", "x 1-D", "rowptr int64", "rowptr length", "z1 shape", "acc dtype", "scale shape",
                                  "val shape", "strided z2", "out shape", "requires grad", "strided x"])
def test_shape_dtype_and_grad_errors_raise(case):
    rowptr, colind, x = _operands()
    kw = dict(a=1.0)
    if case == "x dtype":
        x = x.double()
    elif case == "x 1-D":
        x = x[:, 0].contiguous()
    elif case == "rowptr int64":
        rowptr = rowptr.long()
    elif case == "rowptr length":
        rowptr = rowptr[:-1].contiguous()
    elif case == "z1 shape":
        kw.update(z1=torch.randn(6, 5), c1=1.0)
    elif case == "acc dtype":
        kw.update(acc=torch.zeros(6, 4, dtype=torch.float64), d=1.0)
    elif case == "scale shape":
        kw.update(dst_scale=torch.ones(5))
    elif case == "val shape":
        kw.update(val=torch.ones(5))
    elif case == "strided z2":
        kw.update(z2=torch.randn(4, 6).t(), c2=1.0)
    elif case == "out shape":
        kw.update(out=torch.empty(6, 3))
    elif case == "requires grad":
        x = x.requires_grad_()
    elif case == "strided x":
        x = torch.randn(4, 6).t()
    val = kw.pop("val", None)
    with pytest.raises(_lib.BackendError):
        filter_step(rowptr, colind, val, x, **kw)


def test_bessel_series_matches_scipy():
    iv = pytest.importorskip("scipy.special").iv
    for n in range(21):
        for s in (0.1, 0.5, 1.0, 5.0):
            want = float(iv(n, s))
            assert abs(bessel_i(n, s) - want) <= 1e-14 * want, (n, s)
    with pytest.raises(ValueError):
        bessel_i(-1, 0.5)


@pytest.mark.parametrize("graph", sorted(cases.GRAPHS))
@pytest.mark.parametrize("kind", cases.KINDS)
def test_filters_match_the_reference_within_the_float32_bound(graph, kind):
    pytest.importorskip("sklearn")
    rowptr, colind = cases.GRAPHS[graph]()
    gold = cases.load("filters_" + graph)
    emb = torch.from_numpy(gold["a"]).float()
    out = spectral_filter(kind, T(rowptr), T(colind), emb).numpy().astype(np.float64)
    err_new = float(np.abs(out - gold[kind]).max())
    err_ref = float(np.abs(cases.restate_f32(kind, rowptr, colind, gold["a"], bessel_i).astype(np.float64) - gold[kind]).max())
    print("%s %s: err_new %.3e err_ref %.3e max|golden| %.3f" % (graph, kind, err_new, err_ref, np.abs(gold[kind]).max()))
    assert err_new <= cases.bound(err_ref, gold[kind])
    assert torch.equal(emb, torch.from_numpy(gold["a"]).float())  # the input is not written


def test_filter_parameters_and_refusals():
    rowptr, colind = cases.ragged()
    emb = torch.randn(300, 4)
    rp, ci = T(rowptr), T(colind)
    assert torch.equal(spectral_filter("prone", rp, ci, emb, order=1), emb)
    a = spectral_filter("heat", rp, ci, emb, t=0.7, k=4)
    assert a.shape == emb.shape and not torch.equal(a, spectral_filter("heat", rp, ci, emb))
    with pytest.raises(ValueError):
        spectral_filter("sc", rp, ci, emb)
    with pytest.raises(ValueError):
        spectral_filter("ppr", rp, ci, emb, mu=0.1)
    with pytest.raises(_lib.BackendError):
        spectral_filter("ppr", rp, ci, emb.requires_grad_())
    srp, sci, scale = spectral.with_self_loops(rp, ci)
    deg = np.diff(rowptr)
    assert np.array_equal(np.diff(srp.numpy()), deg + 1) and np.array_equal(scale.numpy(), (1.0 / (deg + 1)).astype(np.float32))
    for i in (0, 1, 7):
        assert sorted(sci[srp[i]:srp[i + 1]].tolist()) == sorted(colind[rowptr[i]:rowptr[i + 1]].tolist() + [i])


def test_prefactorisation_matches_the_reference():
    rowptr, colind = cases.ragged()
    gold = cases.load("prefact_ragged")["data"]
    rp, ci, val = embedding.prone_prefactorization(T(rowptr).long(), T(colind).long())
    assert np.array_equal(rp.numpy(), rowptr) and np.array_equal(ci.numpy(), colind)  # degree-0 rows and columns stay empty
    err = float(np.abs(val.numpy().astype(np.float64) - gold).max())
    print("pre-factorisation: err %.3e, bound %.3e" % (err, 8 * cases.EPS * np.abs(gold).max()))
    assert err <= 8 * cases.EPS * np.abs(gold).max()
    assert np.diff(rowptr)[0] == 0 and not np.isin(0, colind)


def test_dense_embedding_matches_the_reference_up_to_column_signs():
    gold = cases.load("dense")
    u, s, _ = np.linalg.svd(gold["x"].astype(np.float32), full_matrices=False)
    e32 = u * np.sqrt(s)
    e32 = (e32 / np.linalg.norm(e32, axis=1, keepdims=True)).astype(np.float64)
    want = cases.cosine(gold["emb"])
    deviation = float(np.abs(cases.cosine(e32) - want).max())
    emb = embedding.dense_embedding(torch.from_numpy(gold["x"]).float())
    err = float(np.abs(cases.cosine(emb.numpy().astype(np.float64)) - want).max())
    print("dense embedding: err %.3e, float32 SVD deviation %.3e" % (err, deviation))
    assert emb.dtype == torch.float32 and err <= 4 * deviation
    # a rank-deficient input: the dead direction is a zero column, nothing is nan
    x = torch.from_numpy(gold["x"]).float()
    x[:, 7] = x[:, 0]
    low = embedding.dense_embedding(x)
    assert torch.isfinite(low).all() and int((low.abs().sum(0) == 0).sum()) == 1


def test_prone_embedding_is_finite_unit_norm_and_repeatable():
    rowptr, colind = cases.ragged()
    csr = (T(rowptr).long(), T(colind).long())
    a = embedding.prone(csr, dim=8, step=5, seed=3)
    b = embedding.prone(csr, dim=8, step=5, seed=3)
    assert a.shape == (300, 8) and a.dtype == torch.float32 and torch.isfinite(a).all() and torch.equal(a, b)
    norm = a.norm(dim=1)
    connected = torch.from_numpy(np.diff(rowptr) > 0)
    assert torch.allclose(norm[connected], torch.ones(int(connected.sum())), atol=1e-5)
    assert embedding.prone(csr, dim=8, step=1, seed=3).shape == (300, 8)
    with pytest.raises(ValueError):
        embedding.prone(csr, dim=0)
