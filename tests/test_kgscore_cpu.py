"""Sampled triple scoring on the CPU: the OpenMP host twin of sampled_scores against the law of csrc/kgscore_law.h restated in
numpy float32 (bit for bit: scores, grad_q, grad_table), against a float64 evaluation of the same formulas within the derived
bound of tests/_kgscore_cases.py::exact, and against torch autograd of the gather composition within that bound taken twice
(torch's float32 sums obey the same bound in their own order); equal results from run to run; only the gradients that are
asked for are computed; the refusals, the check flag and the status codes of the C entry points of both libraries (every
status is returned before anything is launched, so the HIP ones are asked here as well)."""
import ctypes

import numpy as np
import pytest
import torch

import _kgscore_cases as C
import _offset as O
from cogdl_amd import _lib
from cogdl_amd.operators import sampled_scores
from cogdl_amd.operators import kgscore as K


def tensors(name, grad=True):
    c = C.make(name)
    q, table = torch.from_numpy(c["q"].copy()), torch.from_numpy(c["table"].copy())
    if grad:
        q.requires_grad_()
        table.requires_grad_()
    return q, table, torch.from_numpy(c["idx"].copy()), torch.from_numpy(c["g"].copy())


def run(name, kind, idx_dtype=torch.int64):
    q, table, idx, g = tensors(name)
    s = sampled_scores(q, table, idx.to(idx_dtype), kind, C.GAMMA)
    gq, gt = torch.autograd.grad(s, (q, table), g)
    return s.detach().numpy(), gq.numpy(), gt.numpy()


def within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err - bound).max())
    print("%s: max |err| %.3e, max err / bound %.3f" % (what, err.max(), float((err / np.maximum(bound, 1e-300)).max())))
    assert worst <= 0.0, what


@pytest.mark.parametrize("name,kind", C.CASES)
def test_twin_equals_the_law_bit_for_bit(name, kind):
    s, gq, gt = run(name, kind, torch.int32 if name == "scalar_66" else torch.int64)
    ls, lq, lt = C.law(name, kind)
    assert C.bits_equal(s, ls), "scores"
    assert C.bits_equal(gq, lq), "grad_q"
    assert C.bits_equal(gt, lt), "grad_table"
    if C.SHAPES[name][2] == 40:  # an entity no id names gets a row of +0
        assert not gt[list(C.UNNAMED)].view(np.int32).any()


@pytest.mark.parametrize("name,kind", C.CASES)
def test_twin_within_the_derived_bound_of_float64(name, kind):
    s, gq, gt = run(name, kind)
    es, eq, et, bs, bq, bt = C.exact(name, kind)
    within(s, es, bs, "scores")
    within(gq, eq, bq, "grad_q")
    within(gt, et, bt, "grad_table")


@pytest.mark.parametrize("name,kind", C.CASES)
def test_twin_agrees_with_torch_autograd_of_the_gather_composition(name, kind):
    s, gq, gt = run(name, kind)
    q, table, idx, g = tensors(name)
    ref = K.gather_composition(q, table, idx, kind, C.GAMMA)
    rq, rt = torch.autograd.grad(ref, (q, table), g)
    _, _, _, bs, bq, bt = C.exact(name, kind)
    within(s, ref.detach().numpy().astype(np.float64), 2 * bs, "scores")
    within(gq, rq.numpy().astype(np.float64), 2 * bq, "grad_q")
    within(gt, rt.numpy().astype(np.float64), 2 * bt, "grad_table")


def test_zero_difference_has_zero_derivative():
    """Row 0 of q equals its first candidate's row: l1 and cl2 contribute exactly nothing there, as torch does."""
    for kind in ("l1", "cl2"):
        q, table, idx, _ = tensors("few_terms")
        g = torch.zeros(idx.shape)
        g[0, 0] = 1.0
        s = sampled_scores(q, table, idx, kind, C.GAMMA)
        gq, gt = torch.autograd.grad(s, (q, table), g)
        assert s[0, 0].item() == C.GAMMA and not gq.numpy().view(np.int32).any() and not gt.numpy().view(np.int32).any()
        rq, rt = torch.autograd.grad(K.gather_composition(q, table, idx, kind, C.GAMMA), (q, table), g)
        assert not rq.abs().max().item() and not rt.abs().max().item()


def test_equal_from_run_to_run_and_for_shifted_operands():
    for kind in C.KINDS:
        first = run("many_j_250", kind)
        again = run("many_j_250", kind)
        assert all(C.bits_equal(a, b) for a, b in zip(first, again))
        c = C.make("many_j_250")
        q, _ = O.shifted(torch.from_numpy(c["q"].copy()), 1)
        table, _ = O.shifted(torch.from_numpy(c["table"].copy()), 1)
        idx, _ = O.shifted(torch.from_numpy(c["idx"].astype(np.int32)), 1)
        g, _ = O.shifted(torch.from_numpy(c["g"].copy()), 1)
        assert q.data_ptr() % 16 == 4 and table.data_ptr() % 16 == 4
        q.requires_grad_()
        table.requires_grad_()
        s = sampled_scores(q, table, idx, kind, C.GAMMA)
        gq, gt = torch.autograd.grad(s, (q, table), g)
        assert all(C.bits_equal(a, b.detach().numpy()) for a, b in zip(first, (s, gq, gt)))


def test_only_the_gradients_asked_for_are_computed(monkeypatch):
    calls = []
    real = _lib.twin_call
    monkeypatch.setattr(_lib, "twin_call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    want = {(True, True): ["kg_score", "kg_score_grad_q", "kg_score_grad_table"], (True, False): ["kg_score", "kg_score_grad_q"],
            (False, True): ["kg_score", "kg_score_grad_table"]}
    for (need_q, need_t), names in want.items():
        del calls[:]
        q, table, idx, g = tensors("few_terms", grad=False)
        q.requires_grad_(need_q)
        table.requires_grad_(need_t)
        s = sampled_scores(q, table, idx, "cl2", C.GAMMA)
        s.backward(g)
        assert calls == names
        assert (q.grad is not None) == need_q and (table.grad is not None) == need_t
    del calls[:]
    q, table, idx, _ = tensors("few_terms", grad=False)
    assert not sampled_scores(q, table, idx, "dot").requires_grad and calls == ["kg_score"]
    q.requires_grad_()
    s = sampled_scores(q, table, idx, "dot")
    (gq,) = torch.autograd.grad(s.sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):  # once_differentiable
        gq.sum().backward()


def test_check_flag_and_out_of_range_ids():
    q, table, idx, g = tensors("scalar_66")
    n = table.shape[0]
    for bad in (-1, n):
        broken = idx.clone()
        broken[3, 1] = bad
        with pytest.raises(_lib.BackendError):
            sampled_scores(q, table, broken, "l1", C.GAMMA)
        # check=False: NaN at that position; a valid id there with a zero gradient gives the same gradients everywhere
        s = sampled_scores(q, table, broken, "l1", C.GAMMA, check=False)
        assert torch.isnan(s[3, 1]) and int(torch.isnan(s).sum()) == 1
        g0 = g.clone()
        g0[3, 1] = 0.0
        gq, gt = torch.autograd.grad(s, (q, table), g)
        s_ok = sampled_scores(q, table, idx, "l1", C.GAMMA)
        wq, wt = torch.autograd.grad(s_ok, (q, table), g0)
        keep = torch.ones_like(s, dtype=torch.bool)
        keep[3, 1] = False
        assert C.bits_equal(s[keep].detach().numpy(), s_ok[keep].detach().numpy())
        assert C.bits_equal(gq.numpy(), wq.numpy()) and C.bits_equal(gt.numpy(), wt.numpy())
    # the torch route treats such an id alike
    s64 = sampled_scores(q.double(), table.double(), broken, "l1", C.GAMMA, check=False)
    assert torch.isnan(s64[3, 1]) and int(torch.isnan(s64).sum()) == 1


def test_refusals_and_the_torch_route():
    q, table, idx, _ = tensors("few_terms", grad=False)
    for args in ((q, table, idx, "conve"), (q[0], table, idx, "dot"), (q, table[:, :4], idx, "dot"), (q, table, idx[0], "dot"),
                 (q, table, idx.float(), "dot"), (q, table, idx[:0], "dot"), (q, table.double(), idx, "dot"),
                 (q.long(), table.long(), idx, "dot"), (q.numpy(), table, idx, "dot"),
                 (q[:, :5], table[:, :5], idx, "cl2")):
        with pytest.raises(ValueError):
            sampled_scores(*args)
    with pytest.raises(_lib.BackendError):
        sampled_scores(q.to("meta"), table, idx, "dot")
    with pytest.raises(_lib.BackendError):
        sampled_scores(q.to("meta"), table.to("meta"), idx.to("meta"), "dot", check=False)
    # other dtypes and empty operands run the gather composition
    for kind in C.KINDS:
        want = K.gather_composition(q.double(), table.double(), idx, kind, C.GAMMA)
        assert torch.equal(sampled_scores(q.double(), table.double(), idx, kind, C.GAMMA), want)
    assert sampled_scores(q[:0], table, idx[:0], "dot").shape == (0, 3)
    assert sampled_scores(q, table, idx[:, :0], "dot").shape == (1, 0)
    assert sampled_scores(q[:, :0], table[:, :0], idx, "l1", 2.0).tolist() == [[2.0, 2.0, 2.0]]
    assert torch.isnan(sampled_scores(q, table[:0], idx, "dot", check=False)).all()
    with pytest.raises(_lib.BackendError):
        sampled_scores(q, table[:0], idx, "dot")
    # a non-contiguous operand is read as its values
    wide = O.strided(q)
    assert C.bits_equal(sampled_scores(wide, table, idx, "dot").numpy(), sampled_scores(q, table, idx, "dot").numpy())


def test_c_abi_status_codes():
    """null, misaligned, invalid and empty arguments, in the order the entry points check them; the HIP entry points return
    every one of these before a launch, so they are asked without a GPU."""
    host, hip = _lib.host(), _lib.hip()
    q, table, idx, g = tensors("few_terms", grad=False)
    idx = idx.int()
    b, k = idx.shape
    n, d = table.shape
    out_s, out_q, out_t = torch.empty(b, k), torch.empty(b, d), torch.empty(n, d)
    ptr, pos = K.inverted_index(idx, n)
    P = lambda t: t.data_ptr()
    OK, EINVAL, EALIGN = 0, 1, 3  # COGDL_HIP_* (COGDL_HOST_OK / _EINVAL are the same numbers)
    assert hip.cogdl_hip_strerror(EINVAL) and hip.cogdl_hip_strerror(EALIGN)

    def score(lib, prefix, tail, q_=P(q), t_=P(table), i_=P(idx), o_=P(out_s), B=b, K_=k, N=n, D=d, kind=0):
        return getattr(lib, prefix + "kg_score")(q_, t_, i_, B, K_, N, D, kind, 0.0, o_, *tail)

    def grad_q(lib, prefix, tail, q_=P(q), t_=P(table), i_=P(idx), g_=P(g), o_=P(out_q), B=b, K_=k, N=n, D=d, kind=0):
        return getattr(lib, prefix + "kg_score_grad_q")(q_, t_, i_, g_, B, K_, N, D, kind, o_, *tail)

    def grad_t(lib, prefix, tail, q_=P(q), t_=P(table), g_=P(g), p_=P(ptr), s_=P(pos), o_=P(out_t), B=b, K_=k, N=n, D=d, kind=0):
        return getattr(lib, prefix + "kg_score_grad_table")(q_, t_, g_, p_, s_, B, K_, N, D, kind, o_, *tail)

    for lib, prefix, tail, ERANGE in ((host, "cogdl_host_", (), 2), (hip, "cogdl_hip_", (None,), 6)):  # COGDL_*_ERANGE
        for fn in (score, grad_q, grad_t):
            assert fn(lib, prefix, tail, kind=3) == EINVAL and fn(lib, prefix, tail, kind=-1) == EINVAL
            assert fn(lib, prefix, tail, B=-1) == EINVAL and fn(lib, prefix, tail, D=-1) == EINVAL
            assert fn(lib, prefix, tail, D=5, kind=2) == EINVAL                      # odd D with cl2
            assert fn(lib, prefix, tail, N=2 ** 31 - 1) == ERANGE
            assert fn(lib, prefix, tail, B=2 ** 16, K_=2 ** 15) == ERANGE            # B K at the int32 limit
            assert fn(lib, prefix, tail, q_=None) == EINVAL and fn(lib, prefix, tail, o_=None) == EINVAL
            assert fn(lib, prefix, tail, kind=3, q_=None) == EINVAL                  # sizes first
        # an empty output returns OK before any pointer is looked at
        assert score(lib, prefix, tail, B=0, q_=None, o_=None) == OK and score(lib, prefix, tail, K_=0, i_=None, o_=None) == OK
        assert grad_q(lib, prefix, tail, B=0, o_=None) == OK and grad_q(lib, prefix, tail, D=0, q_=None, o_=None) == OK
        assert grad_t(lib, prefix, tail, N=0, o_=None, p_=None) == OK and grad_t(lib, prefix, tail, D=0, o_=None) == OK
        assert score(lib, prefix, tail, i_=None) == EINVAL and grad_q(lib, prefix, tail, g_=None) == EINVAL
        assert grad_t(lib, prefix, tail, p_=None) == EINVAL and grad_t(lib, prefix, tail, s_=None) == EINVAL
    # the kernels' own conditions: 4-byte alignment (null before alignment), rows of at most 16384 floats
    tail, ERANGE = (None,), 6
    for fn in (score, grad_q, grad_t):
        assert fn(hip, "cogdl_hip_", tail, q_=P(q) + 2) == EALIGN and fn(hip, "cogdl_hip_", tail, o_=P(out_s) + 1) == EALIGN
        assert fn(hip, "cogdl_hip_", tail, q_=P(q) + 2, t_=None) == EINVAL
        assert fn(hip, "cogdl_hip_", tail, D=16385) == ERANGE
        assert fn(hip, "cogdl_hip_", tail, D=16385, q_=P(q) + 2) == EALIGN
    assert ctypes.sizeof(ctypes.c_void_p) == 8
    # the twin serves wider rows than the kernels
    wide_q, wide_t = torch.randn(1, 16400), torch.randn(2, 16400)
    s = sampled_scores(wide_q, wide_t, torch.tensor([[1, 0]]), "dot")
    terms = wide_q.double() * wide_t[[1, 0]].double()
    assert ((s[0].double() - terms.sum(1)).abs() <= C.gamma_n(16400 + 8) * terms.abs().sum(1)).all()
