"""Sampled triple scoring on the GPU: the HIP kernels of sampled_scores equal the host twin bit for bit -- scores, grad_q and
grad_table -- on every shared case of tests/_kgscore_cases.py and kind, with operands on 16 bytes (the 16-byte loads where D
allows) and 4 bytes into an allocation (the scalar loads): equal bits either way.  The memory the operator needs above its
inputs and outputs stays below a quarter of one [B, K, D] gather, which the torch composition exceeds several times over; the
served route raises no TorchRouteWarning, float64 exactly one."""
import warnings

import numpy as np
import pytest
import torch

import _kgscore_cases as C
import _offset as O
from cogdl_amd import _lib
from cogdl_amd.operators import kgscore as K
from cogdl_amd.operators import sampled_scores
from cogdl_amd.operators.ops import _ROUTE_NOTED, TorchRouteWarning

pytestmark = pytest.mark.gpu

DEV = "cuda"
_TWIN = {}


def twin(name, kind):
    """The host twin's (scores, grad_q, grad_table), once per case."""
    if (name, kind) not in _TWIN:
        c = C.make(name)
        q, table = torch.from_numpy(c["q"].copy()).requires_grad_(), torch.from_numpy(c["table"].copy()).requires_grad_()
        s = sampled_scores(q, table, torch.from_numpy(c["idx"].copy()), kind, C.GAMMA)
        gq, gt = torch.autograd.grad(s, (q, table), torch.from_numpy(c["g"].copy()))
        _TWIN[(name, kind)] = (s.detach().numpy(), gq.numpy(), gt.numpy())
    return _TWIN[(name, kind)]


def kernels(name, kind, elems):
    """sampled_scores forward + backward on the GPU with every operand `elems` floats past a 16-byte boundary, on the kernels'
    route (a TorchRouteWarning is an error), as numpy."""
    c = C.make(name)
    q, _ = O.shifted(torch.from_numpy(c["q"].copy()), elems, device=DEV)
    table, _ = O.shifted(torch.from_numpy(c["table"].copy()), elems, device=DEV)
    idx, _ = O.shifted(torch.from_numpy(c["idx"].astype(np.int32)), elems, device=DEV)
    g, _ = O.shifted(torch.from_numpy(c["g"].copy()), elems, device=DEV)
    assert q.data_ptr() % 16 == 4 * elems and table.data_ptr() % 16 == 4 * elems
    q.requires_grad_()
    table.requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = sampled_scores(q, table, idx, kind, C.GAMMA)
        gq, gt = torch.autograd.grad(s, (q, table), g)
    assert s.is_cuda and gq.is_cuda and gt.is_cuda
    return s.detach().cpu().numpy(), gq.cpu().numpy(), gt.cpu().numpy()


@pytest.mark.parametrize("name,kind", C.CASES)
def test_kernels_equal_the_twin_bit_for_bit_on_both_load_paths(name, kind):
    want = twin(name, kind)
    for elems in (0, 1):
        got = kernels(name, kind, elems)
        for what, a, b in zip(("scores", "grad_q", "grad_table"), got, want):
            assert C.bits_equal(a, b), (what, "offset %d floats" % elems, float(np.abs(a - b).max()))


def test_int64_ids_unchecked_ids_and_run_to_run():
    c = C.make("many_j_250")
    q, table = torch.from_numpy(c["q"].copy()).to(DEV), torch.from_numpy(c["table"].copy()).to(DEV)
    idx, g = torch.from_numpy(c["idx"].copy()).to(DEV), torch.from_numpy(c["g"].copy()).to(DEV)
    q.requires_grad_()
    table.requires_grad_()
    outs = []
    for _ in range(2):
        s = sampled_scores(q, table, idx, "cl2", C.GAMMA)
        outs.append([t.detach().cpu().numpy() for t in (s,) + torch.autograd.grad(s, (q, table), g)])
    assert all(C.bits_equal(a, b) for a, b in zip(*outs)) and all(C.bits_equal(a, b) for a, b in zip(outs[0], twin("many_j_250", "cl2")))
    broken = idx.clone()
    broken[3, 1], broken[5, 0] = -1, table.shape[0]
    with pytest.raises(_lib.BackendError):
        sampled_scores(q, table, broken, "cl2", C.GAMMA)
    s = sampled_scores(q, table, broken, "cl2", C.GAMMA, check=False)
    gq, gt = torch.autograd.grad(s, (q, table), g)
    qc, tc = q.detach().cpu().requires_grad_(), table.detach().cpu().requires_grad_()
    sc = sampled_scores(qc, tc, broken.cpu(), "cl2", C.GAMMA, check=False)
    wq, wt = torch.autograd.grad(sc, (qc, tc), g.cpu())
    assert int(torch.isnan(s).sum()) == 2 and bool(torch.isnan(s[3, 1])) and bool(torch.isnan(s[5, 0]))
    assert np.array_equal(s.detach().cpu().numpy(), sc.detach().numpy(), equal_nan=True)
    assert C.bits_equal(gq.cpu().numpy(), wq.numpy()) and C.bits_equal(gt.cpu().numpy(), wt.numpy())


def test_memory_stays_below_a_quarter_of_the_gather():
    b, k, d, n = 64, 64, 512, 1000
    limit = b * k * d * 4 // 4
    gen = torch.Generator().manual_seed(5)
    q = torch.randn(b, d, generator=gen).to(DEV).requires_grad_()
    table = torch.randn(n, d, generator=gen).to(DEV).requires_grad_()
    idx = torch.randint(0, n, (b, k), generator=gen).to(DEV)
    g = torch.randn(b, k, generator=gen).to(DEV)

    def extra(fn):
        """peak allocated bytes during forward + backward above the inputs and the three outputs"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        s = fn()
        gq, gt = torch.autograd.grad(s, (q, table), g)
        torch.cuda.synchronize()
        outputs = sum(t.numel() * t.element_size() for t in (s, gq, gt))
        return torch.cuda.max_memory_allocated() - base - outputs

    for kind in C.KINDS:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ours = extra(lambda: sampled_scores(q, table, idx, kind, C.GAMMA))
        torchs = extra(lambda: K.gather_composition(q, table, idx, kind, C.GAMMA))
        print("%s: operator %d bytes, torch composition %d bytes, limit %d" % (kind, ours, torchs, limit))
        assert ours < limit, kind
        assert torchs > 4 * limit, kind  # at least the [B, K, D] gather itself


def test_one_warning_for_float64_none_on_the_served_route():
    for key in [key for key in _ROUTE_NOTED if key[0] == "sampled_scores"]:
        _ROUTE_NOTED.discard(key)
    c = C.make("few_terms")
    q, table, idx = (torch.from_numpy(c[k].copy()).to(DEV) for k in ("q", "table", "idx"))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        sampled_scores(q, table, idx, "dot")
        a = sampled_scores(q.double(), table.double(), idx, "l1", C.GAMMA)
        sampled_scores(q.double(), table.double(), idx, "cl2", C.GAMMA)
    assert [w.category for w in seen] == [TorchRouteWarning] and "float64" in str(seen[0].message)
    es = C.exact("few_terms", "l1")[0]
    assert np.abs(a.cpu().numpy() - es).max() <= 1e-12
