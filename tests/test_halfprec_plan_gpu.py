"""The 16-bit launches over XCD plans (xcdplan.MODE = "force"), held to "fp32 arithmetic, rounded once, to nearest, on store"
(include/cogdl_hip.h): csr_spmm (csr_spmm_xcd_raw; SPMMFunction in both directions) and the fused GAT operator
(cogdl_hip_gat_fwd_xcd / _bwd_xcd), on the graphs of tests/test_xcd_gpu.py -- the smallest that reach every merge path of a plan.

csr_spmm: every output within  0.5 * ulp(|want| + slack) + slack  of the float64 result on the rounded inputs (tests/_halfprec.py;
terms = the row's degree, + 1 for out +=: a plan re-associates a long row into fp32 part records and merges them, which the
any-order summation bound covers), and -- with integer data, where every fp32 partial sum in any order is exact -- EQUAL to the
exact sum rounded once, ties included: that pins the irrelevance of the merge order and the store rounding together.
What the widths reach (spmm_geometry with 16-byte lanes allowed, csrc/spmm.hip; (vec, lanes per row); f16 and bf16 alike):
k = 1 (1, 4), 7 (1, 8), 2 (2, 4), 16 (2, 8: narrowed), and the 16-byte lanes only the plan launch has: 40 (8, 8: five of the
eight lanes busy), 64 (8, 8), 200 (8, 32: 25 busy); one column tile each.  Rows of at most SPLIT = 256 edges stay whole,
longer ones are cut by owner XCD into pieces of at most 512 edges, row 100 of the hub graph into ~80 parts (merged by a whole
workgroup), the one-owner graph's long rows into parts of a single XCD.

Fused GAT: the inputs, oracle calls and bounds of tests/_gat_halfprec.py (as tests/test_halfprec_gat_gpu.py) on the square
versions of the hub and one-owner graphs.  Both plan entries take f16 as they take bf16 (csrc/gat.hip dispatches on the dtype code;
nothing is declined for the type), so both are run; the test spies on the C entry points and states which ran: with the operator's
padding every shape here is a single column tile -- forward (8, 8 lanes, 1 tile), backward one group at vec 8 -- so BOTH passes
run the plan kernels and the ordinary entries are never called.  Not reached in 16 bits over a plan: the raw (unpadded) widths
-- vec 1 / 2 / 4 lanes of the plan kernels -- and H > 8."""
import functools

import numpy as np
import pytest
import torch

import _gat_halfprec as gat16
import _halfprec as hp
import _xcd_graphs
from cogdl_amd import _lib, xcdplan
from cogdl_amd.operators.spmm import SPMMFunction, csr_spmm_xcd_raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
WIDTHS = [1, 2, 7, 16, 40, 64, 200]


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "force")
    xcdplan.XPLANS.clear()
    yield
    xcdplan.XPLANS.clear()


@functools.lru_cache(maxsize=None)
def _graph(kind):
    g = _xcd_graphs.graph(kind)
    return g, g.degrees().numpy()


@functools.lru_cache(maxsize=None)
def _plan(kind):
    g, _ = _graph(kind)
    return xcdplan.build(g.rowptr.to(DEV), g.colind.to(DEV))


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _refs(oracle, g, w, x):
    """float64 (want, scale) of A x for the 16-bit tensors w (or None) and x."""
    rp, ci, xf = g.rowptr.numpy(), g.colind.numpy(), x.float().numpy()
    wf = None if w is None else w.float().numpy()
    return oracle.csr_spmm_f64(rp, ci, wf, xf), oracle.csr_spmm_abs(rp, ci, wf, xf)


# ------------------------------------------------------------------------------------------------------------ csr_spmm
@pytest.mark.parametrize("kind", _xcd_graphs.KINDS)
@DTYPES
@pytest.mark.parametrize("k", WIDTHS)
def test_csr_spmm_xcd_within_half_an_ulp(oracle, kind, dtype, k):
    (g, deg), plan = _graph(kind), _plan(kind)
    gen = torch.Generator().manual_seed(k)
    x = torch.randn(g.n_cols, k, generator=gen).to(dtype)
    w = g.weight.to(dtype)
    base = torch.randn(g.num_nodes, k, generator=gen).to(dtype)
    for name, val in (("weighted", w), ("unweighted", None)):
        want, scale = _refs(oracle, g, val, x)
        got = csr_spmm_xcd_raw(plan, None if val is None else val.to(DEV), x.to(DEV))
        assert got.dtype == dtype and got.shape == (g.num_nodes, k)
        hp.assert_close(got, want, scale, deg[:, None], dtype, "%s %s k=%d" % (kind, name, k))
        assert torch.equal(got, csr_spmm_xcd_raw(plan, None if val is None else val.to(DEV), x.to(DEV)))  # fixed merge order
        # out += A x: the sum continues from the stored 16-bit value (one more term), rounded once
        out = base.clone().to(DEV)
        res = csr_spmm_xcd_raw(plan, None if val is None else val.to(DEV), x.to(DEV), out=out)
        assert res.data_ptr() == out.data_ptr()
        hp.assert_close(res, want + _np64(base), scale + np.abs(_np64(base)), deg[:, None] + 1, dtype,
                        "%s %s accumulate k=%d" % (kind, name, k))


@pytest.mark.parametrize("kind", _xcd_graphs.KINDS)
@DTYPES
@pytest.mark.parametrize("k", WIDTHS)
def test_csr_spmm_xcd_integer_data_is_the_exact_sum_rounded_once(oracle, kind, dtype, k):
    """Weights and features in {-2 .. 2}: every product and every fp32 partial sum is an integer below 2^24, whatever the order
    -- whole rows (at most SPLIT edges) and rows merged from many part records alike have to be the exact sum, cast once
    (hp.assert_exact: no slack; on the hub rows sums beyond 256 are odd half the time, and an odd sum there is a tie in bf16).
    The accumulation target holds integers up to 3000 (even beyond 256 in bf16, beyond 2048 in f16), so that out += ties in
    short rows and in f16 too.  An f16 sum beyond 65504 would correctly be inf: with this data none is."""
    (g, deg), plan = _graph(kind), _plan(kind)
    assert (deg <= xcdplan.SPLIT).sum() > 10 and (kind == "short" or plan.n_parts > 0)
    gen = torch.Generator().manual_seed(100 + k)
    x = torch.randint(-2, 3, (g.n_cols, k), generator=gen).to(dtype)
    w = torch.randint(-2, 3, (g.nnz,), generator=gen).to(dtype)
    base = torch.randint(-3000, 3001, (g.num_nodes, k), generator=gen).to(dtype)
    unrepresentable = 0
    for name, val in (("weighted", w), ("unweighted", None)):
        want, scale = _refs(oracle, g, val, x)
        got = csr_spmm_xcd_raw(plan, None if val is None else val.to(DEV), x.to(DEV))
        hp.assert_exact(got, want, scale, dtype, "%s %s k=%d" % (kind, name, k))
        res = csr_spmm_xcd_raw(plan, None if val is None else val.to(DEV), x.to(DEV), out=base.clone().to(DEV))
        want_acc = want + _np64(base)
        hp.assert_exact(res, want_acc, scale + np.abs(_np64(base)), dtype, "%s %s accumulate k=%d" % (kind, name, k))
        for exact in (want, want_acc):
            cast = torch.from_numpy(exact).to(dtype)
            assert float(torch.isinf(cast).float().mean()) <= 0.01
            unrepresentable += int((cast.double().numpy() != exact).sum())
    assert unrepresentable > 0  # (the accumulating launches always round: the check is not vacuous)


@pytest.mark.parametrize("kind", ["hubs", "rect"])
@DTYPES
def test_spmm_function_takes_the_plan_in_both_directions_16bit(oracle, dtype, kind, monkeypatch):
    """SPMMFunction with the plan forced: forward over the CSR plan, grad_x over the plan of the transpose -- two plan launches,
    counted -- both within half an ulp; grad_x against an independently built transpose (scipy) in float64.  The hub graph's
    transpose has no row beyond SPLIT (its plan is whole rows only); the rectangular graph's has nothing else (97 columns of
    ~700 edges: every row of the transpose is cut by owner and merged)."""
    import scipy.sparse as sp

    import cogdl_amd.operators.spmm as spmm_mod

    g, deg = _graph(kind)
    calls = []
    real = spmm_mod.csr_spmm_xcd_raw
    monkeypatch.setattr(spmm_mod, "csr_spmm_xcd_raw", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    gen = torch.Generator().manual_seed(32)
    x0 = torch.randn(g.n_cols, 32, generator=gen).to(dtype)
    gout = torch.randn(g.num_nodes, 32, generator=gen).to(dtype)
    w0 = g.weight.to(dtype)
    x = x0.to(DEV).requires_grad_()
    out = SPMMFunction.apply(g.rowptr.to(DEV), g.colind.to(DEV), x, w0.to(DEV), False)
    out.backward(gout.to(DEV))
    assert len(calls) == 2
    assert out.dtype == dtype and x.grad.dtype == dtype
    want, scale = _refs(oracle, g, w0, x0)
    hp.assert_within(_np64(out), want, hp.bound(want, scale, deg[:, None], dtype), "forward")
    rp, ci = g.rowptr.numpy(), g.colind.numpy()
    at = sp.csr_matrix((_np64(w0), ci, rp), shape=(g.num_nodes, g.n_cols)).T.tocsr()
    gn = _np64(gout)
    col_deg = np.bincount(ci, minlength=g.n_cols)
    assert (col_deg.min() > xcdplan.SPLIT) == (kind == "rect") and (col_deg.max() <= xcdplan.SPLIT) == (kind == "hubs")
    want_x, scale_x = at @ gn, abs(at) @ np.abs(gn)
    hp.assert_within(_np64(x.grad), want_x, hp.bound(want_x, scale_x, col_deg[:, None], dtype), "grad_x")


# ------------------------------------------------------------------------------------------------------------ fused GAT
GAT_KINDS = {"xcd-hubs": "hubs", "xcd-one_owner": "one_owner"}
for _name, _kind in GAT_KINDS.items():
    # (both graphs have rows of hundreds to thousands of edges: the hub graphs' S_REL)
    gat16.register(_name, functools.partial(lambda kind: _xcd_graphs.square(_xcd_graphs.graph(kind)), _kind), gat16.S_REL["hubs"])
GAT_ENTRIES = ("cogdl_hip_gat_fwd_xcd", "cogdl_hip_gat_bwd_xcd", "cogdl_hip_gat_fwd", "cogdl_hip_gat_dropout_fwd", "cogdl_hip_gat_bwd",
               "cogdl_hip_gat_dropout_bwd")


@pytest.fixture
def gat_entries(monkeypatch):
    """Counts the calls of the fused GAT entry points and keeps their status codes."""
    lib, seen = _lib.hip(), []

    def spy(name, real):
        def call(*args):
            rc = real(*args)
            seen.append((name, rc))
            return rc
        return call

    for name in GAT_ENTRIES:
        monkeypatch.setattr(lib, name, spy(name, getattr(lib, name)))
    return seen


@pytest.mark.parametrize("kind", list(GAT_KINDS))
@DTYPES
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("h,f", [(8, 8), (1, 41), (4, 16), (3, 5)])
def test_fused_gat_xcd_16bit_within_half_an_ulp(gat_entries, kind, dtype, p, h, f):
    gat16.check(kind, h, f, dtype, p, True)
    # the plan kernels are the ones that ran, in both passes: no entry declined, the ordinary entries were not called
    assert gat_entries == [("cogdl_hip_gat_fwd_xcd", 0), ("cogdl_hip_gat_bwd_xcd", 0)], gat_entries
