"""f16 / bf16 csr_spmm and mhspmm at their ORDINARY launches (no XCD plan), held to "fp32 arithmetic, rounded once, to
nearest, on store" (include/cogdl_hip.h): every output within half an ulp of the float64 result on the rounded inputs plus
the fp32 summation error (tests/_halfprec.py; nothing in the bound is measured).

What the widths reach for 2-byte elements (spmm_geometry, csrc/spmm.hip; (vec, lanes per row, column tiles)):
    csr_spmm  k = 1 (1, 4, 1)   2 (2, 4, 1)   6 (2, 4, 1)   7 (1, 8, 1)   15 (1, 16, 1)   16 (2, 8, 1: narrowed from vec 4)
              31 (1, 32, 1)   32 (2, 16, 1: narrowed)   40 (4, 16, 1)   41 (1, 64, 1)   50 (2, 32, 1)   64 (4, 16, 1)
              80 (4, 20, 1: the group that does not divide the wave)   128 (4, 32, 1)   300 (4, 64, 2: ragged)   602 (2, 64, 5: ragged)
              2 bytes into the storage: 8 (1, 8, 1), 20 (1, 20, 1), 64 (1, 64, 1);  4 bytes into it: 40 (2, 20, 1)
              -- every (vec, lanes) pair the ordinary 16-bit launch can choose: vec 1 and 2 at 4 to 64 lanes and at 20, vec 4 at
              16 to 64 and at 20 (vec 4 below 16 lanes is narrowed to vec 2; vec 8 belongs to the XCD plans)
    mhspmm    (8, 8) (4, 16, 1)   (1, 41) (1, 64, 1)   (3, 5) (1, 16, 1)   (2, 16) (2, 16, 1)   (4, 6) (2, 16, 1)   (16, 2) (2, 16, 1)
              (6, 12) (4, 32, 1)   (8, 64) (4, 64, 2)
vec >= 2 takes the raw-word mask and fused multiply-adds of SpmmOp::apply, vec 1 the per-element select and multiply-then-add.
The hub graph's rows beyond cogdl_hip_exact_row_edges (128 here) take the long-row path (fp32 piece records, fixed order)."""
import functools

import numpy as np
import pytest
import torch

import _halfprec as hp
from cogdl_amd import _lib, synth, xcdplan
from cogdl_amd.operators.mhspmm import csrmhspmm, mhspmm_raw
from cogdl_amd.operators.spmm import csr_spmm_raw, csrspmm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
GRAPHS = pytest.mark.parametrize("kind", ["random", "hubs"])
HUBS = ((3, 129), (4, 1000), (17, 5000), (18, 257), (40, 128))


@pytest.fixture(autouse=True)
def ordinary_launch(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")  # (the default: these graphs are far below any plan's size)


@functools.lru_cache(maxsize=None)
def _graph(kind):
    if kind == "random":
        g = synth.random_csr(301, 257, 9)
    elif kind == "hubs":
        g = synth.hub_csr(60, 90, hubs=HUBS)
    elif kind == "mh-random":
        g = synth.random_csr(120, 100, 8)
    else:
        raise KeyError(kind)
    deg = g.degrees().numpy()
    if kind == "hubs":
        assert exact_edges(g.nnz) == 128 and (deg > 128).sum() == 4 and (deg == 128).sum() >= 1
    return g, deg


def exact_edges(nnz):
    return int(_lib.hip().cogdl_hip_exact_row_edges(int(nnz)))


def _d(t):
    return None if t is None else t.to(DEV)


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(kind, k, dtype):
    """Inputs (rounded to dtype) and the float64 references of one (graph, width, dtype), computed once and never modified."""
    from oracle import oracle

    g, deg = _graph(kind)
    gen = torch.Generator().manual_seed(1000 + k)
    x = torch.randn(g.n_cols, k, generator=gen).to(dtype)
    w = g.weight.to(dtype)
    rp, ci = g.rowptr.numpy(), g.colind.numpy()
    xf, wf = x.float().numpy(), w.float().numpy()
    ref = {"w": (oracle.csr_spmm_f64(rp, ci, wf, xf), oracle.csr_spmm_abs(rp, ci, wf, xf)),
           "u": (oracle.csr_spmm_f64(rp, ci, None, xf), oracle.csr_spmm_abs(rp, ci, None, xf))}
    for pair in ref.values():
        for a in pair:
            a.setflags(write=False)
    return g, deg, x, w, ref


def _spmm(g, val, x, **kw):
    return csr_spmm_raw(_d(g.rowptr), _d(g.colind), _d(val), _d(x), **kw)


# ------------------------------------------------------------------------------------------------------------ csr_spmm
@GRAPHS
@DTYPES
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
@pytest.mark.parametrize("k", [1, 2, 6, 7, 16, 32, 40, 41, 80, 128, 300, 602, 15, 31, 50])
def test_csr_spmm_widths_within_half_an_ulp(oracle, kind, dtype, weighted, k):
    g, deg, x, w, ref = _case(kind, k, dtype)
    want, scale = ref["w" if weighted else "u"]
    got = _spmm(g, w if weighted else None, x)
    assert got.dtype == dtype and got.shape == (g.num_nodes, k)
    hp.assert_close(got, want, scale, deg[:, None], dtype, "csr_spmm %s k=%d" % (kind, k))
    assert torch.equal(got, _spmm(g, w if weighted else None, x))  # no atomics: run-to-run identical


@GRAPHS
@DTYPES
@pytest.mark.parametrize("k", [7, 16, 80, 300])
def test_csr_spmm_unweighted_rows_equal_the_fp32_sum_rounded_once(oracle, kind, dtype, k):
    """val = NULL: the kernel only adds, in CSR order, in both arithmetic paths -- rows up to the exact-row bound are the
    fp32 reference loop's result, rounded once."""
    g, deg, x, _, _ = _case(kind, k, dtype)
    want = torch.from_numpy(oracle.csr_spmm(g.rowptr, g.colind, None, x.float())).to(dtype)
    got = _spmm(g, None, x).cpu()
    short = torch.from_numpy(deg <= exact_edges(g.nnz))
    assert short.sum() >= 56
    assert torch.equal(got[short], want[short])


@DTYPES
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
@pytest.mark.parametrize("k", [7, 16, 80, 300])
def test_csr_spmm_long_rows_with_and_without_workspace(oracle, dtype, weighted, k):
    """Without the workspace every row is summed sequentially; with it rows beyond the exact-row bound are pieces combined in
    a fixed order: the short rows do not notice, the long ones stay inside the bound either way."""
    g, deg, x, w, ref = _case("hubs", k, dtype)
    want, scale = ref["w" if weighted else "u"]
    val = w if weighted else None
    seq, split = _spmm(g, val, x, split_long_rows=False), _spmm(g, val, x, split_long_rows=True)
    short = torch.from_numpy(deg <= exact_edges(g.nnz)).to(DEV)
    assert torch.equal(seq[short], split[short])
    long_ = ~short.cpu().numpy()
    for name, got in (("sequential", seq), ("pieces", split)):
        hp.assert_close(got.cpu()[long_], want[long_], scale[long_], deg[long_, None], dtype, "%s k=%d" % (name, k))


@GRAPHS
@DTYPES
@pytest.mark.parametrize("k", [7, 64, 80])
def test_csr_spmm_accumulate(oracle, kind, dtype, k):
    """out += A x: the sum continues from the stored 16-bit value (one more term), rounded once."""
    g, deg, x, w, ref = _case(kind, k, dtype)
    want, scale = ref["w"]
    base = torch.randn(g.num_nodes, k, generator=torch.Generator().manual_seed(k)).to(dtype)
    out = base.clone().to(DEV)
    res = _spmm(g, w, x, out=out)
    assert res.data_ptr() == out.data_ptr()
    hp.assert_close(res, want + _np64(base), scale + np.abs(_np64(base)), deg[:, None] + 1, dtype, "accumulate k=%d" % k)


@DTYPES
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
@pytest.mark.parametrize("k", [7, 80])
def test_csr_spmm_row_order_changes_no_bit(dtype, weighted, k):
    g, deg, x, w, _ = _case("hubs", k, dtype)
    val = w if weighted else None
    plain = _spmm(g, val, x)
    m = g.num_nodes
    orders = {"random": torch.randperm(m, generator=torch.Generator().manual_seed(3)),
              "by degree": torch.argsort(torch.from_numpy(deg), descending=True, stable=True)}
    for name, order in orders.items():
        assert torch.equal(_spmm(g, val, x, row_order=order.int().to(DEV)), plain), name
        base = torch.ones(m, k).to(dtype)
        assert torch.equal(_spmm(g, val, x, row_order=order.int().to(DEV), out=base.to(DEV)), _spmm(g, val, x, out=base.to(DEV))), name


@DTYPES
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
@pytest.mark.parametrize("k", [7, 16, 64])
def test_csr_spmm_non_finite_inputs(oracle, dtype, weighted, k):
    """Row 0 of x is all NaN -- the row masked slots and lanes past the last column read -- so a mask that lets anything
    through poisons rows that never name column 0.  vec >= 2 (k = 16, 64) masks the raw 32-bit words, vec 1 (k = 7) selects
    per element."""
    g = synth.random_csr(97, 64, 5, seed=11)  # degrees 0 .. 10: most are no multiple of the 8- or 16-lane group's chunk
    colind = g.colind.clone()
    row = torch.repeat_interleave(torch.arange(97), g.degrees())
    colind[(colind == 0) & (row % 2 == 1)] = 1  # odd rows never reference column 0
    touched = torch.zeros(97, dtype=torch.bool)
    touched[row[colind == 0]] = True
    assert touched.any() and not touched[1::2].any() and (g.degrees()[1::2] > 0).any()
    x = torch.randn(64, k, generator=torch.Generator().manual_seed(k)).to(dtype)
    x[0, :] = float("nan")
    x[3, 5] = float("inf")
    x[20, 0] = -float("inf")
    w = g.weight.to(dtype) if weighted else None
    wf = None if w is None else w.float().numpy()
    with np.errstate(invalid="ignore"):
        want = oracle.csr_spmm_f64(g.rowptr, colind, wf, x.float())
        scale = oracle.csr_spmm_abs(g.rowptr, colind, wf, x.float())
    got = csr_spmm_raw(_d(g.rowptr), _d(colind), _d(w), _d(x)).float().cpu().numpy().astype(np.float64)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert not np.isnan(got[~touched.numpy()][:, 1:5]).any()  # (columns no inf sits in)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    deg = np.broadcast_to(g.degrees().numpy()[:, None], want.shape)
    hp.assert_close(got[fin], want[fin], scale[fin], deg[fin], dtype, "finite elements k=%d" % k)


def _edge_graph(cols_of_rows, n_cols):
    deg = torch.tensor([len(c) for c in cols_of_rows])
    rowptr = torch.zeros(len(cols_of_rows) + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    colind = torch.tensor([c for cols in cols_of_rows for c in cols], dtype=torch.int32)
    return rowptr, colind


@pytest.mark.parametrize("k", [7, 16, 64])
def test_csr_spmm_range_edges(oracle, k):
    """The store at the ends of the range, on short rows, equal to the fp32 reference loop's result cast once: f16 sums
    beyond 65504 (and the tie at 65520) store inf; sums of f16 subnormals keep their bits, and quarter-weighted ones round
    to even in the subnormal range; bf16 sums near 3e38 stay finite up to the tie against 2^128."""
    # ---- f16
    vals = [30000.0, 32768.0, 16.0, 65504.0, 8.0, 2.0 ** -20, 3 * 2.0 ** -24, 2.0 ** -24, 5 * 2.0 ** -22, -(2.0 ** -21), 1.0, -65504.0]
    col = torch.tensor(vals).to(torch.float16)
    assert torch.equal(col.float(), torch.tensor(vals))  # all representable
    fac = torch.tensor([1.0, 0.5, 1.0, 0.25])[torch.arange(k) % 4]
    x = (col.float()[:, None] * fac[None, :]).to(torch.float16)
    rows = [[0, 0, 0], [0, 1], [1, 1], [3, 2], [3, 4], [3, 2, 4], [11, 2], [11, 2, 2], [5, 6], [7, 7, 7], [5, 6, 7, 8, 9], [6, 7, 9],
            [10, 5], [], [8, 9, 9, 6, 6, 6, 7]]
    rowptr, colind = _edge_graph(rows, len(vals))
    want = torch.from_numpy(oracle.csr_spmm(rowptr, colind, None, x.float())).to(torch.float16)
    assert bool(torch.isinf(want).any()) and bool(((want != 0) & (want.abs() < 2.0 ** -14)).any())
    assert float(want[3, 0]) == float("inf") and float(want[4, 0]) == 65504.0  # 65520 ties to even = inf; 65512 rounds down
    got = csr_spmm_raw(_d(rowptr), _d(colind), None, _d(x)).cpu()
    assert torch.equal(got, want)
    # power-of-two weights: every product and sum is exact in fp32 (no difference between fma and multiply-add), the store
    # rounds multiples of 2^-26 to multiples of 2^-24
    w = torch.tensor([0.25, 0.5, 0.125])[torch.arange(colind.numel()) % 3].to(torch.float16)
    sub = [8, 9, 10, 11, 14]
    want_w = torch.from_numpy(oracle.csr_spmm(rowptr, colind, w.float(), x.float())).to(torch.float16)
    got_w = csr_spmm_raw(_d(rowptr), _d(colind), _d(w), _d(x)).cpu()
    assert torch.equal(got_w[sub], want_w[sub])
    # ---- bf16
    big = float(torch.finfo(torch.bfloat16).max)
    vals = [1e38, big, 2.0 ** 119, 2.0 ** 118, -big, 1.5e38, 1.0]
    col = torch.tensor(vals).to(torch.bfloat16)
    x = (col.float()[:, None] * fac[None, :]).to(torch.bfloat16)
    rows = [[0, 0, 0], [0, 0, 0, 0], [1, 2], [1, 3], [4, 2], [4, 3], [5, 5], [5, 0], [1, 6], [], [0, 5, 6]]
    rowptr, colind = _edge_graph(rows, len(vals))
    want = torch.from_numpy(oracle.csr_spmm(rowptr, colind, None, x.float())).to(torch.bfloat16)
    assert float(want[2, 0]) == float("inf") and float(want[3, 0]) == big and float(want[0, 0]) > 2.9e38
    got = csr_spmm_raw(_d(rowptr), _d(colind), None, _d(x)).cpu()
    assert torch.equal(got, want)


def _offset_view(t, elems=1):
    """A copy of `t` that starts `elems` elements into its storage (a contiguous view of a bigger 1-D buffer)."""
    store = torch.empty(t.numel() + elems, dtype=t.dtype, device=DEV)
    view = store[elems:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == elems * t.element_size()
    return view


@GRAPHS
@DTYPES
@pytest.mark.parametrize("k,elems", [(8, 1), (64, 1), (20, 1), (40, 2)])
def test_csr_spmm_operands_two_bytes_into_their_storage(oracle, kind, dtype, k, elems):
    """x (and the out= target) 2 bytes into an allocation: the geometry falls back to one element per lane -- the other
    arithmetic path, so not necessarily the aligned call's bits, but the same bound ((40, 2): 4 bytes in, two elements per
    lane in groups of 20).  Unweighted rows only add on either path: bit for bit the fp32 loop's result rounded once."""
    g, deg, _, w, _ = _case(kind, 7, dtype)
    gen = torch.Generator().manual_seed(k)
    x = torch.randn(g.n_cols, k, generator=gen).to(dtype)
    base = torch.randn(g.num_nodes, k, generator=gen).to(dtype)
    rp, ci, wf, xf = g.rowptr.numpy(), g.colind.numpy(), w.float().numpy(), x.float().numpy()
    want, scale = oracle.csr_spmm_f64(rp, ci, wf, xf), oracle.csr_spmm_abs(rp, ci, wf, xf)
    got = csr_spmm_raw(_d(g.rowptr), _d(g.colind), _d(w), _offset_view(x, elems))
    hp.assert_close(got, want, scale, deg[:, None], dtype, "misaligned x, k=%d" % k)
    for xin in (_offset_view(x, elems), _d(x)):
        out = _offset_view(base, elems)
        csr_spmm_raw(_d(g.rowptr), _d(g.colind), _d(w), xin, out=out)
        hp.assert_close(out, want + _np64(base), scale + np.abs(_np64(base)), deg[:, None] + 1, dtype, "misaligned out, k=%d" % k)
    short = torch.from_numpy(deg <= exact_edges(g.nnz))
    want_u = torch.from_numpy(oracle.csr_spmm(rp, ci, None, xf)).to(dtype)
    got_u = csr_spmm_raw(_d(g.rowptr), _d(g.colind), None, _offset_view(x, elems)).cpu()
    assert torch.equal(got_u[short], want_u[short])
    out = _offset_view(torch.zeros(g.num_nodes, k).to(dtype), elems)
    csr_spmm_raw(_d(g.rowptr), _d(g.colind), None, _offset_view(x, elems), out=out)
    assert torch.equal(out.cpu()[short], want_u[short])


@GRAPHS
@pytest.mark.parametrize("k", [8, 64])
def test_csr_spmm_fp32_operands_four_bytes_into_their_storage_stay_bit_exact(oracle, kind, k):
    g, deg = _graph(kind)
    x = torch.randn(g.n_cols, k, generator=torch.Generator().manual_seed(k))
    want = oracle.csr_spmm(g.rowptr, g.colind, g.weight, x)
    short = deg <= exact_edges(g.nnz)
    # (without the workspace every row is sequential: bit-exact at any length)
    got = csr_spmm_raw(_d(g.rowptr), _d(g.colind), _d(g.weight), _offset_view(x), split_long_rows=False)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    got = csr_spmm_raw(_d(g.rowptr), _d(g.colind), _d(g.weight), _offset_view(x))
    assert got.cpu().numpy()[short].tobytes() == want[short].tobytes()
    out = _offset_view(torch.zeros(g.num_nodes, k))
    csr_spmm_raw(_d(g.rowptr), _d(g.colind), _d(g.weight), _offset_view(x), out=out)
    assert out.cpu().numpy()[short].tobytes() == want[short].tobytes()


@DTYPES
@pytest.mark.parametrize("k", [7, 32])
def test_csrspmm_autograd_16bit(oracle, dtype, k, monkeypatch):
    """SPMMFunction with 16-bit features and weights on a rectangular operand: grad_x = A^T g through the cached transpose
    (one 16-bit csr_spmm launch), grad_w = the fp32 dot products rounded once to the weights' dtype."""
    import scipy.sparse as sp

    import cogdl_amd.operators.spmm as spmm_mod
    from cogdl_amd.plan import PLANS

    PLANS.clear()
    xcdplan.XPLANS.clear()
    taken = []
    real = spmm_mod.csr_spmm_xcd_raw
    monkeypatch.setattr(spmm_mod, "csr_spmm_xcd_raw", lambda *a, **kw: (taken.append(1), real(*a, **kw))[1])
    g, deg, x0, w0, ref = _case("hubs", k, dtype)
    m, n = g.num_nodes, g.n_cols
    assert m != n
    x, w = _d(x0).requires_grad_(), _d(w0).requires_grad_()
    gout = torch.randn(m, k, generator=torch.Generator().manual_seed(5)).to(dtype)
    out = csrspmm(_d(g.rowptr), _d(g.colind), x, w)
    out.backward(_d(gout))
    assert not taken
    hp.assert_close(out, ref["w"][0], ref["w"][1], deg[:, None], dtype, "forward")
    rp, ci = g.rowptr.numpy(), g.colind.numpy()
    at = sp.csr_matrix((_np64(w0), ci, rp), shape=(m, n)).T.tocsr()
    gn = _np64(gout)
    col_deg = np.bincount(ci, minlength=n)
    assert x.grad.dtype == dtype and col_deg.max() > 64
    hp.assert_close(x.grad, at @ gn, abs(at) @ np.abs(gn), col_deg[:, None], dtype, "grad_x")
    row = np.repeat(np.arange(m), deg)
    terms = gn[row] * _np64(x0)[ci]
    assert w.grad.dtype == w0.dtype == dtype
    hp.assert_close(w.grad, terms.sum(1), np.abs(terms).sum(1), k, dtype, "grad_w")
    PLANS.clear()


# -------------------------------------------------------------------------------------------------------------- mhspmm
MH_SHAPES = [(8, 8), (1, 41), (3, 5), (2, 16), (4, 6), (16, 2), (6, 12), (8, 64)]


@functools.lru_cache(maxsize=None)
def _mh_case(kind, h, f, dtype):
    g, deg = _graph(kind)
    gen = torch.Generator().manual_seed(100 * h + f)
    att = torch.rand(g.nnz, h, generator=gen)
    feat = torch.randn(g.n_cols, h, f, generator=gen).to(dtype)
    gout = torch.randn(g.num_nodes, h, f, generator=gen).to(dtype)
    row = np.repeat(np.arange(g.num_nodes), deg)
    col = g.colind.numpy().astype(np.int64)
    a, ft, go = _np64(att), _np64(feat), _np64(gout)
    fwd_terms = a[:, :, None] * ft[col]                      # [E, H, F]
    want, scale = np.zeros((g.num_nodes, h, f)), np.zeros((g.num_nodes, h, f))
    np.add.at(want, row, fwd_terms)
    np.add.at(scale, row, np.abs(fwd_terms))
    bwd_terms = a[:, :, None] * go[row]
    gfeat, gfeat_scale = np.zeros((g.n_cols, h, f)), np.zeros((g.n_cols, h, f))
    np.add.at(gfeat, col, bwd_terms)
    np.add.at(gfeat_scale, col, np.abs(bwd_terms))
    dots = go[row] * ft[col]
    ref = dict(want=want, scale=scale, gfeat=gfeat, gfeat_scale=gfeat_scale, gatt=dots.sum(-1), gatt_scale=np.abs(dots).sum(-1),
               col_deg=np.bincount(col, minlength=g.n_cols))
    for a_ in ref.values():
        a_.setflags(write=False)
    return g, deg, att, feat, gout, ref


@pytest.mark.parametrize("kind", ["mh-random", "hubs"])
@DTYPES
@pytest.mark.parametrize("h,f", MH_SHAPES)
def test_mhspmm_forward_within_half_an_ulp(kind, dtype, h, f):
    g, deg, att, feat, _, ref = _mh_case(kind, h, f, dtype)
    got = mhspmm_raw(_d(g.rowptr), _d(g.colind), _d(att), _d(feat))
    assert got.dtype == dtype and got.shape == (g.num_nodes, h, f)
    hp.assert_close(got, ref["want"], ref["scale"], deg[:, None, None], dtype, "mhspmm %s (%d, %d)" % (kind, h, f))
    assert torch.equal(got, mhspmm_raw(_d(g.rowptr), _d(g.colind), _d(att), _d(feat)))


@pytest.mark.parametrize("kind", ["mh-random", "hubs"])
@DTYPES
@pytest.mark.parametrize("h,f", MH_SHAPES)
def test_mhspmm_backward_16bit(kind, dtype, h, f):
    """grad_feat: cogdl_hip_mhspmm_eid on the cached transpose (attention left in CSR order), a 16-bit launch; grad_att: fp32
    dot products of F terms."""
    from cogdl_amd.plan import PLANS

    PLANS.clear()
    g, deg, att0, feat0, gout, ref = _mh_case(kind, h, f, dtype)
    feat, att = _d(feat0).requires_grad_(), _d(att0).requires_grad_()
    out = csrmhspmm(_d(g.rowptr), _d(g.colind), feat, att)
    out.backward(_d(gout))
    assert feat.grad.dtype == dtype and att.grad.dtype == torch.float32
    hp.assert_close(feat.grad, ref["gfeat"], ref["gfeat_scale"], ref["col_deg"][:, None, None], dtype,
                    "grad_feat %s (%d, %d)" % (kind, h, f))
    hp.assert_within(att.grad.cpu().numpy(), ref["gatt"], (2 * f + 2) * 2.0 ** -24 * ref["gatt_scale"], "grad_att (%d, %d)" % (h, f))
    PLANS.clear()
