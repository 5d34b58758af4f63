"""-inf, +inf and NaN operands of the softmax and max kernels on the GPU, against the float64 references of
tests/_nonfinite_cases.py ("Non-finite operands").

edge_softmax   per (row, head) torch.softmax of the run in float64 on the values as stored: a -inf logit next to a finite one
               is exactly 0, a run of nothing but -inf / with a +inf / with a NaN is NaN in exactly the entries where the float64
               result is, every other (row, head) is untouched; the backward is s (g - sum s g) on the saved output.  Every
               kernel path: the flat kernel in both tile sizes and its two-kernel form, the time-out escape, the row kernels
               with 16-byte and 4-byte lanes, the generic kernel, the hub-row path, f32 / f16 / bf16.
fused GAT      the float64 composition leaky-ReLU -> softmax -> weighted sum with the same containment, both forward kernels.
scatter_max    the maximum over the row's non-NaN values wherever the NaN stands (short rows and the chunk-parallel path).
readout        segment max and sort-pool on the device, byte for byte against the host twin and the law."""
import numpy as np
import pytest
import torch

import _halfprec as hp
import _nonfinite_cases as nf
from cogdl_amd import _lib
from cogdl_amd.operators.edge_softmax import csr_edge_softmax
from cogdl_amd.operators.mhspmm import csrmhspmm
from cogdl_amd.operators.readout import segment_pool, sort_pool
from cogdl_amd.operators.scatter_max import scatter_max, scatter_max_bp, scatter_max_bp_csc, scatter_max_fp
from cogdl_amd.plan import csr2csc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tuning(key, value):
    _lib.hip().cogdl_hip_set_tuning(key, value)


@pytest.fixture(params=[0, 4, 5, 7], ids=["flat-kernel", "row-kernels-vec4-auto", "row-kernels-scalar-rows",
                                            "row-kernels-scalar-everywhere"])
def es_lanes(request):
    """Tuning key 7 (as in tests/test_ops_gpu.py): bit 2 forces the row kernels, bit 0 their 4-byte row lanes, bit 1 their
    4-byte hub-row path."""
    _tuning(7, request.param)
    yield request.param
    _tuning(7, 0)


@pytest.fixture(params=[0, 64, 64 | 256], ids=["small-problem-tiles", "full-size-tiles", "full-size-tiles-split-forward"])
def es_tiles(request):
    """Tuning key 9: bit 6 = the flat kernel's full-size tiles on graphs of test size, bit 8 = the forward's two-kernel form."""
    _tuning(9, request.param)
    yield request.param
    _tuning(9, 0)


@pytest.fixture(params=[0, 1, 2], ids=["auto", "edgewise-softmax", "chunkwise-softmax"])
def gat_kernel(request):
    """Tuning key 5: the fused GAT forward's edge-wise online softmax (1) or chunk-wise softmax (2)."""
    _tuning(5, request.param)
    yield request.param
    _tuning(5, 0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _check_softmax(c, what):
    """One case, forward + backward + repeat, against the contract."""
    dtype = c["v"].dtype
    rp = c["rowptr"].to(DEV)
    row, deg, want = c["row"], c["deg"], c["want"]
    m, h = deg.shape[0], want.shape[1]
    vd = c["v"].to(DEV).requires_grad_()
    out = csr_edge_softmax(rp, vd)
    assert out.dtype == dtype
    got = out.detach().double().cpu().numpy()
    # ---- forward
    assert np.array_equal(np.isnan(got), c["want_nan"]), "%s: %d entries NaN, %d expected" % (
        what, int(np.isnan(got).sum()), int(c["want_nan"].sum()))
    assert np.all(got[c["zero"]] == 0.0), what + ": a masked entry of a live run is not exactly 0"
    ok = ~c["want_nan"]
    want0, got0 = np.where(ok, want, 0.0), np.where(ok, got, 0.0)
    if dtype == torch.float32:
        np.testing.assert_allclose(got0, want0, rtol=1e-5, atol=1e-9, err_msg=what)
        sum_tol = np.full((m, h), 1e-5)
    else:
        terms_f, terms_b = hp.softmax_terms(c["rowptr64"], c["spread"])
        limit_f = hp.bound(want0, want0, terms_f, dtype)
        hp.assert_within(got0, want0, limit_f, what + " forward")
        sum_tol = np.zeros((m, h))
        np.add.at(sum_tol, row, limit_f)  # (the sum of a run's stores is off by at most the sum of their bounds)
        sum_tol += 1e-12
    sums = np.zeros((m, h))
    np.add.at(sums, row, got0)
    live = (deg > 0)[:, None] & ~c["run_nan"]
    assert np.all(np.abs(sums - 1.0)[live] <= sum_tol[live]), what + ": a live run does not sum to one"
    again = csr_edge_softmax(rp, c["v"].to(DEV))
    assert torch.equal(_bits(again), _bits(out.detach())), what + ": the result does not repeat bit for bit"
    # ---- backward, judged on the output the kernel saved
    out.backward(c["g"].to(DEV))
    assert vd.grad.dtype == dtype
    gin = vd.grad.double().cpu().numpy()
    run_nan_e = c["run_nan"][row]
    assert np.array_equal(np.isnan(gin), run_nan_e), what + ": NaN gradients outside the runs whose forward is NaN (or missing)"
    assert np.all(gin[c["zero"]] == 0.0), what + ": a masked entry got a gradient"
    want_g, scale_g = nf.softmax_grad_rows(c["rowptr64"], got0, c["g"].double().numpy())
    err = np.where(run_nan_e, 0.0, np.abs(gin - want_g))
    if dtype == torch.float32:
        limit_b = 1e-5 * scale_g + 1e-12
    else:
        limit_b = hp.bound(np.where(run_nan_e, 0.0, want_g), scale_g, terms_b, dtype)
    with np.errstate(invalid="ignore"):
        bad = ~(err <= limit_b) & ~run_nan_e
    assert not bad.any(), "%s backward: %d outside the bound, worst %.3e" % (what, int(bad.sum()), float(err[bad].max()))


# ------------------------------------------------------------------------------------------------------ edge_softmax
@pytest.mark.parametrize("pattern", nf.PATTERNS)
@pytest.mark.parametrize("gname", nf.GRAPHS)
def test_edge_softmax_f32_every_pattern_and_lane_layout(gname, pattern, es_lanes):
    for h in nf.HEADS:
        _check_softmax(nf.softmax_case(gname, pattern, h), "%s %s H=%d key7=%d" % (gname, pattern, h, es_lanes))


@pytest.mark.parametrize("pattern", nf.PATTERNS)
def test_edge_softmax_f32_hub_rows_in_both_tile_sizes(pattern, es_tiles):
    for h in (1, 2, 4, 8, 64):  # (the shapes the flat kernel covers)
        _check_softmax(nf.softmax_case("hubs", pattern, h), "hubs %s H=%d key9=%d" % (pattern, h, es_tiles))


def test_edge_softmax_whole_masked_tiles(es_tiles, es_lanes):
    """A row of 20000 edges (H = 1) whose first 16384 logits are -inf: flat-kernel tiles, and pieces of the hub-row path, that
    hold nothing but -inf inside a row that is alive."""
    _check_softmax(nf.hub_tile_case(), "hub20000 key9=%d key7=%d" % (es_tiles, es_lanes))


@pytest.mark.parametrize("tiles", [0, 64], ids=["small-problem-tiles", "full-size-tiles"])
def test_edge_softmax_masked_pieces_through_the_timeout_escape(tiles):
    """Tuning key 8 = -1: every cross-tile wait gives up at once and the row statistics are recomputed from global memory."""
    _tuning(9, tiles)
    _tuning(8, -1)
    try:
        for h in (1, 8, 64):
            _check_softmax(nf.softmax_case("hubs", "blocks", h), "hubs blocks H=%d escape" % h)
        _check_softmax(nf.hub_tile_case(), "hub20000 escape")
        from cogdl_amd.operators import edge_softmax as es_mod

        torch.cuda.synchronize()
        assert int(es_mod.LAST_WORKSPACE[:4].view(torch.int32)[0]) > 0  # (the escape was taken)
    finally:
        _tuning(8, 0)
        _tuning(9, 0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("pattern", [p for p in nf.PATTERNS if p != "wide"])
@pytest.mark.parametrize("gname", nf.GRAPHS)
def test_edge_softmax_16bit_user_style_masks(gname, pattern, dtype):
    """masked_fill(mask, -1e9) then .to(dtype): -inf in f16, a finite -1e9 in bf16 (a fully masked bf16 run is a run of equal
    logits: 1 / deg, not NaN)."""
    for h in nf.HEADS_16:
        c = nf.softmax_case(gname, pattern, h, dtype)
        if pattern != "poison":
            stored = c["v"].float().numpy()[c["mask"]]
            assert stored.size and (np.isneginf(stored).all() if dtype == torch.float16 else
                                    (np.isfinite(stored).all() and (stored < -9.9e8).all()))
        _check_softmax(c, "%s %s H=%d %s" % (gname, pattern, h, dtype))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_edge_softmax_16bit_hub_rows_in_both_tile_sizes(dtype, es_tiles):
    for pattern in ("leading", "blocks", "dead", "poison"):
        for h in (1, 8):
            _check_softmax(nf.softmax_case("hubs", pattern, h, dtype), "hubs %s H=%d %s key9=%d" % (pattern, h, dtype, es_tiles))


# --------------------------------------------------------------------------------------------------------- fused GAT
def _same_nan_and_close(got, want, rtol, atol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: %d NaN, %d expected" % (what, int(np.isnan(got).sum()),
                                                                                        int(np.isnan(want).sum()))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=rtol, atol=atol, err_msg=what)


@pytest.mark.parametrize("kind", ["masked", "poison"])
@pytest.mark.parametrize("gname", ["deg40", "hubs"])
@pytest.mark.parametrize("h,f", [(8, 8), (1, 41), (4, 16)])
@pytest.mark.parametrize("pad", [True, False], ids=["padded-rows", "raw-width"])
def test_fused_gat_masked_sources_and_poisoned_rows(gat_kernel, gname, h, f, pad, kind, monkeypatch):
    from cogdl_amd.operators import fused_gat
    from cogdl_amd.operators.fused_gat import fused_gat_func

    monkeypatch.setattr(fused_gat, "PAD_FEATURES", pad)
    c = nf.gat_case(gname, h, f, kind)
    rp, ci = c["rowptr"].to(DEV), c["colind"].to(DEV)
    ar, ac, ft = (c[k].to(DEV).requires_grad_() for k in ("a_row", "a_col", "feat"))
    out = fused_gat_func(ar, ac, rp, ci, rp, ci, 0.2, ft)
    what = "%s %s H=%d F=%d" % (gname, kind, h, f)
    _same_nan_and_close(out.detach().cpu().numpy(), c["out"], 2e-5, 2e-6, what + " forward")
    out.backward(c["gout"].to(DEV))
    for got, ref, name in zip((ar.grad, ac.grad, ft.grad), c["grads"], ("attn_row", "attn_col", "feat")):
        _same_nan_and_close(got.cpu().numpy(), ref, 2e-4, 2e-5, what + " grad " + name)


@pytest.mark.parametrize("kind", ["masked", "poison"])
@pytest.mark.parametrize("gname", ["deg40", "hubs"])
def test_fused_gat_agrees_with_the_unfused_operators(gat_kernel, gname, kind):
    from cogdl_amd.operators.fused_gat import fused_gat_func

    c = nf.gat_case(gname, 8, 8, kind)
    rp, ci = c["rowptr"].to(DEV), c["colind"].to(DEV)
    ar, ac, ft = (c[k].to(DEV) for k in ("a_row", "a_col", "feat"))
    fused = fused_gat_func(ar, ac, rp, ci, rp, ci, 0.2, ft)
    row = torch.from_numpy(c_row(c)).to(DEV)
    score = torch.nn.functional.leaky_relu(ar[row] + ac[ci.long()], 0.2)
    unfused = csrmhspmm(rp, ci, ft, csr_edge_softmax(rp, score))
    assert torch.equal(torch.isnan(fused), torch.isnan(unfused))
    ok = ~torch.isnan(fused)
    assert bool(torch.isnan(fused).any()) and torch.allclose(fused[ok], unfused[ok], rtol=2e-5, atol=2e-6)


def c_row(c):
    return nf.rows_of(c["rowptr"].numpy())[1]


# ------------------------------------------------------------------------------------------------------- scatter_max
@pytest.mark.parametrize("hubs", [False, True], ids=["ragged", "hub-rows"])
@pytest.mark.parametrize("k", [1, 12, 100, 128])
def test_scatter_max_nan_never_beats_a_number(oracle, k, hubs):
    lib = _lib.hip()
    thresh = lib.cogdl_hip_long_row_threshold(2000)
    rowptr, colind, x, want, want_id, n_src = nf.scatter_max_case(k, thresh, hubs)
    nnz = int(rowptr[-1])
    assert lib.cogdl_hip_long_row_threshold(nnz) == thresh
    deg = np.diff(rowptr.numpy())
    assert (deg.max() > thresh) == hubs and (not hubs or sorted(deg)[-3] > thresh)
    rp, ci = rowptr.to(DEV), colind.to(DEV)
    out, idx = scatter_max_fp(rp, ci, x.to(DEV))
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(idx.cpu().numpy(), want_id)
    # both backward forms route the gradient to the reported max_id
    gr = torch.randn(nf.N_ROWS, k, generator=torch.Generator().manual_seed(1))
    want_g = oracle.scatter_max_bwd(gr, want_id, n_src)
    assert np.array_equal(want_g, nf.scatter_max_grad_law(gr.numpy(), want_id, n_src).astype(np.float32))
    got_g = scatter_max_bp(gr.to(DEV), idx, n_src).cpu().numpy()
    np.testing.assert_allclose(got_g, want_g, rtol=1e-5, atol=1e-5)
    plan = csr2csc(rp, ci, n_src)
    got_c = scatter_max_bp_csc(plan.colptr, plan.rowind, gr.to(DEV), idx, n_src).cpu().numpy()
    assert got_c.tobytes() == want_g.tobytes()  # (every source has one out-edge here: one term per element)
    xd = x.to(DEV).requires_grad_()
    res = scatter_max(rp, ci, xd)
    assert res.detach().cpu().numpy().tobytes() == want.tobytes()
    res.backward(gr.to(DEV))
    assert xd.grad.cpu().numpy().tobytes() == want_g.tobytes()


# ----------------------------------------------------------------------------------------------------------- readout
# every device path of csrc/readout.hip: pooling up to kExactNodes = 4096 rows (one kernel) and beyond (the four ways, chunks
# of 1024 rows); sort-pool up to kLdsNodes = 2048 rows in LDS and beyond (tiles of 2048 through the workspace); 0 = the
# ptr-gap empty segment
READOUT_LENGTHS = (3, 0, 5, 1, 7, 64, 65, 2, 129, 300, 0, 4, 9, 33, 2048, 2049, 4096, 4097, 5000, 0, 6)


def test_readout_segment_max_and_sort_pool_planted_values():
    x, ptr = nf.readout_case(READOUT_LENGTHS)
    assert max(READOUT_LENGTHS) > _lib.hip().cogdl_hip_segment_exact_nodes() > 4000
    assert max(READOUT_LENGTHS) > _lib.hip().cogdl_hip_sort_pool_lds_nodes() >= 2048
    xt, pt = torch.from_numpy(np.array(x)), torch.from_numpy(ptr)
    want, arg = nf.segment_max_law(x, ptr)
    b, f = want.shape
    grad = torch.arange(1, b * f + 1, dtype=torch.float32).view(b, f)
    res = {}
    for dev in ("cpu", DEV):
        xd = xt.detach().to(dev).requires_grad_()
        out = segment_pool(xd, pt.to(dev), "max")
        out.backward(grad.to(dev))
        res[dev] = (out.detach().cpu().numpy(), xd.grad.cpu().numpy())
    assert res[DEV][0].tobytes() == res["cpu"][0].tobytes() == want.tobytes()
    assert res[DEV][1].tobytes() == res["cpu"][1].tobytes()
    want_gx = np.zeros_like(res["cpu"][1])
    for g in range(b):
        for c in range(f):
            if arg[g, c] >= 0:
                want_gx[arg[g, c], c] = grad[g, c]
    assert np.array_equal(res[DEV][1], want_gx)
    for k in (1, 30, 2100):
        for key_col in range(len(nf.PLANTED)):
            o_h, i_h = sort_pool(xt, pt, k, key_col)
            o_d, i_d = sort_pool(xt.to(DEV), pt.to(DEV), k, key_col)
            assert torch.equal(i_d.cpu(), i_h), (k, key_col)
            assert o_d.cpu().numpy().tobytes() == o_h.numpy().tobytes(), (k, key_col)
        if k <= 30:
            want_o, want_i = nf.sort_pool_law(x, ptr, k, 0)
            o_d, i_d = sort_pool(xt.to(DEV), pt.to(DEV), k, 0)
            assert np.array_equal(i_d.cpu().numpy(), want_i) and o_d.cpu().numpy().tobytes() == want_o.tobytes()
