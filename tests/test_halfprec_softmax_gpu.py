"""csr_edge_softmax in f16 / bf16 -- the flat kernel (csrc/edge_softmax_flat.hip), the row kernel and the hub-row path
(csrc/edge_softmax.hip), forward and backward -- held to "fp32 arithmetic, rounded once, to nearest, on store" (include/cogdl_hip.h).

Reference: the float64 row softmax of the ROUNDED inputs (hp.row_softmax).  The backward reference is computed from the 16-bit forward
output the kernel actually saved, so the two passes are judged separately.
    forward    hp.bound(want, want, terms_f, dtype)        terms_f = deg + ceil(A) + 16 per (row, head), A = max |v - max_row|
    backward   hp.bound(want_g, scale_g, deg + 16, dtype)  want_g = s (g - sum s g), scale_g = s (|g| + sum |s g|)
i.e. half an ulp of the output plus the fp32 slack (2 terms + 2) 2^-24 x scale of tests/_halfprec.py.  tests/test_halfprec_bound_cpu.py
pins that a truncating store, or an exp(v - max) parked in 16 bits before the division, is outside these bounds for a large share
of the elements while the 2^-7 / 2^-10 relative tolerances of tests/test_ops_gpu.py see neither.

Where the terms come from (units of 2^-24 relative to the result; checked against es_exp and the reductions of both files):
  * es_exp = __expf: the hardware exponential, one ulp (<= 2 units) plus |x| units from the scaling of the argument
    (edge_softmax.hip:24-26).  Numerator exp(v - max): <= 2 + A.  The denominator is a sum of such terms with positive weights: the
    same 2 + A once more, not per term.
  * Row sum.  No path adds more than deg values one after the other -- lanes walk strided elements (maxsum_strided, wg_piece_lds,
    row_in_lds), butterflies and the merges of wave partials and of piece records are logarithmic or short -- and the online
    (max, sum) of maxsum_strided / wg_piece_global pays per batch of 4 (8) elements at most 5 (9) additions plus one rescale (an
    exponential, <= 2 units, and a multiplication): <= 2 per element, which is the 2 x terms of hp.slack with terms = deg.  The
    ARGUMENTS of all rescale factors a partial sum meets (running maximum -> row maximum, in steps) add up to at most A: A more units.
    The flat forward's register path (KEEP_P) scales p = exp(v - max_piece) by exp(max_piece - max_row) / sum_row: the same A,
    one more exponential and one more multiplication.
  * The division 1 / sum, the multiplication by it, the difference v - max (exact for 16-bit inputs unless the exponents are far
    apart), the merge of piece records (combine / ms_combine: one more rescale per level): covered by the constant 16, i.e. 32 units.
  * Backward: <s, g> is deg fused multiply-adds (products of two 16-bit numbers are exact in fp32) in any grouping, then one
    subtraction and one multiplication: terms = deg, margin 16.
  * Nothing between the statistics and the store is rounded to 16 bits: the flat kernel stages RAW values in LDS in their own
    type (exact) and lds_st writes only FINAL values (row_in_lds), which the store step copies; pieces of rows that cross a tile
    keep their raw values until the row totals are known.
Inputs keep A <= 40 (asserted on the reference): no fp32 intermediate is then subnormal -- bf16 shares fp32's exponent range, so a
flushed fp32 denormal would show as a false failure.

What runs (16-bit tiles: 16384 elements forward, 8192 backward; "small problems" -- every graph here -- a quarter of that; tuning key
9 bit 6 = the full-size tiles, bit 8 = the forward's two-kernel form):
    flat kernel   H = 1, 2, 8, 64 x three tile settings on a graph of 300 rows of 0 .. 400 edges (a tenth of them empty, a run of
                  40 empty rows): at H = 64 a tile is 64 / 256 edges forward and 32 / 128 backward, at H = 8 512 / 256 in the
                  small-problem tiles, so rows cross tile borders as head and tail pieces, as halo rows (at most a quarter of a
                  tile: recomputed from global memory by both tiles) and as one-row tiles (register path); every row has
                  2 terms_f + 2 <= 1024 = a quarter of f16's half ulp, so a wrong store rounding cannot hide;
                  the FLAT_HUBS structures of tests/test_ops_gpu.py (rows of thousands of edges over dozens of tiles; the bound is
                  honest but, by construction, loose on the hub rows themselves);
                  the recompute-from-global escape (tuning key 8 = -1: every cross-tile wait gives up at once) on rows of 300 ..
                  3000 edges, H = 8 and 64.
    row kernels   H = 3, 5, 100, 256 (the flat kernel does not cover them) and H = 8 with the flat kernel switched off (tuning key 7
                  = 4, 5, 7), on the same graph and on the hub graph of test_edge_softmax_16bit_row_kernels_native: the generic
                  kernel and edge_softmax_long_apply_kernel for the value type.
    f16 range     one row of 20,000 edges, H = 1: outputs around 5e-5 and below, i.e. f16 SUBNORMALS, under the unchanged bound
                  (hp.ulp is the subnormal spacing there).
Not reached in 16 bits: rows beyond K_max = 512 tiles (the init kernel's records; fp32 only, test_ops_gpu.py), H = 4, 16, 32 of the
flat kernel (same code, other lane counts), the half-size 16-bit tiles of tuning key 9 bit 2."""
import functools

import numpy as np
import pytest
import torch

import _halfprec as hp
from cogdl_amd import _lib, synth
from cogdl_amd.operators import edge_softmax as es_mod
from cogdl_amd.operators.edge_softmax import csr_edge_softmax

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
FLAT_HUBS = {"mixed": ((3, 1023), (4, 1025), (17, 9000), (18, 2048), (40, 5)), "one-huge-first-row": ((0, 20000),),
             "hubs-at-the-end": ((58, 3000), (59, 4100))}  # (tests/test_ops_gpu.py: FLAT_HUBS)
NATIVE_HUBS = ((3, 129), (4, 1000), (17, 5000), (18, 257))


@pytest.fixture(params=[4, 5, 7], ids=["row-kernels-vec4-auto", "row-kernels-scalar-rows", "row-kernels-scalar-everywhere"])
def es_lanes(request):
    """Tuning key 7 (tests/test_ops_gpu.py: es_lanes), its non-zero settings: bit 2 forces the row kernels, bit 0 their 4-byte row
    lanes, bit 1 their 4-byte hub-row path (the 16-bit row kernels are 2-byte lanes throughout: all three have to agree)."""
    _lib.hip().cogdl_hip_set_tuning(7, request.param)
    yield request.param
    _lib.hip().cogdl_hip_set_tuning(7, 0)


@pytest.fixture(params=[0, 64, 64 | 256], ids=["small-problem-tiles", "full-size-tiles", "full-size-tiles-split-forward"])
def es_tiles(request):
    """Tuning key 9 (tests/test_ops_gpu.py: es_tiles): quarter-size tiles (what graphs of test size get), bit 6 the full-size tiles
    of true-size graphs, bit 8 the forward's two-kernel form."""
    _lib.hip().cogdl_hip_set_tuning(9, request.param)
    yield request.param
    _lib.hip().cogdl_hip_set_tuning(9, 0)


@functools.lru_cache(maxsize=None)
def _rowptr(gkey):
    if gkey == "medium":  # 300 rows of 0 .. 400 edges, a tenth of them empty, a run of 40 empty rows
        rng = np.random.default_rng(300)
        deg = rng.integers(0, 401, size=300)
        deg[rng.random(300) < 0.1] = 0
        deg[120:160] = 0
        deg[0], deg[299] = 400, 399  # (a long first and last row)
    elif gkey == "escape":  # rows of a few hundred to 3000 edges: several tiles each, far below K_max tiles
        deg = synth.hub_csr(40, 40, hubs=((2, 3000), (3, 1500), (20, 700), (39, 300)), seed=1).degrees().numpy()
    elif gkey == "one-row":
        deg = np.array([20000])
    elif gkey == "native-hubs":
        deg = synth.hub_csr(60, 60, hubs=NATIVE_HUBS, seed=3).degrees().numpy()
    else:
        name, cap = gkey
        hubs = tuple((r, min(d, cap)) for r, d in FLAT_HUBS[name])
        deg = synth.hub_csr(60, 60, hubs=hubs, seed=1).degrees().numpy()
    rowptr = np.zeros(deg.shape[0] + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    rowptr.setflags(write=False)
    return rowptr


@functools.lru_cache(maxsize=6)
def _case(gkey, h, dtype):
    """Inputs (rounded to dtype), the float64 forward reference and its limit: computed once, never modified."""
    rowptr = _rowptr(gkey)
    e = int(rowptr[-1])
    gen = torch.Generator().manual_seed(1000 + h)
    v = (3.0 * torch.randn(e, h, generator=gen)).to(dtype)
    g = torch.randn(e, h, generator=gen).to(dtype)
    want, spread = hp.row_softmax(rowptr, v.double().numpy())
    assert spread.max() <= 40.0, spread.max()
    terms_f, terms_b = hp.softmax_terms(rowptr, spread)
    limit_f = hp.bound(want, want, terms_f, dtype)
    for a in (want, limit_f, terms_b):
        a.setflags(write=False)
    return rowptr, v, g, want, limit_f, terms_b, float(terms_f.max()) if e else 0.0


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _run(rp, v, g):
    vd = v.to(DEV).requires_grad_()
    out = csr_edge_softmax(rp, vd)
    out.backward(g.to(DEV))
    return out.detach(), vd.grad


def check(gkey, h, dtype, what):
    """Forward + backward, twice: dtypes, run-to-run identical bits, both passes inside their bounds (the worst ratios are printed)."""
    rowptr, v, g, want, limit_f, terms_b, _ = _case(gkey, h, dtype)
    rp = torch.tensor(rowptr, dtype=torch.int32).to(DEV)
    out, gin = _run(rp, v, g)
    assert out.dtype == v.dtype == gin.dtype == dtype and out.shape == v.shape == gin.shape
    out2, gin2 = _run(rp, v, g)
    assert torch.equal(out, out2) and torch.equal(gin, gin2)  # fixed merge order, no atomics on data
    out64, gin64 = _np64(out), _np64(gin)
    _, _, want_g, scale_g = hp.row_softmax(rowptr, None, g.double().numpy(), s=out64)
    limit_b = hp.bound(want_g, scale_g, terms_b, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        print("%s: worst error / bound forward %.4f, backward %.4f" % (
            what, float(np.nanmax(np.abs(out64 - want) / limit_f)), float(np.nanmax(np.abs(gin64 - want_g) / limit_b))))
    hp.assert_within(out64, want, limit_f, what + " forward")
    hp.assert_within(gin64, want_g, limit_b, what + " backward")
    return out64, gin64


# ---------------------------------------------------------------------------------------------------------- flat kernel
@DTYPES
@pytest.mark.parametrize("h", [1, 2, 8, 64])
def test_flat_kernel_tile_borders_and_slots(es_tiles, dtype, h):
    """Rows of 0 .. 400 edges across tile borders, in every tile setting: the case where a wrong store rounding cannot hide."""
    rowptr, _, _, _, _, _, max_terms = _case("medium", h, dtype)
    deg = np.diff(rowptr)
    assert 2 * max_terms + 2 <= 1024  # the fp32 slack is at most 2^-14 relative: a quarter of f16's half ulp
    assert deg.max() == 400 and (deg == 0).mean() > 0.15 and (deg[120:160] == 0).all() and (deg >= 64).sum() > 150
    check("medium", h, dtype, "flat, borders, H=%d" % h)


@DTYPES
@pytest.mark.parametrize("tiles", [0, 64], ids=["small-problem-tiles", "full-size-tiles"])
@pytest.mark.parametrize("hubs", list(FLAT_HUBS))
@pytest.mark.parametrize("h", [1, 2, 8, 64])
def test_flat_kernel_hub_rows(dtype, tiles, hubs, h):
    """Rows of thousands of edges over dozens of tiles (H = 64: capped at 3000 edges, as tests/test_ops_gpu.py)."""
    _lib.hip().cogdl_hip_set_tuning(9, tiles)
    try:
        check((hubs, 3000 if h == 64 else 1 << 30), h, dtype, "flat, %s, H=%d" % (hubs, h))
    finally:
        _lib.hip().cogdl_hip_set_tuning(9, 0)


@DTYPES
@pytest.mark.parametrize("h", [8, 64])
def test_flat_kernel_recompute_from_global_escape(dtype, h):
    """Tuning key 8 = -1: every cross-tile wait gives up at once and the workgroup recomputes the row statistics from global memory
    (wg_piece_global for the value type: the online (max, sum) in batches of 8) -- tested in fp32 only before."""
    _lib.hip().cogdl_hip_set_tuning(8, -1)
    try:
        check("escape", h, dtype, "flat, escape, H=%d" % h)
        torch.cuda.synchronize()
        escapes = int(es_mod.LAST_WORKSPACE[:4].view(torch.int32)[0])  # (of the backward launch, the last one)
        assert escapes > 0, escapes
    finally:
        _lib.hip().cogdl_hip_set_tuning(8, 0)


# ---------------------------------------------------------------------------------------------------------- row kernels
@DTYPES
@pytest.mark.parametrize("gkey", ["medium", "native-hubs"])
@pytest.mark.parametrize("h", [3, 5, 100, 256])
def test_row_kernels_widths_the_flat_kernel_does_not_cover(dtype, gkey, h):
    check(gkey, h, dtype, "row kernels, %s, H=%d" % (gkey, h))


@DTYPES
@pytest.mark.parametrize("gkey", ["medium", "native-hubs"])
def test_row_kernels_with_the_flat_kernel_switched_off(es_lanes, dtype, gkey):
    check(gkey, 8, dtype, "row kernels (key 7 = %d), %s, H=8" % (es_lanes, gkey))


# ------------------------------------------------------------------------------------------------------------ f16 range
@pytest.mark.parametrize("lanes", [0, 4], ids=["flat-kernel", "row-kernels"])
def test_f16_outputs_near_and_below_the_smallest_normal_number(lanes):
    """One row of 20,000 edges, H = 1: the softmax is around 5e-5 = 2^-14 (f16's smallest normal number is 6.1e-5) and smaller,
    so most outputs are f16 subnormals, spaced 2^-24 apart.  hp.ulp gives that spacing: the bound applies unchanged -- a store
    that flushed subnormals to zero would be off by up to 6e-5 against a bound of 3e-8."""
    _lib.hip().cogdl_hip_set_tuning(7, lanes)
    try:
        out64, _ = check("one-row", 1, torch.float16, "f16 subnormal range (key 7 = %d)" % lanes)
    finally:
        _lib.hip().cogdl_hip_set_tuning(7, 0)
    sub = (out64 > 0) & (out64 < 2.0 ** -14)
    assert sub.mean() > 0.5 and (out64 == 0).mean() < 0.5, (sub.mean(), (out64 == 0).mean())
