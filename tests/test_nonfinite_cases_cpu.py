"""No GPU needed.  (1) The case builders of tests/_nonfinite_cases.py hold what they claim (they assert it themselves) and
their float64 references agree with torch.softmax / torch autograd on a padded dense copy, so the reference is not one
implementation trusted on its own.  (2) The host twin of the readout (libcogdl_host.so) against a numpy restatement of
csrc/readout_law.h with NaN, +inf, -inf, -0.0 and +0.0 planted at a segment's first row, last row and middle, a column that is
all NaN and one that is all -inf."""
import numpy as np
import pytest
import torch

import _nonfinite_cases as nf
from cogdl_amd.operators.readout import segment_pool, sort_pool


def _dense(rowptr, a, fill):
    """[m, max_deg, H] copy of the per-edge array a, padded with `fill`."""
    deg, row, pos = nf.rows_of(rowptr)
    out = np.full((deg.shape[0], max(int(deg.max()), 1), a.shape[1]), fill, dtype=np.float64)
    out[row, pos] = a
    return out


@pytest.mark.parametrize("pattern", nf.PATTERNS)
@pytest.mark.parametrize("gname", ["deg3", "deg40", "hubs"])
def test_softmax_reference_is_torch_softmax(gname, pattern):
    for h in (1, 5, 8):
        c = nf.softmax_case(gname, pattern, h)
        deg, row, pos = nf.rows_of(c["rowptr64"])
        v64 = c["v"].double().numpy()
        dense = torch.from_numpy(_dense(c["rowptr64"], v64, -np.inf)).requires_grad_()
        sm = torch.softmax(dense, dim=1)
        got = sm.detach().numpy()[row, pos]
        assert np.array_equal(np.isnan(got), c["want_nan"])
        ok = ~c["want_nan"]
        np.testing.assert_allclose(got[ok], c["want"][ok], rtol=1e-12, atol=0)
        assert np.all(got[c["zero"]] == 0.0)
        # backward: autograd of that float64 softmax == s (g - sum s g); NaN only in runs whose forward is NaN
        g64 = c["g"].double().numpy()
        sm.backward(torch.from_numpy(_dense(c["rowptr64"], g64, 0.0)))
        auto = dense.grad.numpy()[row, pos]
        want_g, _ = nf.softmax_grad_rows(c["rowptr64"], c["want"], g64)
        assert np.array_equal(np.isnan(auto), c["run_nan"][row]) and np.array_equal(np.isnan(want_g), c["run_nan"][row])
        live = ~c["run_nan"][row]
        np.testing.assert_allclose(auto[live], want_g[live], rtol=1e-9, atol=1e-15)
        assert np.all(auto[c["zero"]] == 0.0) and np.all(want_g[c["zero"]] == 0.0)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_user_style_mask_is_minus_inf_in_f16_and_a_number_in_bf16(dtype):
    for pattern in ("leading", "blocks", "dead"):
        c = nf.softmax_case("deg40", pattern, 8, dtype)
        stored = c["v"].float().numpy()[c["mask"]]
        if dtype == torch.float16:
            assert np.isneginf(stored).all()
        else:
            assert np.isfinite(stored).all() and np.all(stored == stored[0]) and stored[0] < -9.9e8
            assert not c["want_nan"].any()


def test_hub_tile_case_masks_whole_tiles():
    c = nf.hub_tile_case()
    assert int(c["mask"].sum()) == 16384 and abs(float(c["want"][c["row"] == 7].sum()) - 1.0) < 1e-12


@pytest.mark.parametrize("kind", ["masked", "poison"])
def test_gat_cases_hold_their_edges(kind):
    for gname in ("deg40", "hubs"):
        c = nf.gat_case(gname, 4, 16, kind)
        nan_rows = np.isnan(c["out"]).any(axis=(1, 2))
        assert 0 < int(nan_rows.sum()) < nf.N_ROWS
        ga_row, ga_col, g_feat = c["grads"]
        # NaN gradients of attn_row appear only in (row, head) whose forward is NaN
        assert np.array_equal(np.isnan(ga_row), np.isnan(c["out"]).any(axis=2))
        assert np.isnan(g_feat).any() and not np.isnan(g_feat).all()


def test_scatter_max_law_on_a_hand_made_row():
    nan, inf = float("nan"), float("inf")
    rowptr = np.array([0, 4, 4, 6, 9])
    colind = np.arange(9)
    x = np.array([[nan, 1.0], [2.0, nan], [2.0, 5.0], [nan, 5.0], [nan, -inf], [nan, -inf], [inf, 0.0], [inf, -0.0], [nan, 1.0]],
                 dtype=np.float32)
    out, idx = nf.scatter_max_law(rowptr, colind, x)
    assert out[0].tolist() == [2.0, 5.0] and idx[0].tolist() == [1, 2]
    assert out[1].tolist() == [0.0, 0.0] and idx[1].tolist() == [-1, -1]
    assert np.isnan(out[2, 0]) and idx[2, 0] == 4 and out[2, 1] == -inf and idx[2, 1] == 4
    assert out[3].tolist() == [inf, 1.0] and idx[3].tolist() == [6, 8]
    for k in (1, 12):
        for hubs in (False, True):
            nf.scatter_max_case(k, 128, hubs)  # (asserts its own claims)


# ------------------------------------------------------------------------------------------------ readout, host twin
LENGTHS = (3, 0, 5, 1, 7, 64, 65, 2, 129, 300, 0, 4, 9, 33)


def _argmax_of(x, ptr):
    """The argmax the operator routed its gradient to: row i of segment g got grad[g, c] = g * F + c + 1."""
    xt = torch.from_numpy(np.array(x)).requires_grad_()
    res = segment_pool(xt, torch.from_numpy(ptr), "max")
    b, f = res.shape
    grad = torch.arange(1, b * f + 1, dtype=torch.float32).view(b, f)
    res.backward(grad)
    return res.detach().numpy(), xt.grad.numpy(), grad.numpy()


def test_host_segment_max_is_the_law():
    x, ptr = nf.readout_case(LENGTHS)
    want, arg = nf.segment_max_law(x, ptr)
    got, gx, grad = _argmax_of(x, ptr)
    assert got.tobytes() == want.tobytes()  # (byte for byte: -inf where nothing is above -inf, never a NaN, the sign of a zero)
    assert not np.isnan(got).any() and np.isneginf(got).any()
    want_gx = np.zeros_like(gx)
    for g in range(want.shape[0]):
        for c in range(want.shape[1]):
            if arg[g, c] >= 0:
                want_gx[arg[g, c], c] = grad[g, c]
    assert np.array_equal(gx, want_gx)
    # the law's sentences, on the planted segments: a NaN is never taken; ties go to the smallest row; nothing above -inf -> arg = lo
    nan_col = [g for g in range(len(LENGTHS)) if LENGTHS[g] >= 3 and np.isnan(x[ptr[g]:ptr[g + 1], 0]).all()]
    assert nan_col and all(want[g, 0] == -np.inf and arg[g, 0] == ptr[g] for g in nan_col)
    inf_col = [g for g in range(len(LENGTHS)) if LENGTHS[g] >= 3 and np.isneginf(x[ptr[g]:ptr[g + 1], 1]).all()]
    assert inf_col and all(want[g, 1] == -np.inf and arg[g, 1] == ptr[g] for g in inf_col)
    zeros = [g for g in range(len(LENGTHS)) if LENGTHS[g] >= 3 and want[g, 3] == 0 and np.signbit(want[g, 3])]
    assert zeros and all(arg[g, 3] == ptr[g] for g in zeros)  # -0.0f first, +0.0f second: +0.0f > -0.0f is false


@pytest.mark.parametrize("k", [1, 4, 70])
def test_host_sort_pool_is_the_law(k):
    x, ptr = nf.readout_case(LENGTHS)
    for key_col in range(len(nf.PLANTED)):
        want, idx = nf.sort_pool_law(x, ptr, k, key_col)
        out, got_idx = sort_pool(torch.from_numpy(np.array(x)), torch.from_numpy(ptr), k, key_col)
        assert np.array_equal(got_idx.numpy(), idx), key_col
        assert out.numpy().tobytes() == want.tobytes(), key_col
    # every NaN as the largest key: a NaN key comes first; -0.0f counts as +0.0f: planted zeros keep their row order
    _, idx = nf.sort_pool_law(x, ptr, 1, 0)
    with_nan = [g for g in range(len(LENGTHS)) if np.isnan(x[ptr[g]:ptr[g + 1], 0]).any()]
    assert with_nan and all(np.isnan(x[idx[g, 0], 0]) for g in with_nan)
    assert nf.sort_word(-0.0, 3) == nf.sort_word(0.0, 3) and nf.sort_word(float("nan"), 0) < nf.sort_word(float("inf"), 0)
    assert nf.sort_word(1.0, 0) < nf.sort_word(0.5, 0) < nf.sort_word(-0.0, 0) < nf.sort_word(-1.0, 0) < nf.sort_word(float("-inf"), 0)
