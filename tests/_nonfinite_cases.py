"""Case builders and float64 references for the non-finite contract of the softmax and max operators (DESIGN.md,
"Non-finite operands"), shared by test_nonfinite_cases_cpu.py and test_nonfinite_gpu.py.

Nothing here calls the library under test: the references are numpy / torch loops over rows that state the law directly.  Every
builder asserts what it claims about its own output, so a case that no longer holds its edge fails loudly."""
import functools

import numpy as np
import torch

from cogdl_amd import synth

NINF = float("-inf")
PATTERNS = ("leading", "trailing", "blocks", "half", "dead", "poison", "wide")
HEADS = (1, 2, 4, 8, 64, 3, 5, 100)
HEADS_16 = (1, 8, 64, 5, 100)
HUBS = ((3, 1023), (4, 1025), (17, 9000), (18, 2048), (40, 5))
GRAPHS = ("deg3", "deg40", "deg700", "hubs")
N_ROWS = 60


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "hubs":
        return synth.hub_csr(N_ROWS, N_ROWS, hubs=HUBS, seed=11, weighted=False)
    if name == "hub20000":  # one hub row of 20000 edges (H = 1: whole masked flat-kernel tiles at both tile sizes)
        return synth.hub_csr(N_ROWS, N_ROWS, hubs=((7, 20000),), seed=12, weighted=False)
    deg = int(name[3:])
    return synth.random_csr(N_ROWS, N_ROWS, deg, seed=deg, weighted=False)


def rows_of(rowptr):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    deg = np.diff(rowptr)
    row = np.repeat(np.arange(deg.shape[0]), deg)
    pos = np.arange(int(rowptr[-1])) - rowptr[:-1][row]
    return deg, row, pos


# ------------------------------------------------------------------------------------------------ float64 references
def softmax_rows(rowptr, v):
    """Per (row, head): exp(v - max) / sum in float64, row by row.  A run of nothing but -inf, or with a +inf or a NaN in it,
    comes out NaN by the arithmetic alone (-inf - -inf, inf - inf, max with a NaN), as torch.softmax gives it."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    v = np.asarray(v, dtype=np.float64)
    out = np.empty_like(v)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rowptr.shape[0] - 1):
            lo, hi = rowptr[r], rowptr[r + 1]
            if hi == lo:
                continue
            x = v[lo:hi]
            e = np.exp(x - np.max(x, axis=0, keepdims=True))  # (np.max hands a NaN on)
            out[lo:hi] = e / e.sum(axis=0, keepdims=True)
    return out


def softmax_grad_rows(rowptr, s, g):
    """s * (g - sum_row s * g) and the sum of its absolute terms s * (|g| + sum_row |s * g|), float64, row by row."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    s, g = np.asarray(s, dtype=np.float64), np.asarray(g, dtype=np.float64)
    want, scale = np.empty_like(s), np.empty_like(s)
    with np.errstate(invalid="ignore"):
        for r in range(rowptr.shape[0] - 1):
            lo, hi = rowptr[r], rowptr[r + 1]
            sg = s[lo:hi] * g[lo:hi]
            want[lo:hi] = s[lo:hi] * (g[lo:hi] - sg.sum(axis=0, keepdims=True))
            scale[lo:hi] = np.abs(s[lo:hi]) * (np.abs(g[lo:hi]) + np.abs(sg).sum(axis=0, keepdims=True))
    return want, scale


def live_spread(rowptr, v, want):
    """[m, H]: max |v - max_row| over the entries of a run whose result is not zero (what the exponential's relative error
    |x| 2^-24 scales with: tests/_halfprec.py softmax_terms); 0 for empty, dead and NaN runs."""
    deg, row, _ = rows_of(rowptr)
    v = np.asarray(v, dtype=np.float64)
    m, h = deg.shape[0], v.shape[1]
    mx = np.full((m, h), -np.inf)
    with np.errstate(invalid="ignore"):
        np.fmax.at(mx, row, v)
        d = np.abs(v - mx[row])
        d[~(want > 0)] = 0.0
    spread = np.zeros((m, h))
    np.fmax.at(spread, row, d)
    return spread


# --------------------------------------------------------------------------------------------------- mask patterns
def _pick_rows(deg):
    """(largest, second largest, smallest non-empty) row by degree, ties by row id."""
    order = sorted((r for r in range(len(deg)) if deg[r] > 0), key=lambda r: (-deg[r], r))
    assert len(order) >= 3
    return order[0], order[1], order[-1]


def _poison_rows(deg):
    """Two non-empty rows with a non-empty neighbour on both sides, at least three rows apart."""
    ok = [r for r in range(1, len(deg) - 1) if deg[r - 1] > 0 and deg[r] > 0 and deg[r + 1] > 0]
    a = max(ok, key=lambda r: (deg[r], -r))
    far = [r for r in ok if abs(r - a) >= 3]
    assert far
    return a, far[-1] if far[-1] != a else far[0]


def mask_of(name, rowptr, h, seed=0):
    """bool [E, H], True = masked.  The pattern is shifted by a different offset for every head."""
    deg, row, pos = rows_of(rowptr)
    e = pos.shape[0]
    d = deg[row][:, None]
    hd = np.arange(h)[None, :]
    if name in ("leading", "trailing"):
        q = (pos[:, None] + hd) % np.maximum(d, 1)
        mask = q < d - 3 if name == "leading" else q >= 3
        live = np.zeros((deg.shape[0], h), dtype=np.int64)
        np.add.at(live, row, ~mask)
        assert np.array_equal(live, np.broadcast_to(np.minimum(deg, 3)[:, None], live.shape))
    elif name == "blocks":
        mask = (np.arange(e)[:, None] + 150 + 37 * hd) % 307 < 300  # (runs over the flat edge array, whatever the rows)
        assert mask.any() and (~mask).any()
    elif name == "half":
        mask = torch.rand(e, h, generator=torch.Generator().manual_seed(100 + seed)).numpy() < 0.5
        assert 0.4 < mask.mean() < 0.6
    elif name == "dead":
        a, b, c = _pick_rows(deg)
        mask = np.zeros((e, h), dtype=bool)
        mask[row == a] = True                 # every head
        mask[row == b, h - 1] = True          # a single head
        mask[np.ix_(row == c, np.arange(h) % 2 == 0)] = True  # every other head
    else:
        raise ValueError(name)
    return mask


@functools.lru_cache(maxsize=None)
def softmax_case(gname, pattern, h, dtype=torch.float32):
    """-> dict(rowptr, v [E, H] of dtype, g, mask, want, want_nan, spread): one edge_softmax case and its float64 reference on
    the values AS STORED.  f32 masks are -inf; 16-bit masks are written the way users write them, masked_fill(-1e9) and then
    the cast, which is -inf in f16 and a finite -1e9 in bf16."""
    gr = graph(gname)
    rowptr = gr.rowptr.numpy().astype(np.int64)
    deg, row, pos = rows_of(rowptr)
    e = int(rowptr[-1])
    gen = torch.Generator().manual_seed(7 * h + len(pattern))
    v = 3.0 * torch.randn(e, h, generator=gen)
    g = torch.randn(e, h, generator=gen).to(dtype)
    mask = np.zeros((e, h), dtype=bool)
    if pattern == "poison":
        a, b = _poison_rows(deg)
        v = v.to(dtype)
        v[int(rowptr[a]) + int(deg[a]) // 2, h // 2] = float("inf")
        v[int(rowptr[b]), h - 1] = float("nan")
        where = {"inf": (a, h // 2), "nan": (b, h - 1)}
    elif pattern == "wide":
        assert dtype == torch.float32
        a = _pick_rows(deg)[0]
        sign = torch.where(torch.rand(int(deg[a]), h, generator=gen) < 0.5, -1.0, 1.0)
        sign[0], sign[-1] = 1.0, -1.0
        v[int(rowptr[a]):int(rowptr[a + 1])] = 3e38 * sign
        where = {"row": a}
    else:
        mask = mask_of(pattern, rowptr, h, seed=h)
        tm = torch.from_numpy(mask)
        v = v.masked_fill(tm, NINF) if dtype == torch.float32 else v.masked_fill(tm, -1e9).to(dtype)
        where = {}
    want = softmax_rows(rowptr, v.double().numpy())
    want_nan = np.isnan(want)
    run_nan = np.zeros((deg.shape[0], h), dtype=bool)
    np.logical_or.at(run_nan, row, want_nan)
    # ---- what the case claims about itself
    if pattern == "poison":
        (ra, ha), (rb, hb) = where["inf"], where["nan"]
        expect = np.zeros_like(run_nan)
        expect[ra, ha] = expect[rb, hb] = True
        assert np.array_equal(run_nan, expect) and np.isnan(want).any()
        assert not run_nan[[ra - 1, ra + 1, rb - 1, rb + 1]].any()
    elif pattern == "wide":
        assert not want_nan.any()
        x = v[int(rowptr[where["row"]]):int(rowptr[where["row"] + 1])].numpy()
        with np.errstate(over="ignore"):
            assert np.isfinite(x).all() and np.isinf(x.max() - x.min())  # the difference overflows float32
    elif pattern == "dead":
        a, b, c = _pick_rows(deg)
        if dtype == torch.bfloat16:
            assert not want_nan.any()  # -1e9 is a number in bf16: a run of equal logits
        else:
            assert run_nan[a].all() and run_nan[b, h - 1] and run_nan[c, 0]
            assert int(run_nan.sum()) == h + 1 + (h + 1) // 2 and np.isnan(want).any()
    if pattern in ("leading", "trailing", "blocks", "half", "dead"):
        stored = v.float().numpy()
        if dtype == torch.bfloat16:
            assert np.isfinite(stored[mask]).all() and (stored[mask] < -9.9e8).all()
        else:
            assert np.isneginf(stored[mask]).all() and mask.any()
    has_live = np.zeros((deg.shape[0], h), dtype=bool)
    np.logical_or.at(has_live, row, ~mask)
    zero = mask & ~run_nan[row] & has_live[row]  # masked, in a run that has a live logit: exactly 0
    assert np.all(want[zero] == 0.0)
    spread = live_spread(rowptr, v.double().numpy(), want)
    for a_ in (want, mask, want_nan, spread):
        a_.setflags(write=False)
    return dict(rowptr=gr.rowptr, rowptr64=rowptr, v=v, g=g, mask=mask, want=want, want_nan=want_nan, run_nan=run_nan,
                zero=zero, spread=spread, row=row, deg=deg)


@functools.lru_cache(maxsize=None)
def hub_tile_case():
    """H = 1, one row of 20000 edges whose first 16384 are masked: whole flat-kernel tiles (8192 and 2048 edges) of -inf."""
    gr = graph("hub20000")
    rowptr = gr.rowptr.numpy().astype(np.int64)
    deg, row, pos = rows_of(rowptr)
    assert deg[7] == 20000
    e = int(rowptr[-1])
    gen = torch.Generator().manual_seed(5)
    v = 3.0 * torch.randn(e, 1, generator=gen)
    g = torch.randn(e, 1, generator=gen)
    mask = ((row == 7) & (pos < 16384))[:, None]
    v = v.masked_fill(torch.from_numpy(mask), NINF)
    lo = int(rowptr[7])
    for tile in (8192, 2048):  # at least one whole tile of the row is masked at either tile size
        first = -(-lo // tile) * tile
        assert first + tile <= lo + 16384
    want = softmax_rows(rowptr, v.double().numpy())
    assert not np.isnan(want).any() and np.all(want[mask] == 0.0)
    return dict(rowptr=gr.rowptr, rowptr64=rowptr, v=v, g=g, mask=mask, want=want, want_nan=np.isnan(want),
                run_nan=np.zeros((N_ROWS, 1), dtype=bool), zero=mask, spread=live_spread(rowptr, v.double().numpy(), want),
                row=row, deg=deg)


# ------------------------------------------------------------------------------------------------------- fused GAT
def gat_reference(rowptr, colind, a_row, a_col, feat, gout, slope=0.2):
    """float64 composition leaky-ReLU -> per-row torch-free softmax -> weighted sum, and its autograd gradients.
    -> out [N, H, F], (grad attn_row, grad attn_col, grad feat), att [E, H] (numpy)."""
    dd = torch.float64
    rowptr64 = np.asarray(rowptr, dtype=np.int64)
    n = rowptr64.shape[0] - 1
    deg, row, _ = rows_of(rowptr64)
    row_t, col_t = torch.from_numpy(row), torch.as_tensor(np.asarray(colind), dtype=torch.long)
    ar, ac, ft = (t.detach().to(dd).clone().requires_grad_() for t in (a_row, a_col, feat))
    s = torch.nn.functional.leaky_relu(ar[row_t] + ac[col_t], slope)
    parts = []
    for r in range(n):
        lo, hi = int(rowptr64[r]), int(rowptr64[r + 1])
        if hi > lo:
            x = s[lo:hi]
            e = torch.exp(x - x.max(dim=0, keepdim=True).values)
            parts.append(e / e.sum(dim=0, keepdim=True))
    att = torch.cat(parts) if parts else s
    out = torch.zeros(n, feat.shape[1], feat.shape[2], dtype=dd).index_add_(0, row_t, att.unsqueeze(-1) * ft[col_t])
    out.backward(gout.to(dd))
    return out.detach().numpy(), (ar.grad.numpy(), ac.grad.numpy(), ft.grad.numpy()), att.detach().numpy()


@functools.lru_cache(maxsize=None)
def gat_case(gname, h, f, kind):
    """kind "masked": attn_col[u] = -inf for a third of the source nodes, chosen so that some rows see a masked first edge,
    some a masked first chunk (8 edges and more), some only masked neighbours and some none; kind "poison": a +inf and a NaN
    in attn_row."""
    gr = graph(gname)
    rowptr = gr.rowptr.numpy().astype(np.int64)
    colind = gr.colind.numpy().astype(np.int64).copy()
    deg, row, pos = rows_of(rowptr)
    n = deg.shape[0]
    gen = torch.Generator().manual_seed(h * 100 + f)
    a_row, a_col = torch.randn(n, h, generator=gen), torch.randn(n, h, generator=gen)
    feat, gout = torch.randn(n, h, f, generator=gen), torch.randn(n, h, f, generator=gen)
    if kind == "masked":
        masked_src = np.arange(n) % 3 == 0
        # the structure is the test's own: point chosen rows at masked / live sources so that every situation occurs
        nonempty = [r for r in range(n) if deg[r] > 0]
        big = [r for r in nonempty if deg[r] >= 24]
        chunk = big[0]
        only, first = [r for r in nonempty if r != chunk and deg[r] >= 2][:2]
        colind[rowptr[only]:rowptr[only + 1]] = 3 * (np.arange(deg[only]) % (n // 3))          # nothing but masked sources
        k = min(int(deg[chunk]) - 1, 64)
        assert k >= 8
        colind[rowptr[chunk]:rowptr[chunk] + k] = 0                                              # a masked first chunk
        colind[rowptr[chunk] + k] = 1
        colind[rowptr[first]] = 3                                                                # a masked first edge
        if deg[first] > 1:
            colind[rowptr[first] + 1] = 4
        a_col[torch.from_numpy(masked_src)] = NINF
        edge_masked = masked_src[colind]
        seen = np.zeros(n, dtype=np.int64)
        np.add.at(seen, row, edge_masked)
        assert (seen[nonempty] == 0).any() and seen[only] == deg[only] and edge_masked[rowptr[first]]
        assert edge_masked[rowptr[chunk]:rowptr[chunk] + k].all() and not edge_masked[rowptr[chunk] + k]
    else:
        a, b = _poison_rows(deg)
        a_row[a, h // 2] = float("inf")
        a_row[b, h - 1] = float("nan")
    ci = torch.from_numpy(colind.astype(np.int32))
    out, grads, att = gat_reference(rowptr, colind, a_row, a_col, feat, gout)
    assert np.isnan(out).any()
    if kind == "masked":
        assert np.isnan(out[only]).all() and not np.isnan(out[[r for r in range(n) if r != only and seen[r] < deg[r]]]).any()
        assert np.all(att[edge_masked & ~np.isnan(att).any(axis=1)] == 0.0)
    else:
        expect = np.zeros((n, h), dtype=bool)
        expect[a, h // 2] = expect[b, h - 1] = True
        assert np.array_equal(np.isnan(out).any(axis=2), expect)
    return dict(rowptr=gr.rowptr, colind=ci, a_row=a_row, a_col=a_col, feat=feat, gout=gout, out=out, grads=grads)


# ----------------------------------------------------------------------------------------------------- scatter_max
def scatter_max_law(rowptr, colind, x):
    """out = the maximum over the row's non-NaN values, max_id = the colind of its first occurrence in CSR order; a column
    whose values in the row are all NaN gives NaN with the first edge's colind; an empty row gives 0 / -1."""
    rowptr, colind = np.asarray(rowptr, dtype=np.int64), np.asarray(colind, dtype=np.int64)
    x = np.asarray(x, dtype=np.float32)
    m, k = rowptr.shape[0] - 1, x.shape[1]
    out, idx = np.zeros((m, k), dtype=np.float32), np.full((m, k), -1, dtype=np.int32)
    for r in range(m):
        lo, hi = rowptr[r], rowptr[r + 1]
        if hi == lo:
            continue
        vals = x[colind[lo:hi]]  # [deg, k]
        for c in range(k):
            col = vals[:, c]
            num = ~np.isnan(col)
            if not num.any():
                out[r, c], idx[r, c] = np.nan, colind[lo]
            else:
                best = col[num].max()
                first = int(np.nonzero(num & (col == best))[0][0])
                out[r, c], idx[r, c] = best, colind[lo + first]
    return out, idx


def scatter_max_grad_law(grad, idx, n_src):
    """grad_src[idx[r, c], c] += grad[r, c] in float64, rows in increasing order."""
    grad = np.asarray(grad, dtype=np.float64)
    out = np.zeros((n_src, grad.shape[1]))
    for r in range(grad.shape[0]):
        for c in range(grad.shape[1]):
            if idx[r, c] >= 0:
                out[idx[r, c], c] += grad[r, c]
    return out


def scatter_max_case(k, thresh, hubs=True):
    """One structure per kind: every edge of the planted rows points at its OWN source row (colind = a permutation inside the
    row), so that a value can be planted per edge.  -> (rowptr, colind int32 tensors, x [n_src, k], want, want_id, n_src)"""
    gen = torch.Generator().manual_seed(k + (1 if hubs else 0))
    if hubs:
        deg = torch.randint(0, 9, (N_ROWS,), generator=gen)
        deg[5], deg[6], deg[30] = 3 * thresh + 17, thresh + 1, 2 * thresh
    else:
        deg = torch.randint(0, 13, (N_ROWS,), generator=gen)
        deg[5], deg[6], deg[30] = 9, 1, 12
    deg[0], deg[1], deg[2] = 0, 4, 5
    deg[10:13] = 4
    rowptr = torch.zeros(N_ROWS + 1, dtype=torch.long)
    torch.cumsum(deg, 0, out=rowptr[1:])
    e = int(rowptr[-1])
    colind = torch.arange(e)  # edge i reads source row i: every edge has a value of its own
    x = torch.randn(e, k, generator=gen)
    rp = rowptr.numpy()
    planted = {}

    def plant(name, row, edge, value, cols=slice(None)):
        assert rp[row] <= edge < rp[row + 1], name
        x[edge, cols] = value
        planted[name] = (row, edge)

    nan, inf = float("nan"), float("inf")
    plant("short first", 1, rp[1], nan)
    plant("short last", 2, rp[3] - 1, nan)
    if hubs:
        lo, hi = int(rp[5]), int(rp[6])
        assert hi - lo > thresh and deg[6] > thresh and deg[30] > thresh
        plant("hub first", 5, lo, nan)
        border = (lo // thresh + 2) * thresh  # a chunk border (a global edge index) inside row 5, not its first one
        assert lo < border - thresh and border + 5 < hi
        plant("chunk first", 5, border, nan)
        plant("chunk true max", 5, border + 3, 50.0, slice(0, max(1, k // 2)))  # that chunk holds the row's maximum
        plant("before border", 5, border - 1, nan)
        x[int(rp[6]):int(rp[7]), k - 1] = nan  # a long row whose last column is all NaN
        planted["all nan long"] = (6, int(rp[6]))
        x[int(rp[30]):int(rp[31]):3] = nan    # every third edge of a long row, whatever the chunk and slice borders
        x[int(rp[30]) + thresh - 1, 0] = inf  # a tie between two +inf, either side of a chunk border
        x[int(rp[30]) + thresh + 1, 0] = inf
    x[int(rp[1]):int(rp[2]), 0] = nan  # a short row whose first column is all NaN
    planted["all nan short"] = (1, int(rp[1]))
    short = [10, 11, 12]
    x[int(rp[short[0]]) + 1, :] = inf
    x[int(rp[short[0]]) + 2, :] = inf          # a tie between two +inf: the first wins
    x[int(rp[short[1]]):int(rp[short[1] + 1]), :] = -inf  # nothing above -inf: -inf with the first edge
    x[int(rp[short[2]]), :] = -inf
    want, want_id = scatter_max_law(rp, colind.numpy(), x.numpy())
    assert np.isnan(want).any() and np.isinf(want).any() and (want == -np.inf).any()
    assert np.isnan(want[1, 0]) and want_id[1, 0] == rp[1]
    assert want_id[short[0], 0] == rp[short[0]] + 1
    if hubs:
        assert np.all(want[5, :max(1, k // 2)] == 50.0) and np.isnan(want[6, k - 1]) and want_id[6, k - 1] == rp[6]
        assert want[30, 0] == np.inf and want_id[30, 0] == rp[30] + thresh - 1
        assert not np.isnan(want[30]).any() and not np.isnan(want[5]).any()
    return rowptr.int(), colind.int(), x, want, want_id, e


# --------------------------------------------------------------------------------------------------------- readout
PLANTED = (("nan", float("nan")), ("+inf", float("inf")), ("-inf", NINF), ("-0", -0.0), ("+0", 0.0))


def segment_max_law(x, ptr):
    """readout_law.h, "Max": best = -inf, arg = lo; for the rows in increasing order: x > best takes the row.  An empty
    segment gives 0 and arg = -1."""
    x, ptr = np.asarray(x, dtype=np.float32), np.asarray(ptr, dtype=np.int64)
    n, f = x.shape
    b = ptr.shape[0] - 1
    out, arg = np.zeros((b, f), dtype=np.float32), np.full((b, f), -1, dtype=np.int32)
    for g in range(b):
        lo = min(max(ptr[g], 0), n)
        hi = min(max(ptr[g + 1], lo), n)
        if hi == lo:
            continue
        best, at = np.full(f, -np.inf, dtype=np.float32), np.full(f, lo, dtype=np.int32)
        for i in range(lo, hi):
            with np.errstate(invalid="ignore"):
                take = x[i] > best
            best[take] = x[i][take]
            at[take] = i
        out[g], arg[g] = best, at
    return out, arg


def sort_word(key, pos):
    """readout_law.h, "Sort-pool": the key mapped to an unsigned integer that DEcreases as the key grows (-0.0f counts as
    +0.0f, every NaN as the largest key) in the high half, the row's position inside the graph in the low half."""
    key = np.float32(key)
    if np.isnan(key):
        u = 0xFFFFFFFF
    else:
        if key == 0:
            key = np.float32(0.0)
        u = int(np.array([key], dtype=np.float32).view(np.uint32)[0])
        u = (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)
    return ((~u & 0xFFFFFFFF) << 32) | int(pos)


def sort_pool_law(x, ptr, k, key_col):
    """Both sides keep the min(k, n) smallest words; out rows past n are zero and idx is -1 there."""
    x, ptr = np.asarray(x, dtype=np.float32), np.asarray(ptr, dtype=np.int64)
    b = ptr.shape[0] - 1
    out, idx = np.zeros((b, k, x.shape[1]), dtype=np.float32), np.full((b, k), -1, dtype=np.int32)
    for g in range(b):
        lo, hi = ptr[g], ptr[g + 1]
        words = sorted(sort_word(x[lo + t, key_col], t) for t in range(hi - lo))[:k]
        for j, w in enumerate(words):
            idx[g, j] = lo + (w & 0xFFFFFFFF)
            out[g, j] = x[idx[g, j]]
    return out, idx


@functools.lru_cache(maxsize=None)
def readout_case(lengths, f=5):
    """Segments of the given lengths (0 = the ptr-gap empty segment).  Column c of every segment of three rows and more gets
    PLANTED[c] at its first row (segments 0 mod 3), its last row (1 mod 3) or its middle (2 mod 3); every fourth such segment
    has column 0 all NaN, every fourth (offset 2) column 1 all -inf.  -> (x [N, f], ptr int32)"""
    assert f >= len(PLANTED)
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n = int(ptr[-1])
    x = torch.randn(n, f, generator=torch.Generator().manual_seed(n)).numpy()
    x[np.abs(x) < 0.3] = 0.25  # (keeps the planted zeros the only zeros)
    seen = 0
    for g, ln in enumerate(lengths):
        if ln < 3:
            continue
        lo = int(ptr[g])
        at = (lo, lo + ln - 1, lo + ln // 2)[seen % 3]
        for c, (_, val) in enumerate(PLANTED):
            x[at, c] = val
        if seen % 4 == 1:
            x[lo:lo + ln, 0] = np.nan
        if seen % 4 == 3:
            x[lo:lo + ln, 1] = -np.inf
        if seen % 4 == 2:  # signed zeros against each other: ties go to the smallest row, -0.0f == +0.0f
            x[lo:lo + ln, 3] = -np.abs(x[lo:lo + ln, 3]) - 1.0
            x[lo, 3], x[lo + 1, 3] = -0.0, 0.0
        seen += 1
    assert seen >= 8 and np.isnan(x).any() and np.isinf(x).any() and (np.signbit(x) & (x == 0)).any()
    x.setflags(write=False)
    return x, ptr.astype(np.int32)
