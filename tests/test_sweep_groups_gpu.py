"""csr_spmm over sweep layouts whose groups are ANY rows (include/cogdl_hip.h: cogdl_hip_csr_spmm_sweep_rows,
cogdl_hip_csr_spmm_sweep_rows_guarded; csrc/rowsweep.h: MAPPED; cogdl_amd/sweepplan.py: `assign=`, deal_by_degree).  Which rows
share a wave changes where the waves are in the table at the same moment, never a sum: every result must be bit-identical to
csr_spmm_raw on the same structure.  fp32, F = 128; small tables, the round capped to a few waves where a case wants rounds."""
import pytest
import torch

from cogdl_amd import _lib, plan, sweepplan, synth, xcdplan
from cogdl_amd.operators import spmm as spmm_mod
from cogdl_amd.operators.spmm import csr_spmm_raw, csr_spmm_sweep_forward_raw, csr_spmm_sweep_raw, csrspmm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 128
U64 = (1 << 64) - 1


def _rows():
    return int(_lib.hip().cogdl_hip_csr_spmm_sweep_group_rows())


def _x(n, seed=1):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _hashed(rowptr, colind, n_src):
    fp = plan.Fingerprint(rowptr, colind, n_src, dev_parts=True)
    return fp.dev, fp.key()[4] & U64


def _shuffled(n_rows, r, seed, extra_groups=0):
    """Any assignment: a random permutation of the rows cut into groups of differing sizes, pads in several groups."""
    n_groups = (n_rows + r - 1) // r + extra_groups
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(seed))
    sizes = torch.full((n_groups,), n_rows // n_groups, dtype=torch.long)
    sizes[: n_rows - int(sizes.sum())] += 1
    a = torch.full((n_groups, r), -1, dtype=torch.long)
    at = 0
    for g, s in enumerate(sizes.tolist()):
        a[g, :s] = perm[at:at + s]
        at += s
    return a


@pytest.fixture(scope="module")
def ragged():
    """3 R + 7 rows of 0-40 edges in any column order (10 % of them empty, duplicates), a table of 900 rows (n_src != m); its
    transpose; the ordinary launch's product of each, weighted and not -- computed once."""
    R = _rows()
    g = synth.random_csr(3 * R + 7, 900, 20, seed=11)
    assert int(g.degrees().min()) == 0
    rowptr, colind, w = g.rowptr.to(DEV), g.colind.to(DEV), g.weight.to(DEV)
    x, gout = _x(g.n_cols, 1), _x(g.num_nodes, 2)
    csc = plan.csr2csc(rowptr, colind, g.n_cols)
    want = {("fwd", True): csr_spmm_raw(rowptr, colind, w, x), ("fwd", False): csr_spmm_raw(rowptr, colind, None, x),
            ("bwd", True): csr_spmm_raw(csc.colptr, csc.rowind, csc.transposed_values(w), gout),
            ("bwd", False): csr_spmm_raw(csc.colptr, csc.rowind, None, gout)}
    parts, h = _hashed(rowptr, colind, g.n_cols)
    return g, rowptr, colind, w, x, gout, csc, {k: _bytes(v) for k, v in want.items()}, parts, h


def _backward(ragged, r, assign, weighted=True):
    g, rowptr, colind, w, x, gout, csc, want, _, _ = ragged
    mine = plan.CscPlan(csc.colptr, csc.rowind, csc.perm, csc.m, csc.n_cols, csc.nnz)
    mine.sweep = sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, r, assign)
    assert (mine.sweep.rows is None) == (assign is None)
    got = csr_spmm_sweep_raw(mine, w if weighted else None, gout)
    assert got.shape == (g.n_cols, F)
    assert _bytes(got) == want[("bwd", weighted)], "mapped sweep != ordinary launch on the transpose"
    return mine.sweep


def _forward(ragged, r, assign, weighted=True, match=True):
    g, rowptr, colind, w, x, gout, csc, want, parts, h = ragged
    sp = sweepplan.build_forward(rowptr, colind, g.n_cols, r, assign)
    assert (sp.rows is None) == (assign is None)
    sp.hash = h if match else h ^ 1
    got = csr_spmm_sweep_forward_raw(sp, parts, rowptr, colind, w if weighted else None, x)
    assert _bytes(got) == want[("fwd", weighted)], "guarded pair over a mapped layout != ordinary launch"
    return sp


@pytest.mark.parametrize("r", [1, 5, 33, "R"])
def test_dealt_groups_both_directions(ragged, r):
    """Groups of 1, 5, 33 (a row in LDS) and the most rows: the degree deal (its last round is partial: pad slots in some groups),
    backward and the guarded forward pair with the hash matching and mismatching."""
    r = _rows() if r == "R" else r
    back = _backward(ragged, r, sweepplan.deal_by_degree)
    fwd = _forward(ragged, r, sweepplan.deal_by_degree, match=True)
    _forward(ragged, r, sweepplan.deal_by_degree, match=False)
    pads = [int((sp.rows < 0).sum()) for sp in (back, fwd)]
    assert pads == [sp.n_groups * r - sp.n_rows for sp in (back, fwd)] and (r == 1 or max(pads) > 0)


@pytest.mark.parametrize("r", [5, "R"])
def test_any_assignment_with_pads_empty_groups_and_unweighted(ragged, r):
    """A random assignment with pads in many groups and one group that is all pads; then one whose last group holds only rows
    without edges (a group with no edges: zeros are stored); unweighted as well."""
    r = _rows() if r == "R" else r
    g, _, _, _, _, _, csc, _, _, _ = ragged
    for n_rows, ptr, run in ((csc.n_cols, csc.colptr, _backward), (g.num_nodes, g.rowptr, _forward)):
        a = _shuffled(n_rows, r, seed=r, extra_groups=2)
        assert int((a[:, -1] < 0).sum()) > 1
        a = torch.cat([a, a.new_full((1, r), -1)])  # ... and a group of pads alone
        run(ragged, r, a)
        run(ragged, r, a, weighted=False)
        deg = (ptr[1:] - ptr[:-1]).long().cpu()
        empty = torch.nonzero(deg == 0).flatten()[:r]
        assert empty.numel() > 0
        rest = torch.nonzero(deg >= 0).flatten()
        rest = rest[~torch.isin(rest, empty)]
        b = torch.cat([rest, rest.new_full(((-rest.numel()) % r,), -1), empty, empty.new_full((r - empty.numel(),), -1)]).view(-1, r)
        sp = run(ragged, r, b)
        assert int(sp.goff[-1] - sp.goff[-2]) == 0 and int(sp.rows[-r]) >= 0


def test_forward_match_runs_the_mapped_sweep(ragged):
    """Which side ran, seen from outside: a mapped layout of ANOTHER structure's edges under this structure's hash gives the other
    structure's product exactly when the sweep runs."""
    g, rowptr, colind, w, x, _, _, want, parts, h = ragged
    other = ((colind.long() + 1) % g.n_cols).int()
    y_other = _bytes(csr_spmm_raw(rowptr, other, w, x))
    assert y_other != want[("fwd", True)]
    sp = sweepplan.build_forward(rowptr, other, g.n_cols, 33, sweepplan.deal_by_degree)
    sp.hash = h
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts, rowptr, colind, w, x)) == y_other
    sp.hash = h ^ 1
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts, rowptr, colind, w, x)) == want[("fwd", True)]


def test_several_rounds():
    """3,000 rows with one round capped at 10 waves (tuning key 18): the same waves walk further groups of the map."""
    R = _rows()
    lib = _lib.hip()
    g = synth.scaled(3000, 12, seed=8)
    rowptr, colind, w = g.rowptr.to(DEV), g.colind.to(DEV), g.weight.to(DEV)
    x = _x(g.n_cols, 3)
    csc = plan.csr2csc(rowptr, colind, g.n_cols)
    want_f = _bytes(csr_spmm_raw(rowptr, colind, w, x))
    want_b = _bytes(csr_spmm_raw(csc.colptr, csc.rowind, csc.transposed_values(w), x))
    parts, h = _hashed(rowptr, colind, g.n_cols)
    lib.cogdl_hip_set_tuning(18, 10 * R)
    try:
        assert lib.cogdl_hip_csr_spmm_sweep_round_rows(F, 0) == 10 * R
        csc.sweep = sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, R, sweepplan.deal_by_degree)
        assert csc.sweep.n_groups > 6 * 10
        assert _bytes(csr_spmm_sweep_raw(csc, w, x)) == want_b
        sp = sweepplan.build_forward(rowptr, colind, g.n_cols, R, sweepplan.deal_by_degree)
        sp.hash = h
        assert _bytes(csr_spmm_sweep_forward_raw(sp, parts, rowptr, colind, w, x)) == want_f
    finally:
        lib.cogdl_hip_set_tuning(18, 0)


def test_consecutive_groups_keep_their_entry_and_their_bits(ragged):
    """rows=None: the entries that take no map, on the layout they always took -- the ordinary launch's bytes, and the same bytes
    as the mapped entry over the same groups written out as a map."""
    R = _rows()
    g, _, _, _, _, _, csc, _, _, _ = ragged
    _backward(ragged, R, None)
    _forward(ragged, R, None)
    _forward(ragged, R, None, match=False)
    n = csc.n_cols
    a = torch.full(((n + R - 1) // R * R,), -1, dtype=torch.long)
    a[:n] = torch.arange(n)
    sp = _backward(ragged, R, a)
    plain = sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, R)
    assert torch.equal(sp.src, plain.src) and torch.equal(sp.goff, plain.goff)


def test_a_bad_map_is_refused_before_anything_is_enqueued(ragged):
    g, rowptr, colind, w, x, _, csc, _, _, _ = ragged
    R = _rows()
    a = sweepplan.deal_by_degree(rowptr, R)
    bad = a.clone()
    bad[0, 0] = g.num_nodes  # one past the last row
    with pytest.raises(_lib.BackendError):
        sweepplan.build_forward(rowptr, colind, g.n_cols, R, bad)
    with pytest.raises(_lib.BackendError):
        sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, R, torch.full((csc.n_cols + R,), csc.n_cols, dtype=torch.long))
    # the entry itself: a map of another length than n_groups * r, or none at all
    sp = sweepplan.build_forward(rowptr, colind, g.n_cols, R, a)
    lib = _lib.hip()
    out = torch.full((g.num_nodes, F), 7.0, device=DEV)
    args = (_lib.ptr(sp.goff), _lib.ptr(sp.src), None, _lib.ptr(x), _lib.ptr(out), g.num_nodes, g.n_cols, sp.n_groups, sp.r, F, sp.nnz, 0)
    assert lib.cogdl_hip_csr_spmm_sweep_rows(*args, _lib.ptr(sp.rows), sp.rows.numel() - 1, None) != 0
    assert lib.cogdl_hip_csr_spmm_sweep_rows(*args, None, sp.rows.numel(), None) != 0
    parts, h = _hashed(rowptr, colind, g.n_cols)
    assert lib.cogdl_hip_csr_spmm_sweep_rows_guarded(*args, _lib.ptr(sp.rows), sp.rows.numel() + R, _lib.ptr(parts), h, 1, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------- through autograd, policy included
@pytest.fixture
def fresh(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    monkeypatch.setattr(plan, "VERIFY_HITS", False)
    plan.PLANS.clear()
    plan.clear_identity_memo()
    calls = {"pair": 0, "sweep": 0}
    real_pair, real_sweep = spmm_mod.csr_spmm_sweep_forward_raw, spmm_mod.csr_spmm_sweep_raw
    monkeypatch.setattr(spmm_mod, "csr_spmm_sweep_forward_raw", lambda *a, **k: (calls.__setitem__("pair", calls["pair"] + 1), real_pair(*a, **k))[1])
    monkeypatch.setattr(spmm_mod, "csr_spmm_sweep_raw", lambda *a, **k: (calls.__setitem__("sweep", calls["sweep"] + 1), real_sweep(*a, **k))[1])
    yield calls
    plan.PLANS.clear()
    plan.clear_identity_memo()


@pytest.fixture(scope="module")
def big():
    """The smallest structure the policy admits (a table of 70,000 rows of 512 bytes) and the ordinary launch's products."""
    g = synth.scaled(70_000, 8, seed=4).to(DEV)
    x, gout = _x(g.num_nodes, 0), _x(g.num_nodes, 2)
    csc = plan.csr2csc(g.rowptr, g.colind, g.n_cols)
    want = (_bytes(csr_spmm_raw(g.rowptr, g.colind, g.weight, x)),
            _bytes(csr_spmm_raw(csc.colptr, csc.rowind, csc.transposed_values(g.weight), gout)))
    return g, x, gout, want


@pytest.mark.parametrize("learned", [False, True])
def test_sightings_one_to_four_through_autograd(fresh, big, learned):
    """Constant weights and weights that require grad: sighting 1 ordinary, from 2 on the backward walks the dealt layout, from 3
    on the forward speculates on its own; every result is the ordinary launch's, bit for bit."""
    g, x, gout, (want_out, want_grad) = big
    grads_w = []
    for sighting, (pairs, sweeps) in enumerate(((0, 0), (0, 1), (1, 2), (2, 3)), start=1):
        xd = x.clone().requires_grad_()
        w = g.weight.clone().requires_grad_() if learned else g.weight
        out = csrspmm(g.rowptr.long().int(), g.colind.long().int(), xd, w, True)
        out.backward(gout)
        assert (fresh["pair"], fresh["sweep"]) == (pairs, sweeps), "sighting %d" % sighting
        assert _bytes(out) == want_out and _bytes(xd.grad) == want_grad, "sighting %d" % sighting
        if learned:
            grads_w.append(_bytes(w.grad))
    assert len(set(grads_w)) <= 1
    (csc,) = plan.PLANS.lru.values()
    (sp,) = sweepplan.FORWARD.lru.values()
    for layout, ptr in ((csc.sweep, csc.colptr), (sp, g.rowptr)):  # the policy's layouts are dealt ones
        assert layout.rows is not None and layout.rows.numel() == layout.n_groups * layout.r
        edges = (layout.goff[1:] - layout.goff[:-1]).long()
        assert int(edges.max() - edges.min()) <= int((ptr[1:] - ptr[:-1]).max())  # (the deal's bound: the largest row)
