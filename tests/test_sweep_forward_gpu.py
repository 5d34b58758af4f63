"""The forward pass of csr_spmm over the sweep layout of a structure seen before (cogdl_amd/sweepplan.py: build_forward;
include/cogdl_hip.h: cogdl_hip_csr_spmm_sweep_guarded, cogdl_hip_csr_spmm_guarded, cogdl_hip_csr_fingerprint_dev).  The call
enqueues TWO launches that compare the structure hash on the device -- the sweep runs on a match, the ordinary launch otherwise --
and whichever runs must give the bytes of csr_spmm_raw and of the CPU oracle (oracle/cogdl_oracle.c, which follows
spmm_cpu.cpp:24-35) wherever no row exceeds the exact-row bound.  Which side ran is read off the outputs: a layout that names
ANOTHER structure's edges gives that structure's product when (and only when) the sweep ran."""
import pytest
import torch

from cogdl_amd import _lib, graphs, plan, sweepplan, synth, xcdplan
from cogdl_amd.operators import spmm as spmm_mod
from cogdl_amd.operators.spmm import csr_spmm_raw, csr_spmm_sweep_forward_raw, csrspmm
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 128
U64 = (1 << 64) - 1


def _rows():
    return int(_lib.hip().cogdl_hip_csr_spmm_sweep_group_rows())


def _x(n, seed=1):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed))


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _hashed(rowptr, colind, n_src):
    """-> (device partials, 64-bit hash) of the structure, as a speculating forward call computes them."""
    fp = plan.Fingerprint(rowptr, colind, n_src, dev_parts=True)
    return fp.dev, fp.key()[4] & U64


def _check_pair(g, r, weighted=True, oracle_too=True):
    """The guarded pair over g's own layout in groups of r rows (the hash matches: the sweep runs) against the ordinary launch
    and the oracle, bit for bit."""
    rowptr, colind = g.rowptr.to(DEV), g.colind.to(DEV)
    w = g.weight.to(DEV) if weighted else None
    x = _x(g.n_cols)
    xd = x.to(DEV)
    want = csr_spmm_raw(rowptr, colind, w, xd)
    sp = sweepplan.build_forward(rowptr, colind, g.n_cols, r)
    parts, sp.hash = _hashed(rowptr, colind, g.n_cols)
    got = csr_spmm_sweep_forward_raw(sp, parts, rowptr, colind, w, xd)
    assert got.shape == (g.num_nodes, F)
    assert _bytes(got) == _bytes(want), "guarded pair != ordinary launch"
    if oracle_too:
        ref = oracle.csr_spmm(g.rowptr, g.colind, g.weight if weighted else None, x)
        assert _bytes(got) == ref.tobytes(), "guarded pair != oracle"
    return sp


@pytest.mark.parametrize("r", ["R", 5])
@pytest.mark.parametrize("which", ["3r-1", "3r", "3r+1"])
def test_row_group_boundaries(which, r):
    """3r - 1, 3r and 3r + 1 rows in groups of r = 48 and r = 5 rows: self-loop-appended rows (what the policy admits), a square
    structure."""
    r = _rows() if r == "R" else r
    m = {"3r-1": 3 * r - 1, "3r": 3 * r, "3r+1": 3 * r + 1}[which]
    _check_pair(synth.scaled(m, 6, seed=m), r)


def test_fully_unsorted_rows_and_a_rectangular_table():
    """Rows in random column order, with duplicates and empty rows, gathering from a table of 700 rows (n_src != m): the policy
    would decline (most edges lie behind their row's running maximum); the raw entry must be correct all the same."""
    g = synth.random_csr(3 * _rows() + 7, 700, 20, seed=11)
    assert int(g.degrees().min()) == 0 and g.n_cols != g.num_nodes
    sp = _check_pair(g, _rows())
    assert sp.out_of_order > 0.5
    _check_pair(g, 33)  # (local rows on both sides of the register / LDS split)


def test_row_at_the_exact_row_bound():
    """A row of exactly the long-row threshold: still one sequential sum in both launches and in the oracle."""
    g = synth.hub_csr(400, 150, base_deg=6, hubs=((7, 128),), seed=3)
    assert _lib.hip().cogdl_hip_exact_row_edges(g.nnz) == 128 and int(g.degrees().max()) == 128
    sp = _check_pair(g, _rows())
    assert not sp.long_rows


def test_unweighted():
    _check_pair(synth.scaled(3 * _rows() + 1, 9, seed=5), _rows(), weighted=False)


def test_more_than_one_round():
    """3,000 rows with one round capped at 10 waves (tuning key 18): the same waves walk further groups."""
    R = _rows()
    lib = _lib.hip()
    g = synth.scaled(3000, 12, seed=8)
    lib.cogdl_hip_set_tuning(18, 10 * R)
    try:
        assert lib.cogdl_hip_csr_spmm_sweep_round_rows(F, 0) == 10 * R
        _check_pair(g, R)
    finally:
        lib.cogdl_hip_set_tuning(18, 0)


@pytest.fixture(scope="module")
def twins():
    """Two structures with equal (m, nnz, n_src) and different column ids, a table, and each one's ordinary product."""
    a = synth.scaled(1000, 8, seed=21)
    rowptr, ca, w = a.rowptr.to(DEV), a.colind.to(DEV), a.weight.to(DEV)
    cb = ((ca.long() + 1) % a.n_cols).int()
    x = _x(a.n_cols, seed=4).to(DEV)
    ya, yb = csr_spmm_raw(rowptr, ca, w, x), csr_spmm_raw(rowptr, cb, w, x)
    assert _bytes(ya) != _bytes(yb)
    return a, rowptr, ca, cb, w, x, ya, yb


def test_mismatch_runs_the_ordinary_launch(twins):
    """The candidate is the first structure, the call passes the second: the result is the second's ordinary result."""
    a, rowptr, ca, cb, w, x, ya, yb = twins
    sp = sweepplan.build_forward(rowptr, ca, a.n_cols, _rows())
    _, sp.hash = _hashed(rowptr, ca, a.n_cols)
    parts_b, hash_b = _hashed(rowptr, cb, a.n_cols)
    assert hash_b != sp.hash
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts_b, rowptr, cb, w, x)) == _bytes(yb)
    # ... and the same call with the candidate's own structure takes the layout's side (next test) with the same bytes
    parts_a, _ = _hashed(rowptr, ca, a.n_cols)
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts_a, rowptr, ca, w, x)) == _bytes(ya)


def test_match_runs_the_sweep(twins):
    """Which side ran, seen from outside: a layout of the SECOND structure's edges under the FIRST structure's hash.  A call that
    passes the first structure matches, so the sweep runs -- over the layout it was given: the second structure's product; a
    call whose hash differs gets the ordinary launch over what it passed."""
    a, rowptr, ca, cb, w, x, ya, yb = twins
    sp = sweepplan.build_forward(rowptr, cb, a.n_cols, _rows())
    parts_a, sp.hash = _hashed(rowptr, ca, a.n_cols)
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts_a, rowptr, ca, w, x)) == _bytes(yb)
    sp.hash = (sp.hash + 1) & U64
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts_a, rowptr, ca, w, x)) == _bytes(ya)


def test_in_place_edit_of_one_column_id(twins):
    a, rowptr, ca, _, w, x, ya, _ = twins
    sp = sweepplan.build_forward(rowptr, ca, a.n_cols, _rows())
    _, sp.hash = _hashed(rowptr, ca, a.n_cols)
    edited = ca.clone()
    edited[5] = (int(edited[5]) + 3) % a.n_cols
    want = csr_spmm_raw(rowptr, edited, w, x)
    assert _bytes(want) != _bytes(ya)
    parts, _ = _hashed(rowptr, edited, a.n_cols)
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts, rowptr, edited, w, x)) == _bytes(want)


def test_device_partials_are_the_pinned_ones():
    g = synth.scaled(500, 6, seed=2).to(DEV)
    fp = plan.Fingerprint(g.rowptr, g.colind, g.n_cols, dev_parts=True)
    plain = plan.Fingerprint(g.rowptr, g.colind, g.n_cols)
    assert plain.dev is None and fp.key() == plain.key()
    assert torch.equal(fp.dev.cpu(), fp.host)


def test_entry_points_decline_other_shapes():
    g = synth.scaled(50, 4, seed=1).to(DEV)
    sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, _rows())
    parts, sp.hash = _hashed(g.rowptr, g.colind, g.n_cols)
    with pytest.raises(_lib.BackendError):
        csr_spmm_sweep_forward_raw(sp, parts, g.rowptr, g.colind, None, torch.zeros(50, 64, device=DEV))
    with pytest.raises(_lib.BackendError):
        csr_spmm_sweep_forward_raw(sp, parts[:8], g.rowptr, g.colind, None, torch.zeros(50, F, device=DEV))
    lib = _lib.hip()
    x = torch.zeros(50, F, device=DEV)
    out = torch.empty(50, F, device=DEV)
    args = (_lib.ptr(g.rowptr), _lib.ptr(g.colind), None, _lib.ptr(x), _lib.ptr(out), 50, F, g.nnz)
    assert lib.cogdl_hip_csr_spmm_guarded(*args, 2, _lib.ptr(parts), sp.hash, 0, None, 0, None) != 0   # bf16
    assert lib.cogdl_hip_csr_spmm_guarded(*args, 0, None, sp.hash, 0, None, 0, None) != 0               # no partials
    assert lib.cogdl_hip_csr_spmm_guarded(*args, 0, _lib.ptr(parts), sp.hash, 2, None, 0, None) != 0   # no such sense
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- through autograd, policy included
@pytest.fixture
def fresh(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    monkeypatch.setattr(plan, "VERIFY_HITS", False)
    plan.PLANS.clear()
    plan.clear_identity_memo()
    calls = {"pair": 0, "ordinary": 0}
    real_pair, real_raw = spmm_mod.csr_spmm_sweep_forward_raw, spmm_mod.csr_spmm_raw

    def pair(*a, **k):
        calls["pair"] += 1
        return real_pair(*a, **k)

    def raw(*a, **k):
        calls["ordinary"] += 1
        return real_raw(*a, **k)

    monkeypatch.setattr(spmm_mod, "csr_spmm_sweep_forward_raw", pair)
    monkeypatch.setattr(spmm_mod, "csr_spmm_raw", raw)
    yield calls
    plan.PLANS.clear()
    plan.clear_identity_memo()


@pytest.fixture(scope="module")
def big():
    """The smallest structure the policy admits: a table of 70,000 rows of 512 bytes (35.8 MB, beyond the eight L2s)."""
    g = synth.scaled(70_000, 8, seed=4)
    x, gout = _x(g.num_nodes, seed=0), _x(g.num_nodes, seed=2)
    colptr, rowind, w_t, _ = oracle.csr2csc(g.rowptr, g.colind, g.weight)
    want = oracle.csr_spmm(g.rowptr, g.colind, g.weight, x).tobytes(), oracle.csr_spmm(colptr, rowind, w_t, gout).tobytes()
    return g.to(DEV), x.to(DEV), gout.to(DEV), want


def _step(g, x, w, gout):
    xd = x.clone().requires_grad_()
    # fresh int32 copies of the structure every call, as CogDL's dispatcher makes them
    out = csrspmm(g.rowptr.long().int(), g.colind.long().int(), xd, w, True)
    out.backward(gout)
    return out.detach(), xd.grad


def test_third_sighting_takes_the_guarded_pair(fresh, big):
    g, x, gout, (want_out, want_grad) = big
    results = []
    for sighting, pairs in ((1, 0), (2, 0), (3, 1), (4, 2)):
        results.append(_step(g, x, g.weight, gout))
        assert fresh["pair"] == pairs, "sighting %d" % sighting
    assert fresh["ordinary"] == 3  # the forwards of sightings 1 and 2, the backward of sighting 1 (from 2 on: the sweep)
    for out, grad in results:
        assert _bytes(out) == want_out and _bytes(grad) == want_grad
    (sp,) = sweepplan.FORWARD.lru.values()
    assert sp.out_of_order <= 0.125 and not sp.long_rows and sp._val_p is not None  # constant weights: permuted once, kept
    assert sweepplan.FORWARD.bytes == sp.nbytes() == 4 * (2 * sp.nnz + sp.n_groups + 1) + 4 * sp.nnz
    (csc,) = plan.PLANS.lru.values()
    assert plan.PLANS.bytes == csc.nbytes()  # (the forward layout is not the plan cache's)
    memo = sp._val_p
    _step(g, x, g.weight, gout)
    assert sp._val_p is memo and fresh["pair"] == 3


def test_another_structure_of_the_same_shape_gets_its_own_result(fresh, big):
    """The candidate is registered, then a call passes a structure of the same (m, nnz, n_src) with other column ids: it
    speculates, the device finds the mismatch, and the result is that structure's ordinary result."""
    g, x, gout, _ = big
    for _ in range(3):
        _step(g, x, g.weight, gout)
    assert fresh["pair"] == 1
    other = ((g.colind.long() + 1) % g.n_cols).int()
    want = spmm_mod.csr_spmm_raw(g.rowptr, other, g.weight, x)
    out = csrspmm(g.rowptr.long().int(), other.long().int(), x.clone().requires_grad_(), g.weight, True)
    assert fresh["pair"] == 2 and _bytes(out) == _bytes(want)


def test_learned_weights_are_gathered_per_call(fresh, big):
    g, x, gout, (want_out, want_grad) = big

    def step():
        xd, w = x.clone().requires_grad_(), g.weight.clone().requires_grad_()
        out = csrspmm(g.rowptr.long().int(), g.colind.long().int(), xd, w, True)
        out.backward(gout)
        return out.detach(), xd.grad, w.grad

    first = step()
    runs = [step(), step(), step()]
    assert fresh["pair"] == 2
    for out, gx, gw in runs:
        assert _bytes(out) == want_out and _bytes(gx) == want_grad and _bytes(gw) == _bytes(first[2])
    (sp,) = sweepplan.FORWARD.lru.values()
    assert sp._val_p is None  # nothing memoised


def _registered(g, x, gout):
    for _ in range(2):
        _step(g, x, g.weight, gout)
    assert len(sweepplan.FORWARD.lru) == 1 and len(plan.CANDIDATES) == 1


def test_policy_refusal_inside_transient_structures(fresh, big):
    g, x, gout, (want_out, _) = big
    _registered(g, x, gout)
    with plan.transient_structures():
        out, _ = _step(g, x, g.weight, gout)
    assert fresh["pair"] == 0 and _bytes(out) == want_out


def test_policy_refusal_with_mode_off(fresh, big, monkeypatch):
    g, x, gout, (want_out, _) = big
    _registered(g, x, gout)
    monkeypatch.setattr(xcdplan, "MODE", "off")
    out, _ = _step(g, x, g.weight, gout)
    assert fresh["pair"] == 0 and _bytes(out) == want_out
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    _step(g, x, g.weight, gout)
    assert fresh["pair"] == 1


def test_policy_refusal_under_capture(fresh, big):
    g, x, gout, (want_out, want_grad) = big
    _registered(g, x, gout)
    xd = x.clone().requires_grad_()

    def step():
        out = csrspmm(g.rowptr.long().int(), g.colind.long().int(), xd, g.weight, True)
        xd.grad = None
        out.backward(gout)
        return out, xd.grad

    captured = graphs.capture(step, warmup=1)  # (its one eager run is the recorded one: under the tape like the capture)
    out, grad = captured()
    torch.cuda.synchronize()
    assert fresh["pair"] == 0
    assert _bytes(out) == want_out and _bytes(grad) == want_grad
