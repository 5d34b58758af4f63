"""csr_spmm over the sweep layout of the transpose (include/cogdl_hip.h: cogdl_hip_csr_spmm_sweep; csrc/rowsweep.h;
cogdl_amd/sweepplan.py).  The sweep is a different EXECUTION ORDER of the backward launch, so `grad_x` must be bit-identical to
the ordinary launch on the same transpose, csr_spmm_raw(plan.colptr, plan.rowind, w_t, g), and to the CPU oracle's csr_spmm on
A^T (oracle/cogdl_oracle.c, which follows spmm_cpu.cpp:24-35) wherever no row of the transpose exceeds the exact-row bound."""
import numpy as np
import pytest
import torch

from cogdl_amd import _lib, plan, sweepplan, synth, xcdplan
from cogdl_amd.operators import spmm as spmm_mod
from cogdl_amd.operators.spmm import csr_spmm_raw, csr_spmm_sweep_raw, csrspmm
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 128


def _rows():
    return int(_lib.hip().cogdl_hip_csr_spmm_sweep_group_rows())


def _gout(n, seed=1):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed))


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _check_raw(g, r, weighted=True, oracle_too=True):
    """The sweep over g's transpose in groups of r rows against the ordinary launch and the oracle, bit for bit."""
    rowptr, colind = g.rowptr.to(DEV), g.colind.to(DEV)
    w = g.weight.to(DEV) if weighted else None
    csc = plan.csr2csc(rowptr, colind, g.n_cols)
    gout = _gout(g.num_nodes)
    gd = gout.to(DEV)
    w_t = csc.transposed_values(w) if weighted else None
    want = csr_spmm_raw(csc.colptr, csc.rowind, w_t, gd, split_long_rows=csc.has_hub_columns())
    csc.sweep = sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, r)
    got = csr_spmm_sweep_raw(csc, w, gd)
    assert got.shape == (g.n_cols, F)
    assert _bytes(got) == _bytes(want), "sweep != ordinary launch"
    if oracle_too:
        colptr, rowind, w_t_cpu, _ = oracle.csr2csc(g.rowptr, g.colind, g.weight if weighted else None, n_cols=g.n_cols)
        ref = oracle.csr_spmm(colptr, rowind, w_t_cpu if weighted else None, gout)
        assert _bytes(got) == ref.tobytes(), "sweep != oracle on the transpose"
    return csc


def _transposed(b):
    """The structure whose stable transpose has b's rows (columns ascending inside a row; duplicates kept)."""
    colptr, rowind, w_t, _ = oracle.csr2csc(b.rowptr, b.colind, b.weight, n_cols=b.n_cols)
    w = None if w_t is None else torch.from_numpy(np.asarray(w_t, dtype=np.float32))
    return synth.CSRGraph(torch.from_numpy(np.asarray(colptr)).int(), torch.from_numpy(np.asarray(rowind)).int(), w, b.n_cols, b.num_nodes)


@pytest.mark.parametrize("which", ["1", "R-1", "R", "R+1", "4R+5"])
def test_row_group_boundaries(which):
    """Rows of the transpose: 1, R-1, R, R+1, 4R+5, ragged between 0 and 40 edges (10 % of them empty), gathering from a table
    of 700 rows (rectangular)."""
    R = _rows()
    n_rows = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "4R+5": 4 * R + 5}[which]
    a = _transposed(synth.random_csr(n_rows, 700, 20, seed=n_rows))
    assert (a.num_nodes, a.n_cols) == (700, n_rows)
    deg_t = torch.bincount(a.colind.long(), minlength=a.n_cols)
    assert int(deg_t.max()) <= 40
    _check_raw(a, R)


def test_fewer_rows_per_group_than_the_kernel_holds():
    """Several groups, rows of 0-40 edges, groups of 5 and of 33 rows (local rows on both sides of the register / LDS split)."""
    R = _rows()
    a = _transposed(synth.random_csr(3 * R + 7, 900, 20, seed=11))
    deg_t = torch.bincount(a.colind.long(), minlength=a.n_cols)
    assert int(deg_t.max()) <= 40 and int(deg_t.min()) == 0
    _check_raw(a, 5)
    _check_raw(a, 33)


def _with_column_degree(m, n_cols, col, degree, seed):
    """A ragged structure in which exactly `degree` rows name column `col` (once each)."""
    g = synth.random_csr(m, n_cols, 6, seed=seed)
    colind = g.colind.clone()
    colind[colind == col] = (col + 1) % n_cols
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    rows = torch.nonzero(deg > 0).flatten()[:degree]
    assert rows.numel() == degree
    colind[g.rowptr[rows].long()] = col
    return synth.CSRGraph(g.rowptr, colind, g.weight, m, n_cols)


def test_row_at_the_exact_row_bound():
    """A row of the transpose of exactly the long-row threshold: still one sequential sum in both launches and in the oracle."""
    g = _with_column_degree(400, 150, 7, 128, seed=3)
    thresh = _lib.hip().cogdl_hip_long_row_threshold(g.nnz)
    assert thresh == 128
    csc = _check_raw(g, _rows())
    assert csc._max_col_degree == thresh and not csc.has_hub_columns()


def test_unweighted():
    _check_raw(_transposed(synth.random_csr(3 * _rows() + 1, 500, 9, seed=5, weighted=False)), _rows(), weighted=False)


def test_more_than_one_round():
    """~3,000 rows of the transpose with one round capped at 10 waves (tuning key 18): the same waves walk further groups."""
    R = _rows()
    lib = _lib.hip()
    g = _transposed(synth.random_csr(3000, 1500, 12, seed=8))
    lib.cogdl_hip_set_tuning(18, 10 * R)
    try:
        assert lib.cogdl_hip_csr_spmm_sweep_round_rows(F, 0) == 10 * R
        _check_raw(g, R)
    finally:
        lib.cogdl_hip_set_tuning(18, 0)
    assert lib.cogdl_hip_csr_spmm_sweep_round_rows(F, 0) >= 64 * R


def test_entry_point_declines_other_shapes():
    lib = _lib.hip()
    assert lib.cogdl_hip_csr_spmm_sweep_round_rows(64, 0) == 0 and lib.cogdl_hip_csr_spmm_sweep_round_rows(F, 2) == 0
    g = synth.random_csr(50, 60, 4, seed=1)
    csc = plan.csr2csc(g.rowptr.to(DEV), g.colind.to(DEV), g.n_cols)
    csc.sweep = sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, _rows())
    with pytest.raises(_lib.BackendError):
        csr_spmm_sweep_raw(csc, None, torch.zeros(50, 64, device=DEV))


# ---------------------------------------------------------------------------------------- through autograd, policy included
@pytest.fixture
def fresh(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    plan.PLANS.clear()
    plan.clear_identity_memo()
    calls = []
    real = spmm_mod.csr_spmm_sweep_raw
    monkeypatch.setattr(spmm_mod, "csr_spmm_sweep_raw", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    yield calls
    plan.PLANS.clear()
    plan.clear_identity_memo()


def _step(g, x, w, gout):
    xd = x.clone().requires_grad_()
    # fresh int32 copies of the structure every call, as CogDL's dispatcher makes them
    out = csrspmm(g.rowptr.long().int(), g.colind.long().int(), xd, w, True)
    out.backward(gout)
    return out.detach(), xd.grad


@pytest.fixture(scope="module")
def big():
    """A structure the policy takes: a table of 70,000 rows of 512 bytes (35.8 MB, beyond the eight L2s)."""
    g = synth.scaled(70_000, 8, seed=4)
    gout = _gout(g.num_nodes, seed=2)
    colptr, rowind, w_t, _ = oracle.csr2csc(g.rowptr, g.colind, g.weight)
    return g.to(DEV), gout.to(DEV), oracle.csr_spmm(colptr, rowind, w_t, gout).tobytes()


def test_second_and_third_sighting_take_the_sweep(fresh, big):
    g, gout, want = big
    x = torch.randn(g.num_nodes, F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    out1, grad1 = _step(g, x, g.weight, gout)
    assert fresh == [], "a first sighting keeps the ordinary launch"
    before = plan.PLANS.bytes
    out2, grad2 = _step(g, x, g.weight, gout)
    out3, grad3 = _step(g, x, g.weight, gout)
    assert len(fresh) == 2
    assert _bytes(grad1) == want
    assert _bytes(grad2) == _bytes(grad1) and _bytes(grad3) == _bytes(grad1)
    assert _bytes(out2) == _bytes(out1) and _bytes(out3) == _bytes(out1)
    (csc,) = plan.PLANS.lru.values()
    sp = csc.sweep
    assert sp is not None and sp._val_p is not None  # constant weights: permuted once, kept
    assert plan.PLANS.bytes == csc.nbytes() == before + 4 * (2 * csc.nnz + sp.n_groups + 1) + 4 * csc.nnz
    memo = sp._val_p
    _step(g, x, g.weight, gout)
    assert sp._val_p is memo and csc.sweep is sp


def test_learned_weights_are_not_memoised(fresh, big):
    g, gout, want = big
    x = torch.randn(g.num_nodes, F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))

    def step():
        xd, w = x.clone().requires_grad_(), g.weight.clone().requires_grad_()
        csrspmm(g.rowptr.long().int(), g.colind.long().int(), xd, w, True).backward(gout)
        return xd.grad, w.grad

    gx1, gw1 = step()
    gx2, gw2 = step()
    assert len(fresh) == 1
    assert _bytes(gx1) == want and _bytes(gx2) == want
    assert _bytes(gw2) == _bytes(gw1)
    (csc,) = plan.PLANS.lru.values()
    assert csc.sweep is not None and csc.sweep._val_p is None


def test_hub_transpose_keeps_the_ordinary_launch(fresh):
    """One row of the transpose above the threshold: the policy declines at every sighting, and the result is the ordinary
    launch's (which re-associates that row) bit for bit."""
    g = _with_column_degree(70_000, 70_000, 9, 1500, seed=6)
    assert _lib.hip().cogdl_hip_long_row_threshold(g.nnz) < 1500
    gd = g.to(DEV)
    gout = _gout(g.num_nodes, seed=3).to(DEV)
    x = torch.randn(g.num_nodes, F, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    _, grad1 = _step(gd, x, gd.weight, gout)
    _, grad2 = _step(gd, x, gd.weight, gout)
    _, grad3 = _step(gd, x, gd.weight, gout)
    assert fresh == []
    (csc,) = plan.PLANS.lru.values()
    assert csc.sightings >= 3 and csc.has_hub_columns() and csc.sweep is None
    assert not xcdplan.spmm_backward_sweep(csc, gout)
    want = csr_spmm_raw(csc.colptr, csc.rowind, csc.transposed_values(gd.weight), gout, split_long_rows=True)
    assert _bytes(grad1) == _bytes(want) and _bytes(grad2) == _bytes(want) and _bytes(grad3) == _bytes(want)
