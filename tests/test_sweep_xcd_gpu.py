"""The XCD-aware assignment on the GPU (cogdl_amd/sweepplan.py: deal_by_xcd; csrc/sweep_partition.hip): the kernels' labels are
the host twin's exactly (csrc/sweep_partition_law.h), and layouts built over the assignment give, in every launch form, the
bytes of csr_spmm_raw on the same structure -- which rows share a wave, or an XCD, never changes a sum.  fp32, F = 128."""
import pytest
import torch

from cogdl_amd import _lib, plan, sweepplan, synth, xcdplan
from cogdl_amd.operators import spmm as spmm_mod
from cogdl_amd.operators.spmm import csr_spmm_raw, csr_spmm_sweep_forward_raw, csr_spmm_sweep_raw, csrspmm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 128
U64 = (1 << 64) - 1


def _x(n, seed=1):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def ragged():
    """5,003 rows of 0-24 edges in any column order (rows without edges, duplicates) over a table of 4,700 rows; its transpose;
    the ordinary launch's product of each -- computed once."""
    g = synth.random_csr(5003, 4700, 12, seed=3)
    assert int(g.degrees().min()) == 0
    rowptr, colind, w = g.rowptr.to(DEV), g.colind.to(DEV), g.weight.to(DEV)
    x, gout = _x(g.n_cols, 1), _x(g.num_nodes, 2)
    csc = plan.csr2csc(rowptr, colind, g.n_cols)
    want = {"fwd": _bytes(csr_spmm_raw(rowptr, colind, w, x)),
            "bwd": _bytes(csr_spmm_raw(csc.colptr, csc.rowind, csc.transposed_values(w), gout))}
    fp = plan.Fingerprint(rowptr, colind, g.n_cols, dev_parts=True)
    return g, rowptr, colind, w, x, gout, csc, want, fp.dev, fp.key()[4] & U64


def test_device_labels_are_the_host_twins(ragged):
    """Both directions, 0 to 5 rounds from the same start, and a start with labels only in some parts: equal labels, and the
    kernels give the same labels on a second launch."""
    g, rowptr, colind, _, _, _, csc, _, _, _ = ragged
    for ptr, ind, n_src in ((rowptr, colind, g.n_cols), (csc.colptr, csc.rowind, g.num_nodes)):
        n_rows = ptr.numel() - 1
        for n_parts, rounds in ((8, 0), (8, 1), (8, 5), (3, 4), (1, 2)):
            start = (torch.arange(n_rows) * 7 % n_parts).int()
            cap = torch.bincount(start.long(), minlength=n_parts)
            host = sweepplan.partition_rows(ptr.cpu(), ind.cpu(), n_src, n_parts, cap, rounds, start)
            dev = sweepplan.partition_rows(ptr, ind, n_src, n_parts, cap, rounds, start.to(DEV))
            again = sweepplan.partition_rows(ptr, ind, n_src, n_parts, cap, rounds, start.to(DEV))
            assert dev.is_cuda and torch.equal(dev.cpu(), host) and torch.equal(again, dev), (n_parts, rounds)
            assert (rounds == 0 or n_parts == 1) == torch.equal(host, start)


@pytest.mark.parametrize("r", [1, 5, 33, 48])
def test_every_launch_form_is_bit_identical(ragged, r):
    """Backward sweep, the bare forward walk (the guarded pair on a match) and the pair on a mismatch, over deal_by_xcd layouts
    built on the device; the assignment is the one the host twin gives (r = 48: 105 groups; r = 1: 5,003)."""
    g, rowptr, colind, w, x, gout, csc, want, parts, h = ragged
    mine = plan.CscPlan(csc.colptr, csc.rowind, csc.perm, csc.m, csc.n_cols, csc.nnz)
    mine.sweep = sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, r, sweepplan.deal_by_xcd)
    on_host = sweepplan.deal_by_xcd(csc.colptr.cpu(), r, csc.rowind.cpu().long(), csc.rowind.cpu().long(), csc.m)
    assert torch.equal(mine.sweep.rows.cpu().long(), on_host.reshape(-1))
    assert not torch.equal(on_host, sweepplan.deal_by_degree(csc.colptr.cpu(), r, csc.rowind.cpu().long()))
    assert _bytes(csr_spmm_sweep_raw(mine, w, gout)) == want["bwd"], "backward sweep != ordinary launch on the transpose"
    sp = sweepplan.build_forward(rowptr, colind, g.n_cols, r, sweepplan.deal_by_xcd)
    assert sp.rows is not None and sp.rows.numel() == sp.n_groups * r and sp.n_groups == (g.num_nodes + r - 1) // r
    for match in (True, False):
        sp.hash = h if match else h ^ 1
        assert _bytes(csr_spmm_sweep_forward_raw(sp, parts, rowptr, colind, w, x)) == want["fwd"], "guarded pair, match=%s" % match
    # which side ran on a match: the layout of ANOTHER structure under this structure's hash gives the other's product
    other = ((colind.long() + 1) % g.n_cols).int()
    sp = sweepplan.build_forward(rowptr, other, g.n_cols, r, sweepplan.deal_by_xcd)
    sp.hash = h
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts, rowptr, colind, w, x)) == _bytes(csr_spmm_raw(rowptr, other, w, x))


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


@pytest.mark.parametrize("learned", [False, True])
def test_sightings_one_to_four_carry_the_xcd_assignment(fresh, learned):
    """The smallest structure the policy admits, constant and learned weights: every sighting's results are the ordinary
    launch's bytes, and the policy's two layouts are deal_by_xcd's -- their row maps are what the procedure gives for the
    structure, not deal_by_degree's."""
    assert sweepplan.ASSIGN is sweepplan.deal_by_xcd
    g = synth.scaled(70_000, 8, seed=4).to(DEV)
    x, gout = _x(g.num_nodes, 0), _x(g.num_nodes, 2)
    csc0 = plan.csr2csc(g.rowptr, g.colind, g.n_cols)
    want_out = _bytes(csr_spmm_raw(g.rowptr, g.colind, g.weight, x))
    want_grad = _bytes(csr_spmm_raw(csc0.colptr, csc0.rowind, csc0.transposed_values(g.weight), gout))
    for sighting, (pairs, sweeps) in enumerate(((0, 0), (0, 1), (1, 2), (2, 3)), start=1):
        xd = x.clone().requires_grad_()
        w = g.weight.clone().requires_grad_() if learned else g.weight
        out = csrspmm(g.rowptr.long().int(), g.colind.long().int(), xd, w, True)
        out.backward(gout)
        assert (fresh["pair"], fresh["sweep"]) == (pairs, sweeps), "sighting %d" % sighting
        assert _bytes(out) == want_out and _bytes(xd.grad) == want_grad, "sighting %d" % sighting
    (csc,) = plan.PLANS.lru.values()
    (sp,) = sweepplan.FORWARD.lru.values()
    back = sweepplan.deal_by_xcd(csc.colptr, csc.sweep.r, csc.rowind.long(), csc.rowind.long(), csc.m)
    assert torch.equal(csc.sweep.rows.long(), back.reshape(-1))
    assert not torch.equal(back, sweepplan.deal_by_degree(csc.colptr, csc.sweep.r, csc.rowind.long()))
    assert sp.rows is not None and sp.rows.numel() == sp.n_groups * sp.r
    assert not torch.equal(sp.rows.long(), sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, sp.r, sweepplan.deal_by_degree).rows.long())
