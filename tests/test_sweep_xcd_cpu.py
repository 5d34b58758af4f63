"""The XCD-aware assignment of rows to sweep groups (cogdl_amd/sweepplan.py: deal_by_xcd, partition_rows; the law is
csrc/sweep_partition_law.h) through its host twin, torch on CPU tensors.  What must hold: an assignment checked_assignment
accepts, of ceil(n_rows / r) groups; every XCD holds exactly the rows and the edges its starting deal gave it (no more rows than
its groups have slots, and its edges within 1 % of its share of them); inside an XCD the deal's bound, max - min
edges per group <= the XCD's largest row; the same labels on every call; fewer distinct (XCD, gathered row) pairs than
deal_by_degree; and layouts in which every row still sees its own edges in its own order."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from cogdl_amd import _lib, sweepplan, synth

MASK = (1 << 24) - 1


def _transpose(g):
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    row = torch.repeat_interleave(torch.arange(g.num_nodes), deg)
    perm = torch.sort(g.colind.long(), stable=True).indices
    colptr = torch.zeros(g.n_cols + 1, dtype=torch.long)
    torch.cumsum(torch.bincount(g.colind.long(), minlength=g.n_cols), 0, out=colptr[1:])
    return colptr.int(), row[perm].int(), perm.int()


def _running_max(rowptr, colind):
    row = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), (rowptr[1:] - rowptr[:-1]).long())
    base = row * (int(colind.max()) + 1)
    return torch.cummax(colind.long() + base, 0).values - base


def _xcd_of_rows(assign, n_rows):
    """-> (the XCD of every row, the XCD of every group, n_xcd) under the kernel's rule."""
    n_groups, r = assign.shape
    xcd, n_xcd = sweepplan.group_xcd(n_groups)
    flat = assign.reshape(-1)
    real = torch.nonzero(flat >= 0).flatten()
    out = torch.empty(n_rows, dtype=torch.long)
    out[flat[real]] = xcd[real // r]
    return out, xcd, n_xcd


def _pairs(ptr, ind, xcd_of_row, n_src):
    row = torch.repeat_interleave(torch.arange(ptr.numel() - 1), (ptr[1:] - ptr[:-1]).long())
    return int(torch.unique(xcd_of_row[row] * n_src + ind.long()).numel())


def _check(ptr, ind, key, n_src, r):
    """deal_by_xcd on one structure against everything the module's docstring lists -> (assignment, pairs, the deal's pairs)."""
    n_rows = ptr.numel() - 1
    deg = (ptr[1:] - ptr[:-1]).long()
    a = sweepplan.deal_by_xcd(ptr, r, key, ind, n_src)
    assert a.shape == ((n_rows + r - 1) // r, r)
    sweepplan.checked_assignment(a, n_rows, r)
    assert torch.equal(a, sweepplan.deal_by_xcd(ptr, r, key, ind, n_src)), "two calls, two assignments"
    mine, xcd, n_xcd = _xcd_of_rows(a, n_rows)
    dealt, _, _ = _xcd_of_rows(sweepplan.deal_by_degree(ptr, r, key), n_rows)
    groups_of = torch.bincount(xcd, minlength=n_xcd)
    rows_of, edges_of = torch.bincount(mine, minlength=n_xcd), torch.bincount(mine, weights=deg.double(), minlength=n_xcd)
    assert bool((rows_of <= groups_of * r).all()), "more rows than an XCD's groups have slots"
    # zero rounds: the starting labels -- the partitioner leaves every XCD's rows and edges exactly what they were
    begin, _, _ = _xcd_of_rows(sweepplan.deal_by_xcd(ptr, r, key, ind, n_src, rounds=0), n_rows)
    assert torch.equal(rows_of, torch.bincount(begin, minlength=n_xcd))
    assert torch.equal(edges_of, torch.bincount(begin, weights=deg.double(), minlength=n_xcd))
    # 1 % of the mean: of the XCD's share of the edges by its groups (n_groups need not be a multiple of the XCDs' workgroups;
    # what the bound protects is the tail of the launch, which is edges per WAVE)
    share = float(deg.sum()) * groups_of.double() / a.shape[0]
    assert bool(((edges_of - share).abs() <= 0.01 * share).all()), (edges_of, share)
    if int(groups_of.min()) == int(groups_of.max()):  # ... which is the mean itself where the XCDs hold equally many groups
        assert bool(((edges_of - edges_of.mean()).abs() <= 0.01 * edges_of.mean()).all()), edges_of
    per_group = torch.where(a >= 0, deg[a.clamp(min=0)], torch.zeros_like(a)).sum(1)
    for x in range(n_xcd):
        here = per_group[xcd == x]
        assert int(here.max() - here.min()) <= int(deg[mine == x].max()), "XCD %d" % x
    # the longest rows come first inside a group (they are its register rows)
    d = torch.where(a >= 0, deg[a.clamp(min=0)], torch.full_like(a, -1))
    assert bool((d[:, 1:] <= d[:, :-1]).all())
    return a, _pairs(ptr, ind, mine, n_src), _pairs(ptr, ind, dealt, n_src)


def _check_rows_keep_their_order(sp, ptr, ind, eid_of_edge, assign):
    nnz = ind.numel()
    flat = assign.reshape(-1).long()
    assert torch.equal(sp.rows.long(), flat) and sp.n_groups == assign.shape[0]
    goff, src, eid = sp.goff.long(), sp.src.long(), sp.eid.long()
    group = torch.repeat_interleave(torch.arange(sp.n_groups), goff[1:] - goff[:-1])
    row = flat[group * sp.r + (src >> 24)]
    inv = torch.empty(nnz, dtype=torch.long)
    inv[eid_of_edge.long()] = torch.arange(nnz)
    at = inv[eid]
    assert torch.equal(src & MASK, ind.long()[at])
    owner = torch.repeat_interleave(torch.arange(ptr.numel() - 1), (ptr[1:] - ptr[:-1]).long())
    assert torch.equal(row, owner[at])
    assert torch.equal(at[torch.sort(row, stable=True).indices], torch.arange(nnz))


@pytest.mark.parametrize("r", [1, 5, 33, 48])
def test_both_directions_of_a_ragged_structure(r):
    """5,003 rows (20,011 for the two large r: fewer groups than four per XCD fall back) of 0-24 edges in any column order
    (rows without edges, duplicate pairs) over a table of another size (n_src != n_rows), and its transpose; neither row
    count is a multiple of any r but 1."""
    n = 5003 if r <= 5 else 20011
    g = synth.random_csr(n, n - 303, 12, seed=3)
    assert int(g.degrees().min()) == 0 and g.n_cols != g.num_nodes
    a, pairs, dealt = _check(g.rowptr, g.colind, _running_max(g.rowptr, g.colind), g.n_cols, r)
    assert pairs < dealt
    sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, r, sweepplan.deal_by_xcd)
    _check_rows_keep_their_order(sp, g.rowptr, g.colind, torch.arange(g.nnz), a)
    colptr, rowind, perm = _transpose(g)
    a, pairs, dealt = _check(colptr, rowind, rowind, g.num_nodes, r)
    assert pairs < dealt
    sp = sweepplan.build(colptr, rowind, perm, g.num_nodes, r, sweepplan.deal_by_xcd)
    _check_rows_keep_their_order(sp, colptr, rowind, perm, a)


def test_fewer_pairs_than_the_deal_on_the_simulators_graph():
    """The 20k-row graph of tests/test_sweep_groups_cpu.py's simulator test, r = 5, both directions: strictly fewer distinct
    (XCD, gathered row) pairs than deal_by_degree -- and the simulator's `ideal` is that count."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "exp", "sweep_hit_sim.py")
    spec = importlib.util.spec_from_file_location("sweep_hit_sim", path)
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    g = synth.scaled(20_000, 14, seed=0)
    colptr, rowind, _ = _transpose(g)
    for ptr, ind, key, n_src, fwd in ((colptr, rowind, rowind, g.num_nodes, False),
                                      (g.rowptr, g.colind, _running_max(g.rowptr, g.colind), g.n_cols, True)):
        a, pairs, dealt = _check(ptr, ind, key, n_src, 5)
        assert pairs < dealt
        lib = _lib.hip()
        assert sim.xcd_pairs(ptr.numpy(), ind.numpy(), a.numpy(), lib.cogdl_hip_csr_spmm_sweep_xcds(),
                             lib.cogdl_hip_csr_spmm_sweep_block_waves()) == pairs


def test_falls_back_to_the_deal_where_there_is_nothing_to_gain():
    """Fewer groups than four per XCD, and a structure without edges: deal_by_degree's assignment itself."""
    _, n_xcd = sweepplan.group_xcd(1)
    g = synth.random_csr(1200, 1500, 10, seed=5)
    r = 48
    assert (1200 + r - 1) // r < 4 * n_xcd
    key = _running_max(g.rowptr, g.colind)
    assert torch.equal(sweepplan.deal_by_xcd(g.rowptr, r, key, g.colind, g.n_cols), sweepplan.deal_by_degree(g.rowptr, r, key))
    ptr, none = torch.zeros(2001, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    assert torch.equal(sweepplan.deal_by_xcd(ptr, 5, none, none, 10), sweepplan.deal_by_degree(ptr, 5, none))


def test_partition_rows_holds_the_starting_labels_to_the_capacities():
    g = synth.random_csr(2000, 1500, 10, seed=6)
    start = torch.arange(2000) % 4
    cap = torch.full((4,), 500)
    out = sweepplan.partition_rows(g.rowptr, g.colind, g.n_cols, 4, cap, 3, start)
    assert out.dtype == torch.int32 and torch.equal(torch.bincount(out.long(), minlength=4), cap)
    assert not torch.equal(out.long(), start), "no row moved"
    assert torch.equal(sweepplan.partition_rows(g.rowptr, g.colind, g.n_cols, 4, cap, 0, start).long(), start)
    with pytest.raises(_lib.BackendError):
        sweepplan.partition_rows(g.rowptr, g.colind, g.n_cols, 4, cap - 1, 3, start)
    with pytest.raises(_lib.BackendError):
        sweepplan.partition_rows(g.rowptr, g.colind, g.n_cols, 3, cap[:3] * 2, 3, start)
    with pytest.raises(_lib.BackendError):  # a gathered row outside the table
        sweepplan.partition_rows(g.rowptr, g.colind, g.n_cols - 1000, 4, cap, 3, start)


def test_an_oversize_bucket_waits():
    """The law's bound on a round's cost: 12,000 rows of three edges each over two parts put far more than 2,048 candidates
    into bucket (0, 1, 3) and its mirror -- nobody moves, in any number of rounds; the first 3,000 of the same rows do swap."""
    n = 12_000
    ptr = torch.arange(0, 3 * n + 1, 3, dtype=torch.int32)
    ind = torch.randint(0, 500, (3 * n,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    start = torch.arange(n) % 2
    cap = torch.full((2,), n // 2)
    assert torch.equal(sweepplan.partition_rows(ptr, ind, 500, 2, cap, 3, start).long(), start)
    few = sweepplan.partition_rows(ptr[:3001], ind[:9000], 500, 2, cap, 3, start[:3000]).long()
    assert not torch.equal(few, start[:3000]) and int(few.sum()) == 1500


def test_deal_by_degree_and_assign_forms_are_what_they_were():
    """deal_by_degree's pinned outputs (tests/test_sweep_groups_cpu.py) once more, and `assign=` with a tensor or with
    deal_by_degree as a callable builds the same layout."""
    ptr = torch.arange(0, 13, 2)
    key = torch.tensor([50, 52, 10, 12, 30, 32, 0, 2, 20, 22, 40, 42])
    assert sweepplan.deal_by_degree(ptr, 2, key).tolist() == [[3, 0], [1, 5], [4, 2]]
    assert sweepplan.deal_by_degree(ptr, 2).tolist() == [[0, 5], [1, 4], [2, 3]]
    g = synth.random_csr(2003, 1700, 12, seed=3)
    by_call = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, 5, sweepplan.deal_by_degree)
    by_tensor = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, 5,
                                        sweepplan.deal_by_degree(g.rowptr, 5, _running_max(g.rowptr, g.colind)))
    for name in ("goff", "src", "eid", "rows"):
        assert torch.equal(getattr(by_call, name), getattr(by_tensor, name)), name
