"""Sweep layouts over an explicit assignment of rows to groups (cogdl_amd/sweepplan.py: `assign=`, checked_assignment,
deal_by_degree) and the CPU model that rates an assignment (tools/exp/sweep_hit_sim.py) -- host logic only, torch on CPU tensors.
What an assignment must be: a partition of the rows into groups of at most r rows, pads only as a group's trailing negatives.
What the layout over it must keep for bit-identical sums: a permutation of the edges in which every row sees its own edges in
exactly its own order, whichever rows share its group."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from cogdl_amd import _lib, sweepplan, synth

R = 48  # (csrc/rowsweep.h: kSweepRows; the CPU tests do not ask the library)
MASK = (1 << 24) - 1


def _transpose(g):
    """Stable transpose of a synth.CSRGraph with torch ops -> colptr, rowind, perm (int32), as plan.csr2csc lays them out."""
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    row = torch.repeat_interleave(torch.arange(g.num_nodes), deg)
    perm = torch.sort(g.colind.long(), stable=True).indices
    colptr = torch.zeros(g.n_cols + 1, dtype=torch.long)
    torch.cumsum(torch.bincount(g.colind.long(), minlength=g.n_cols), 0, out=colptr[1:])
    return colptr.int(), row[perm].int(), perm.int()


def _check_assignment(assign, n_rows, r):
    assert assign.shape == ((n_rows + r - 1) // r, r)
    flat = assign.reshape(-1)
    assert torch.equal(torch.sort(flat[flat >= 0]).values, torch.arange(n_rows)), "not a partition of the rows"
    real = assign >= 0
    assert not bool((real[:, 1:] & ~real[:, :-1]).any()), "a pad in front of a row"


def _check_layout(sp, ptr, ind, eid_of_edge, n_src, r, assign, key):
    """sp against the structure (ptr, ind) whose edge e is edge eid_of_edge[e] of the caller; key: the merge key per edge."""
    n_rows, nnz = ptr.numel() - 1, ind.numel()
    flat = assign.reshape(-1).long()
    assert (sp.r, sp.n_rows, sp.n_src, sp.nnz, sp.n_groups) == (r, n_rows, n_src, nnz, flat.numel() // r)
    assert sp.rows.dtype == torch.int32 and torch.equal(sp.rows.long(), flat)
    goff, src, eid = sp.goff.long(), sp.src.long(), sp.eid.long()
    assert goff.numel() == sp.n_groups + 1 and int(goff[0]) == 0 and int(goff[-1]) == nnz and bool((goff[1:] >= goff[:-1]).all())
    assert torch.equal(torch.sort(eid).values, torch.arange(nnz)), "not a permutation of the edges"
    group = torch.repeat_interleave(torch.arange(sp.n_groups), goff[1:] - goff[:-1])
    col, local = src & MASK, src >> 24
    assert nnz == 0 or (int(local.min()) >= 0 and int(local.max()) < r)
    row = flat[group * r + local]
    assert bool((row >= 0).all()), "an edge of a pad slot"
    # the word names the edge that eid names, and the row that owns it
    inv = torch.empty(nnz, dtype=torch.long)
    inv[eid_of_edge.long()] = torch.arange(nnz)
    at = inv[eid]  # the edge's position in (ptr, ind)
    assert torch.equal(col, ind.long()[at])
    owner = torch.repeat_interleave(torch.arange(n_rows), (ptr[1:] - ptr[:-1]).long())
    assert torch.equal(row, owner[at])
    # groups hold exactly the edges of their rows
    deg = (ptr[1:] - ptr[:-1]).long()
    per_group = torch.where(flat >= 0, deg[flat.clamp(min=0)], torch.zeros_like(flat)).view(-1, r).sum(1)
    assert torch.equal(goff[1:] - goff[:-1], per_group)
    # inside a group the merge key never decreases
    same = group[1:] == group[:-1]
    k = key.long()[at]
    assert bool((k[1:] >= k[:-1])[same].all())
    # every row sees its own edges in exactly its own order (duplicate pairs included: positions tell them apart)
    by_row = torch.sort(row, stable=True).indices
    assert torch.equal(at[by_row], torch.arange(nnz))


def _running_max(rowptr, colind):
    out = colind.long().clone()
    for a, b in zip(rowptr[:-1].tolist(), rowptr[1:].tolist()):
        if b > a:
            out[a:b] = torch.cummax(colind[a:b].long(), 0).values
    return out


def _shuffled(n_rows, r, seed, extra_groups=0):
    """Any assignment: a random permutation of the rows cut into groups, the pads spread over several groups."""
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


# ----------------------------------------------------------------------------------------------------------- the assignment
@pytest.mark.parametrize("n_rows,r", [(1, 1), (1, R), (R - 1, R), (R, R), (R + 1, R), (4 * R + 5, R), (301, 5), (301, 33), (7, 1)])
def test_degree_deal_is_a_partition_with_trailing_pads(n_rows, r):
    g = synth.random_csr(n_rows, 90, 6, seed=n_rows + r)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    for key in (None, g.colind):
        a = sweepplan.deal_by_degree(g.rowptr, r, key)
        _check_assignment(a, n_rows, r)
        assert torch.equal(sweepplan.checked_assignment(a, n_rows, r), a.reshape(-1))
        # the longest rows come first inside a group (they are its register rows)
        d = torch.where(a >= 0, deg[a.clamp(min=0)], torch.full_like(a, -1))
        assert bool((d[:, 1:] <= d[:, :-1]).all())


def test_degree_deal_orders_equal_rows_by_their_mean_key():
    """Six rows of two edges, three groups of two: dealt 0 1 2 then back 2 1 0 in ascending order of the mean key, so every group
    gets one early-walking and one late-walking row; without a key the rows keep their order."""
    ptr = torch.arange(0, 13, 2)
    key = torch.tensor([50, 52, 10, 12, 30, 32, 0, 2, 20, 22, 40, 42])  # means 51 11 31 1 21 41 -> rows 3 1 4 2 5 0
    assert sweepplan.deal_by_degree(ptr, 2, key).tolist() == [[3, 0], [1, 5], [4, 2]]
    assert sweepplan.deal_by_degree(ptr, 2).tolist() == [[0, 5], [1, 4], [2, 3]]


def test_degree_deal_balance_bound():
    """What the deal guarantees: max - min edges per group <= the largest row.  (Between two groups the differences of the
    rounds alternate in sign, and each sign's sum telescopes over the sorted degrees.)  Consecutive groups of the same graph are
    spread several times wider."""
    g = synth.scaled(3000, 10, seed=1)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    run = _running_max(g.rowptr, g.colind)
    for r in (7, 42, R):
        a = sweepplan.deal_by_degree(g.rowptr, r, run)
        per_group = torch.where(a >= 0, deg[a.clamp(min=0)], torch.zeros_like(a)).sum(1)
        assert int(per_group.max() - per_group.min()) <= int(deg.max())
    sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, 42)
    cons = (sp.goff[1:-1] - sp.goff[:-2]).long()  # (without the partial last group)
    assert int(cons.max() - cons.min()) > 2 * int(deg.max())


def test_checked_assignment_refuses_what_is_not_a_partition():
    ok = torch.tensor([[2, 0, -1], [1, 3, 4]])
    assert torch.equal(sweepplan.checked_assignment(ok, 5, 3), ok.reshape(-1))
    for bad in ([[2, 0, -1], [1, 3, 5]],      # names row 5 of 5
                [[2, 0, -1], [1, 3, 3]],      # row 3 twice, row 4 never
                [[2, -1, 0], [1, 3, 4]],      # a pad in front of a row
                [[2, 0, -1], [1, 3, -1]],     # row 4 never
                [[2, 0, 1, 3, 4]]):           # not groups of 3
        with pytest.raises(_lib.BackendError):
            sweepplan.checked_assignment(torch.tensor(bad), 5, 3)
    g = synth.random_csr(5, 5, 2, seed=0)
    with pytest.raises(_lib.BackendError):
        sweepplan.build_forward(g.rowptr, g.colind, 5, 3, torch.tensor([[2, 0, -1], [1, 3, 5]]))


# --------------------------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("n_rows,r", [(1, R), (R + 1, R), (4 * R + 5, R), (211, 1), (211, 5), (211, 33)])
def test_backward_layout_over_an_assignment(n_rows, r):
    """Rows of A^T = columns of A; rectangular (37 gathered rows: n_src != n_rows), ragged, empty rows on both sides, duplicate
    pairs; n_rows no multiple of r.  The degree deal and an arbitrary assignment with pads in several groups."""
    g = synth.random_csr(37, n_rows, 5, seed=n_rows)
    colptr, rowind, perm = _transpose(g)
    for assign in (sweepplan.deal_by_degree(colptr, r), _shuffled(n_rows, r, seed=r, extra_groups=1)):
        sp = sweepplan.build(colptr, rowind, perm, g.num_nodes, r, assign)
        _check_layout(sp, colptr, rowind, perm, g.num_nodes, r, assign, rowind)
    # the procedure itself: the builder hands it the merge key
    sp = sweepplan.build(colptr, rowind, perm, g.num_nodes, r, sweepplan.deal_by_degree)
    _check_layout(sp, colptr, rowind, perm, g.num_nodes, r, sweepplan.deal_by_degree(colptr, r, rowind), rowind)


@pytest.mark.parametrize("m,r", [(1, R), (R + 1, R), (4 * R + 5, R), (211, 1), (211, 5), (211, 33)])
def test_forward_layout_over_an_assignment(m, r):
    """The caller's own rows: columns in any order inside a row, duplicates, empty rows, n_src != m."""
    g = synth.random_csr(m, 53, 6, seed=m + 1)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    assert m < 10 or (int(deg.min()) == 0 and bool((g.colind[1:] < g.colind[:-1]).any()))
    run = _running_max(g.rowptr, g.colind)
    for assign in (sweepplan.deal_by_degree(g.rowptr, r), _shuffled(m, r, seed=r)):
        sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, r, assign)
        _check_layout(sp, g.rowptr, g.colind, torch.arange(g.nnz), g.n_cols, r, assign, run)
    sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, r, sweepplan.deal_by_degree)
    _check_layout(sp, g.rowptr, g.colind, torch.arange(g.nnz), g.n_cols, r, sweepplan.deal_by_degree(g.rowptr, r, run), run)
    plain = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, r)
    assert plain.rows is None and sp.out_of_order == plain.out_of_order and sp.long_rows == plain.long_rows


def test_duplicate_pairs_and_shared_sources_keep_their_order():
    """Three copies of one (row, col) pair; two rows of a group naming one source; rows 0 and 2 share a group, row 1 is alone."""
    rowptr = torch.tensor([0, 4, 6, 9], dtype=torch.int32)
    colind = torch.tensor([1, 0, 1, 1, 1, 0, 1, 1, 0], dtype=torch.int32)
    assign = torch.tensor([[2, 0], [1, -1]])
    sp = sweepplan.build_forward(rowptr, colind, 2, 2, assign)
    _check_layout(sp, rowptr, colind, torch.arange(9), 2, 2, assign, _running_max(rowptr, colind))
    # group 0: keys (running maxima) 1 1 1 1 of row 0 and 1 1 1 of row 2, ties in the structure's edge order; then group 1
    assert sp.eid.tolist() == [0, 1, 2, 3, 6, 7, 8, 4, 5]
    assert (sp.src.long() >> 24).tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0] and sp.goff.tolist() == [0, 7, 9]


def test_consecutive_assignment_gives_the_consecutive_layout():
    g = synth.random_csr(4 * R + 5, 150, 6, seed=9)
    n = g.num_nodes
    a = torch.full(((n + R - 1) // R * R,), -1, dtype=torch.long)
    a[:n] = torch.arange(n)
    plain, mapped = (sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, R, x) for x in (None, a))
    assert plain.rows is None and mapped.rows is not None
    for name in ("goff", "src", "eid"):
        assert torch.equal(getattr(plain, name), getattr(mapped, name)), name
    assert mapped.nbytes() == plain.nbytes()  # (the map is not counted: sweepplan.SweepPlan.nbytes)


# ------------------------------------------------------------------------------------------------------------ the simulator
def _sim():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "exp", "sweep_hit_sim.py")
    spec = importlib.util.spec_from_file_location("sweep_hit_sim", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_simulator_rates_the_deal_above_consecutive_groups():
    """A 20k-row uniform graph, its transpose, one round of 4096 waves (r = 5); caches of the table's share that 4 MiB are of the
    benchmark's table (4.8 %: 968 rows) and of half and 1.5 times that.  Also: the simulator's own deal is sweepplan's, and no
    cache beats the one that never evicts."""
    sim = _sim()
    g = synth.scaled(20_000, 14, seed=0)
    ptr, ind = sim.transpose(g.rowptr.numpy().astype(np.int64), g.colind.numpy().astype(np.int64), g.n_cols)
    r = 5
    deal = sim.deal_by_degree(ptr, r, sim.merge_key(ptr, ind))
    assert np.array_equal(deal, sweepplan.deal_by_degree(torch.from_numpy(ptr), r, torch.from_numpy(ind)).numpy())
    assert np.array_equal(sim.deal_by_degree(ptr, r), sweepplan.deal_by_degree(torch.from_numpy(ptr), r).numpy())
    caps = (484, 968, 1452)
    res = {}
    for name, assign in (("consecutive", sim.consecutive(len(ptr) - 1, r)), ("deal", deal)):
        goff, gathered = sim.layout(ptr, ind, assign)
        assert goff[-1] == len(ind) and np.array_equal(np.sort(gathered), np.sort(ind))
        res[name] = sim.simulate(goff, gathered, n_waves=4096, capacities=caps)
        assert all(res[name][c] <= res[name]["ideal"] + 1e-12 for c in caps)
        assert res[name][caps[0]] <= res[name][caps[1]] <= res[name][caps[2]]
    for c in caps:
        assert res["deal"][c] > res["consecutive"][c], (c, res)


def test_simulator_on_a_sequence_worked_by_hand():
    """Two waves of one XCD in lockstep, a cache of one row: wave 0 walks rows 0 1 2, wave 1 walks 0 1 -> the sequence is
    0 0 1 1 2: two hits of five; four distinct (XCD, row)... three distinct rows: ideal 2 / 5."""
    sim = _sim()
    res = sim.simulate(np.array([0, 3, 5]), np.array([0, 1, 2, 0, 1]), n_waves=4096, capacities=(1,))
    assert res["gathers"] == 5 and res[1] == 2 / 5 and res["ideal"] == 2 / 5
    # the same groups on one wave, one after the other (two rounds): 0 1 2 0 1 -> no hit with one row, ideal unchanged
    res = sim.simulate(np.array([0, 3, 5]), np.array([0, 1, 2, 0, 1]), n_waves=1, capacities=(1, 3))
    assert res[1] == 0.0 and res[3] == 2 / 5 and res["ideal"] == 2 / 5
