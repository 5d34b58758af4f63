"""The sweep layout of a stable transpose (cogdl_amd/sweepplan.py) and the policy that decides when the backward pass of
csr_spmm walks it (cogdl_amd/xcdplan.py: spmm_backward_sweep) -- host logic only, the builder is torch code and runs on CPU
tensors.  What the layout must guarantee for bit-identical sums: it is a permutation of the edges, gathered rows ascend inside
a group, and the subsequence of every row's edges is exactly the row's own (CSC) order.  Expected policy values are written out
from the rule list in DESIGN.md section 5 ("Sweep layout"), not computed with the code under test."""
import types

import pytest
import torch

from cogdl_amd import plan, sweepplan, synth, xcdplan

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


def _check(sp, colptr, rowind, perm, n_src, r):
    n_rows, nnz = colptr.numel() - 1, rowind.numel()
    assert (sp.r, sp.n_rows, sp.n_src, sp.nnz) == (r, n_rows, n_src, nnz)
    assert sp.n_groups == (n_rows + r - 1) // r and sp.goff.numel() == sp.n_groups + 1
    goff, src, eid = sp.goff.long(), sp.src.long(), sp.eid.long()
    # offsets: group g holds exactly the CSC range of its rows
    want_off = colptr.long()[torch.clamp(torch.arange(sp.n_groups + 1) * r, max=n_rows)]
    assert torch.equal(goff, want_off) and int(goff[0]) == 0 and int(goff[-1]) == nnz
    # a permutation of the edges (perm is one, eid = perm composed with the layout's order)
    assert torch.equal(torch.sort(eid).values, torch.arange(nnz))
    group = torch.repeat_interleave(torch.arange(sp.n_groups), goff[1:] - goff[:-1])
    col, local = src & MASK, src >> 24
    assert nnz == 0 or (int(local.min()) >= 0 and int(local.max()) < r and int(col.max()) < n_src)
    row = group * r + local
    assert nnz == 0 or int(row.max()) < n_rows
    # the packed word names the edge eid names: gathered row = rowind at that edge's CSC position
    inv = torch.empty(nnz, dtype=torch.long)
    inv[perm.long()] = torch.arange(nnz)
    assert torch.equal(col, rowind.long()[inv[eid]])
    # inside a group gathered rows ascend
    same = group[1:] == group[:-1]
    assert bool((col[1:] >= col[:-1])[same].all())
    # every row sees its own edges in exactly its CSC order (duplicate (row, col) pairs included: eid tells them apart)
    by_row = torch.sort(row, stable=True).indices
    assert torch.equal(eid[by_row], perm.long())
    assert torch.equal(row[by_row], torch.repeat_interleave(torch.arange(n_rows), (colptr[1:] - colptr[:-1]).long()))


@pytest.mark.parametrize("n_rows", [1, R - 1, R, R + 1, 4 * R + 5])
def test_layout_at_group_boundaries(n_rows):
    """Rows of A^T = columns of A: 1, R-1, R, R+1, 4R+5 of them; rectangular (37 gathered rows), ragged, with empty rows of A,
    empty rows of A^T (columns nobody names: more columns than a row's edges reach at n_rows = 4R+5) and duplicate pairs."""
    g = synth.random_csr(37, n_rows, 5, seed=n_rows)
    colptr, rowind, perm = _transpose(g)
    _check(sweepplan.build(colptr, rowind, perm, g.num_nodes, R), colptr, rowind, perm, g.num_nodes, R)


@pytest.mark.parametrize("r", [1, 7, 42])
def test_layout_with_fewer_rows_per_group(r):
    g = synth.random_csr(300, 211, 6, seed=r)
    colptr, rowind, perm = _transpose(g)
    _check(sweepplan.build(colptr, rowind, perm, g.num_nodes, r), colptr, rowind, perm, g.num_nodes, r)


def test_layout_of_a_structure_without_edges_and_with_empty_rows():
    g = synth.random_csr(20, 60, 0, seed=1)
    colptr, rowind, perm = _transpose(g)
    assert rowind.numel() == 0
    _check(sweepplan.build(colptr, rowind, perm, g.num_nodes, R), colptr, rowind, perm, g.num_nodes, R)
    g = synth.random_csr(50, 400, 1, seed=2)  # far more columns than edges: most rows of the transpose are empty
    colptr, rowind, perm = _transpose(g)
    assert int((colptr[1:] == colptr[:-1]).sum()) > 200
    _check(sweepplan.build(colptr, rowind, perm, g.num_nodes, R), colptr, rowind, perm, g.num_nodes, R)


def test_duplicate_pairs_keep_their_order():
    """Three copies of one (row, col) pair and two rows of one group naming the same source: ties keep CSC order."""
    rowptr = torch.tensor([0, 4, 6], dtype=torch.int32)
    colind = torch.tensor([1, 0, 1, 1, 1, 0], dtype=torch.int32)
    g = synth.CSRGraph(rowptr, colind, None, 2, 3)
    colptr, rowind, perm = _transpose(g)
    sp = sweepplan.build(colptr, rowind, perm, 2, R)
    _check(sp, colptr, rowind, perm, 2, R)
    # one group; merged by gathered row 0 then 1; inside a gathered row by CSC position (column 0's edge first)
    assert (sp.src.long() & MASK).tolist() == [0, 0, 0, 0, 1, 1]
    assert (sp.src.long() >> 24).tolist() == [0, 1, 1, 1, 0, 1]
    assert sp.eid.tolist() == [1, 0, 2, 3, 5, 4]


def test_packed_word_limits():
    g = synth.random_csr(10, 10, 2, seed=0)
    colptr, rowind, perm = _transpose(g)
    with pytest.raises(Exception):
        sweepplan.build(colptr, rowind, perm, 1 << 24, R)
    with pytest.raises(Exception):
        sweepplan.build(colptr, rowind, perm, 10, 128)


def test_group_rows_spreads_a_small_structure_over_all_waves():
    assert sweepplan.group_rows(169_343, 4096 * 48, 48) == 42
    assert sweepplan.group_rows(4096 * 48, 4096 * 48, 48) == 48
    assert sweepplan.group_rows(4096 * 48 + 1, 4096 * 48, 48) == 48  # (over capacity: the policy declines before)
    assert sweepplan.group_rows(100, 4096 * 48, 48) == 1
    assert sweepplan.group_rows(70_000, 4096 * 48, 48) == 18


# ---------------------------------------------------------------------------------------------------------------- the policy
ROUND = 4096 * R  # 256 CUs x 16 waves x 48 rows


def _csc(n_rows=169_343, n_src=169_343, sightings=2, hub=False, nnz=2_500_000):
    return types.SimpleNamespace(n_cols=n_rows, m=n_src, nnz=nnz, sightings=sightings, has_hub_columns=lambda: hub)


def _g(n_src=169_343, f=128, dtype=torch.float32):
    return torch.empty(n_src, f, dtype=dtype, device="meta")


@pytest.fixture
def auto(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    assert not plan.taping() and not plan.transient()
    yield
    plan.set_tape(None)


def test_policy_takes_the_headline_shape(auto):
    assert xcdplan.spmm_backward_sweep(_csc(), _g(), round_rows=ROUND) is True
    assert xcdplan.spmm_backward_sweep(_csc(sightings=3), _g(), round_rows=ROUND) is True
    # rectangular: 100,000 rows of the transpose gathering from a table of 70,000 rows (35.8 MB)
    assert xcdplan.spmm_backward_sweep(_csc(n_rows=100_000, n_src=70_000), _g(70_000), round_rows=ROUND) is True
    assert xcdplan.spmm_backward_sweep(_csc(n_rows=ROUND), _g(), round_rows=ROUND) is True  # exactly one round


@pytest.mark.parametrize("what,csc,g", [
    ("bf16", _csc(), _g(dtype=torch.bfloat16)),
    ("fp16", _csc(), _g(dtype=torch.float16)),
    ("F = 64", _csc(), _g(f=64)),
    ("F = 256", _csc(), _g(f=256)),
    ("bf16 rows of 512 bytes", _csc(), _g(f=256, dtype=torch.bfloat16)),
    ("3-D operand", _csc(), torch.empty(169_343, 2, 64, device="meta")),
    ("hub transpose", _csc(hub=True), _g()),
    ("first sighting", _csc(sightings=1), _g()),
    ("over capacity", _csc(n_rows=ROUND + 1), _g()),
    ("table inside the eight L2s", _csc(n_rows=60_000, n_src=60_000), _g(60_000)),
    ("table beyond 2^23 rows", _csc(n_src=(1 << 23) + 1), _g((1 << 23) + 1)),
    ("no edges", _csc(nnz=0), _g()),
])
def test_policy_declines(auto, what, csc, g):
    assert xcdplan.spmm_backward_sweep(csc, g, round_rows=ROUND) is False, what


@pytest.mark.parametrize("mode", ["off", "force"])
def test_policy_declines_outside_auto_mode(monkeypatch, mode):
    monkeypatch.setattr(xcdplan, "MODE", mode)
    assert xcdplan.spmm_backward_sweep(_csc(), _g(), round_rows=ROUND) is False


def test_policy_declines_transient_structures_and_tapes(auto):
    with plan.transient_structures():
        assert xcdplan.spmm_backward_sweep(_csc(), _g(), round_rows=ROUND) is False
    assert xcdplan.spmm_backward_sweep(_csc(), _g(), round_rows=ROUND) is True
    tape = plan.PlanTape()
    plan.set_tape(tape)
    try:
        assert xcdplan.spmm_backward_sweep(_csc(), _g(), round_rows=ROUND) is False  # recording
        tape.mode = "replay"
        assert xcdplan.spmm_backward_sweep(_csc(), _g(), round_rows=ROUND) is False
        assert tape.choices == [] and tape.cpos == 0  # (not a taped decision: a tape never takes the sweep)
    finally:
        plan.set_tape(None)
    assert xcdplan.spmm_backward_sweep(_csc(), _g(), round_rows=ROUND) is True


def test_hub_test_is_asked_last(auto):
    """has_hub_columns() reads back from the device once per plan: a call the other rules decline never pays it."""
    def boom():
        raise AssertionError("has_hub_columns() consulted")

    csc = _csc(sightings=1)
    csc.has_hub_columns = boom
    assert xcdplan.spmm_backward_sweep(csc, _g(), round_rows=ROUND) is False
    csc = _csc(n_rows=ROUND + 1)
    csc.has_hub_columns = boom
    assert xcdplan.spmm_backward_sweep(csc, _g(), round_rows=ROUND) is False


def test_plan_cache_counts_the_layout():
    """The layout (and its memoised weights) grow a cached plan after it was stored: PlanCache.grew keeps `bytes` equal to the
    sum of nbytes() and evicts from the cold end."""
    cache = plan.PlanCache(budget_bytes=10_000)

    def mk(n):
        t = torch.zeros(n, dtype=torch.int32)
        return plan.CscPlan(t, t, t, 1, 1, n)

    a, b = mk(100), mk(100)
    cache.lru["a"], cache.lru["b"] = a, b
    cache.bytes = a.nbytes() + b.nbytes()
    g = synth.random_csr(30, 40, 4, seed=0)
    colptr, rowind, perm = _transpose(g)
    b.sweep = sweepplan.build(colptr, rowind, perm, g.num_nodes, R)
    cache.grew(b, b.sweep.nbytes())
    assert cache.bytes == a.nbytes() + b.nbytes() and b.nbytes() == 1200 + b.sweep.nbytes()
    cache.grew(mk(5), 1 << 20)  # not a cached plan: nothing is counted
    assert cache.bytes == a.nbytes() + b.nbytes()
    cache.grew(b, 9_000)  # over budget: the cold end goes
    assert list(cache.lru) == ["b"] and cache.bytes == b.nbytes() + 9_000
