"""The FORWARD sweep layout (cogdl_amd/sweepplan.py: build_forward), the cache it lives in and the policy that lets a forward
call of csr_spmm speculate on it (cogdl_amd/xcdplan.py: spmm_forward_sweep) -- host logic only, the builder is torch code and
runs on CPU tensors.  What the layout must guarantee for bit-identical sums whatever the column order of the caller's rows: it is
a permutation of the edges, and the subsequence of every row's edges is exactly the row's own CSR order; what makes it a sweep:
inside a group the merge key -- the running maximum of the column inside the row -- never decreases.  Expected policy values are
written out from the rule list in DESIGN.md section 5 ("Forward sweep"), not computed with the code under test."""
import types

import pytest
import torch

from cogdl_amd import plan, sweepplan, synth, xcdplan

R = 48  # (csrc/rowsweep.h: kSweepRows; the CPU tests do not ask the library)
MASK = (1 << 24) - 1


def _running_max(g):
    """Per edge, the largest column among the row's edges up to and including it -- a plain loop over the rows."""
    out = torch.empty(g.nnz, dtype=torch.long)
    rp, col = g.rowptr.tolist(), g.colind.tolist()
    for i in range(g.num_nodes):
        top = -1
        for e in range(rp[i], rp[i + 1]):
            top = max(top, col[e])
            out[e] = top
    return out


def _check(sp, g, r):
    m, nnz, n_src = g.num_nodes, g.nnz, g.n_cols
    assert (sp.r, sp.n_rows, sp.n_src, sp.nnz) == (r, m, n_src, nnz)
    assert sp.n_groups == (m + r - 1) // r and sp.goff.numel() == sp.n_groups + 1
    goff, src, eid = sp.goff.long(), sp.src.long(), sp.eid.long()
    # goff matches rowptr at the group boundaries
    assert torch.equal(goff, g.rowptr.long()[torch.clamp(torch.arange(sp.n_groups + 1) * r, max=m)])
    assert int(goff[0]) == 0 and int(goff[-1]) == nnz
    assert torch.equal(torch.sort(eid).values, torch.arange(nnz))  # a permutation of the edges
    group = torch.repeat_interleave(torch.arange(sp.n_groups), goff[1:] - goff[:-1])
    col, local = src & MASK, src >> 24
    assert nnz == 0 or (int(local.min()) >= 0 and int(local.max()) < r and int(col.max()) < n_src)
    row = group * r + local
    # the packed word names the edge eid names
    assert torch.equal(col, g.colind.long()[eid])
    assert torch.equal(row, torch.repeat_interleave(torch.arange(m), g.degrees())[eid])
    # within each row the layout lists the row's eids in ascending order: exactly the row's CSR order
    by_row = torch.sort(row, stable=True).indices
    assert torch.equal(eid[by_row], torch.arange(nnz))
    # inside a group the keys do not decrease
    run = _running_max(g)
    key = run[eid]
    same = group[1:] == group[:-1]
    assert bool((key[1:] >= key[:-1])[same].all())
    # the out-of-order share equals a direct count
    behind = int((g.colind.long() < run).sum())
    assert sp.out_of_order == (behind / nnz if nnz else 0.0)
    return behind


@pytest.mark.parametrize("r", [1, 7, 48])
@pytest.mark.parametrize("which", ["ragged", "rectangular", "self loops"])
def test_forward_layout(which, r):
    if which == "ragged":  # random column order, duplicates, empty rows
        g = synth.random_csr(4 * R + 5, 211, 6, seed=r)
        assert int(g.degrees().min()) == 0
    elif which == "rectangular":
        g = synth.random_csr(R + 1, 37, 5, seed=r + 1)
    else:  # what CogDL's add_remaining_self_loops leaves: an ascending run plus one appended self loop
        g = synth.scaled(301, 6, seed=r)
    behind = _check(sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, r), g, r)
    if which == "self loops":  # at most the self loop of every row sits behind the row's running maximum
        assert 0 < behind <= g.num_nodes
    else:
        assert behind > g.nnz // 4


@pytest.mark.parametrize("m", [1, R - 1, R, R + 1])
def test_forward_layout_at_group_boundaries(m):
    g = synth.random_csr(m, 90, 5, seed=m)
    _check(sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, R), g, R)


def test_forward_layout_without_edges():
    g = synth.random_csr(20, 60, 0, seed=1)
    assert g.nnz == 0
    sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, R)
    _check(sp, g, R)
    assert sp.out_of_order == 0.0 and not sp.long_rows


def test_forward_layout_of_a_small_example():
    """Row 0 = columns 2 0 2 1 (running maximum 2 2 2 2), row 1 = 0 3 1 (0 3 3): one group merged by (running maximum,
    position), the two out-of-order edges of row 0 and the one of row 1 counted."""
    g = synth.CSRGraph(torch.tensor([0, 4, 7], dtype=torch.int32), torch.tensor([2, 0, 2, 1, 0, 3, 1], dtype=torch.int32), None, 2, 4)
    sp = sweepplan.build_forward(g.rowptr, g.colind, 4, R)
    _check(sp, g, R)
    assert sp.eid.tolist() == [4, 0, 1, 2, 3, 5, 6]
    assert (sp.src.long() & MASK).tolist() == [0, 2, 0, 2, 1, 3, 1]
    assert (sp.src.long() >> 24).tolist() == [1, 0, 0, 0, 0, 1, 1]
    assert sp.out_of_order == 3 / 7


def test_forward_layout_records_rows_beyond_the_exact_row_bound():
    from cogdl_amd import _lib

    g = synth.hub_csr(300, 250, base_deg=4, hubs=((3, 129),), seed=2)
    bound = _lib.hip().cogdl_hip_exact_row_edges(g.nnz)
    assert bound == 128
    assert sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, R).long_rows is True
    g = synth.hub_csr(300, 250, base_deg=4, hubs=((3, 128),), seed=2)
    assert _lib.hip().cogdl_hip_exact_row_edges(g.nnz) == 128
    assert sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, R).long_rows is False


def test_packed_word_limits():
    g = synth.random_csr(10, 10, 2, seed=0)
    with pytest.raises(Exception):
        sweepplan.build_forward(g.rowptr, g.colind, 1 << 24, R)
    with pytest.raises(Exception):
        sweepplan.build_forward(g.rowptr, g.colind, 10, 128)


# ------------------------------------------------------------------------------------------------------------- the cache
@pytest.fixture
def clean():
    plan.PLANS.clear()
    yield
    plan.PLANS.clear()


def _layout(seed=0, hash_=7):
    g = synth.scaled(200, 6, seed=seed)
    sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, R)
    sp.hash = hash_
    return g, sp


def test_plans_clear_empties_the_forward_cache(clean):
    g, sp = _layout()
    key = (0, g.num_nodes, g.nnz, g.n_cols, 7)
    sweepplan.FORWARD.put(key, sp)
    plan.CANDIDATES[key[:4]] = key
    assert sweepplan.candidate(key[:4]) is sp and sweepplan.FORWARD.bytes == sp.nbytes() > 0
    plan.PLANS.clear()
    assert sweepplan.candidate(key[:4]) is None
    assert len(sweepplan.FORWARD.lru) == 0 and sweepplan.FORWARD.bytes == 0 and plan.CANDIDATES == {}


@pytest.fixture
def cpu_gather(monkeypatch):
    monkeypatch.setattr(plan, "gather_rows", lambda perm, src: src[perm.long()])  # (the HIP gather has no CPU path)


def test_forward_layout_is_not_counted_in_the_plan_cache(clean, cpu_gather):
    """plan.PLANS.bytes and CscPlan.nbytes() are the transpose and the BACKWARD's layout; registering the forward's changes
    neither (tests/test_sweep_gpu.py pins their exact values)."""
    g, _ = _layout()
    t = torch.zeros(50, dtype=torch.int32)
    csc = plan.CscPlan(t, t, t, 1, 1, 50)
    plan.PLANS.lru["k"] = csc
    plan.PLANS.bytes = csc.nbytes()
    fp = types.SimpleNamespace(key=lambda: (0, g.num_nodes, g.nnz, g.n_cols, -3))
    sp = sweepplan.build_forward(g.rowptr, g.colind, g.n_cols, R)
    sweepplan.FORWARD.put(fp.key(), sp)
    w = torch.rand(g.nnz)
    w_p = sweepplan.forward_values(sp, w)
    assert torch.equal(w_p, w[sp.eid.long()]) and sweepplan.forward_values(sp, w) is w_p  # constant weights: permuted once
    assert plan.PLANS.bytes == csc.nbytes() == 600 and csc.sweep is None
    assert sweepplan.FORWARD.bytes == sp.nbytes() == 4 * (2 * g.nnz + sp.n_groups + 1) + 4 * g.nnz


def test_forward_cache_evicts_by_bytes_and_drops_the_candidate(clean):
    (g1, a), (g2, b) = _layout(1), _layout(2)
    cache = sweepplan.ForwardCache(budget_bytes=a.nbytes() + b.nbytes() - 1)
    ka, kb = (0, g1.num_nodes, g1.nnz, g1.n_cols, 1), (0, g2.num_nodes, g2.nnz, g2.n_cols, 2)
    plan.CANDIDATES[ka[:4]] = ka
    cache.put(ka, a)
    assert cache.bytes == a.nbytes()
    cache.put(kb, b)
    assert list(cache.lru) == [kb] and cache.bytes == b.nbytes() and ka[:4] not in plan.CANDIDATES
    cache.put(kb, b)  # stored again: counted once
    assert cache.bytes == b.nbytes()


def test_weights_of_a_layout_outside_the_cache_are_not_counted(cpu_gather):
    g, sp = _layout(3)
    before = sweepplan.FORWARD.bytes
    sweepplan.forward_values(sp, torch.rand(g.nnz))
    assert sweepplan.FORWARD.bytes == before


# ------------------------------------------------------------------------------------------------------------ the policy
ROUND = 4096 * R  # 256 CUs x 16 waves x 48 rows
N, NNZ = 169_343, 2_501_719


def _meta(n):
    return torch.empty(n, dtype=torch.int32, device="meta")


def _x(n=N, f=128, dtype=torch.float32):
    return torch.empty(n, f, dtype=dtype, device="meta")


def _fp(m=N, nnz=NNZ, n_src=N, dev=True):
    """A plan.Fingerprint stand-in whose hash is in flight: a wait or a key read fails the test."""
    def boom():
        raise AssertionError("the forward policy never waits for the hash")

    return types.SimpleNamespace(meta=(0, m, nnz, n_src), dev=object() if dev else None, _key=None, key=boom, wait=boom)


def _sp(m=N, nnz=NNZ, n_src=N, out_of_order=0.0628, long_rows=False, hash_=0x1234):
    e = torch.empty(0, dtype=torch.int32)
    sp = sweepplan.SweepPlan(e, e, e, 42, m, n_src, out_of_order, long_rows)
    sp.hash = hash_
    return sp


def _register(sp, m=N, nnz=NNZ, n_src=N):
    key = (0, m, nnz, n_src, 99)
    sweepplan.FORWARD.put(key, sp)
    plan.CANDIDATES[key[:4]] = key


@pytest.fixture
def auto(monkeypatch, clean):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    monkeypatch.setattr(plan, "VERIFY_HITS", False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert not plan.taping() and not plan.transient()
    yield
    plan.set_tape(None)


def _ask(fp=None, x=None, m=N, nnz=NNZ):
    return xcdplan.spmm_forward_sweep(_fp() if fp is None else fp, _meta(m + 1), _meta(nnz), _x() if x is None else x, round_rows=ROUND)


def test_policy_takes_the_headline_shape(auto):
    sp = _sp()
    _register(sp)
    assert _ask() is sp
    at_bound = _sp(out_of_order=0.125)  # the bound itself is admitted
    _register(at_bound)
    assert _ask() is at_bound
    # rectangular: 100,000 rows gathering from a table of 70,000 rows (35.8 MB); exactly one round of rows
    rect = _sp(m=100_000, nnz=800_000, n_src=70_000)
    _register(rect, 100_000, 800_000, 70_000)
    assert _ask(_fp(100_000, 800_000, 70_000), _x(70_000), 100_000, 800_000) is rect
    full = _sp(m=ROUND, nnz=NNZ, n_src=N)
    _register(full, ROUND, NNZ, N)
    assert _ask(_fp(ROUND, NNZ, N), _x(), ROUND, NNZ) is full


@pytest.mark.parametrize("what,x", [
    ("bf16", _x(dtype=torch.bfloat16)),
    ("fp16", _x(dtype=torch.float16)),
    ("F = 64", _x(f=64)),
    ("F = 256", _x(f=256)),
    ("bf16 rows of 512 bytes", _x(f=256, dtype=torch.bfloat16)),
    ("3-D operand", torch.empty(N, 2, 64, device="meta")),
])
def test_policy_declines_other_operands(auto, what, x):
    _register(_sp())
    assert _ask(x=x) is None, what


def test_policy_declines_by_size(auto):
    for m, n_src in ((60_000, 60_000), (N, (1 << 23) + 1), (ROUND + 1, N)):  # inside the eight L2s; beyond 2^23 rows; two rounds
        _register(_sp(m=m, n_src=n_src), m, NNZ, n_src)
        assert _ask(_fp(m, NNZ, n_src), _x(n_src), m, NNZ) is None, (m, n_src)
    _register(_sp(nnz=0), N, 0, N)
    assert _ask(_fp(N, 0, N), _x(), N, 0) is None  # no edges


def test_policy_needs_a_candidate_with_a_layout_for_exactly_this_meta(auto):
    assert _ask() is None                                   # nothing registered
    _register(_sp())
    assert _ask(_fp(nnz=NNZ - 1), nnz=NNZ - 1) is None      # another edge count
    assert _ask(_fp(dev=False)) is None                     # the call did not hash into device memory
    assert xcdplan.spmm_forward_sweep(None, _meta(N + 1), _meta(NNZ), _x(), round_rows=ROUND) is None  # no fingerprint at all
    assert _ask() is not None
    del sweepplan.FORWARD.lru[plan.CANDIDATES[(0, N, NNZ, N)]]  # the layout went (evicted) while the candidate entry stayed
    assert _ask() is None


def test_policy_declines_by_the_layouts_facts(auto):
    _register(_sp(long_rows=True))          # a row above the exact-row bound: the sweep reduces every row sequentially
    assert _ask() is None
    _register(_sp(out_of_order=0.1251))     # more than 1/8 of the edges behind their row's running maximum
    assert _ask() is None
    _register(_sp(out_of_order=0.78))       # rows in random column order at 14.8 edges per row
    assert _ask() is None
    _register(_sp(hash_=None))              # a layout nobody gave its structure's hash
    assert _ask() is None


@pytest.mark.parametrize("mode", ["off", "force"])
def test_policy_declines_outside_auto_mode(auto, monkeypatch, mode):
    _register(_sp())
    monkeypatch.setattr(xcdplan, "MODE", mode)
    assert _ask() is None


def test_policy_declines_transient_structures_tapes_captures_and_verify_mode(auto, monkeypatch):
    sp = _sp()
    _register(sp)
    with plan.transient_structures():
        assert _ask() is None
    assert _ask() is sp
    tape = plan.PlanTape()
    plan.set_tape(tape)
    try:
        assert _ask() is None  # recording
        tape.mode = "replay"
        assert _ask() is None
        assert tape.choices == [] and tape.cpos == 0  # (not a taped decision: a tape never speculates)
    finally:
        plan.set_tape(None)
    assert _ask() is sp
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert _ask() is None
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(plan, "VERIFY_HITS", True)
    assert _ask() is None
    monkeypatch.setattr(plan, "VERIFY_HITS", False)
    assert _ask() is sp


def test_shape_rule_the_backward_asks_before_it_builds(auto):
    assert xcdplan.spmm_forward_sweep_shape(N, NNZ, N, 128, torch.float32, round_rows=ROUND) is True
    assert xcdplan.spmm_forward_sweep_shape(70_000, 630_000, 70_000, 128, torch.float32, round_rows=ROUND) is True
    assert xcdplan.spmm_forward_sweep_shape(N, NNZ, N, 64, torch.float32, round_rows=ROUND) is False
    assert xcdplan.spmm_forward_sweep_shape(N, NNZ, N, 128, torch.bfloat16, round_rows=ROUND) is False
    assert xcdplan.spmm_forward_sweep_shape(60_000, NNZ, 60_000, 128, torch.float32, round_rows=ROUND) is False
    assert xcdplan.spmm_forward_sweep_shape(ROUND + 1, NNZ, N, 128, torch.float32, round_rows=ROUND) is False


def test_declined_layouts_keep_their_facts_not_their_edges(auto, monkeypatch):
    """register_forward on a structure in random column order: the facts stay cached (no second build), the 8 bytes per edge go,
    and the structure does not become a candidate -- calls of its shape hash as they always did."""
    monkeypatch.setattr(sweepplan, "round_rows", lambda k, dtype: ROUND)
    g = synth.random_csr(500, 400, 8, seed=5)
    fp = types.SimpleNamespace(key=lambda: (0, g.num_nodes, g.nnz, g.n_cols, 17))
    sp = sweepplan.register_forward(fp, g.rowptr, g.colind, 128, torch.float32)
    assert sp.out_of_order > 0.125 and sp.src.numel() == 0 and plan.CANDIDATES == {}
    assert sweepplan.register_forward(fp, g.rowptr, g.colind, 128, torch.float32) is sp
    g = synth.scaled(500, 8, seed=5)
    fp = types.SimpleNamespace(key=lambda: (0, g.num_nodes, g.nnz, g.n_cols, -17))
    sp = sweepplan.register_forward(fp, g.rowptr, g.colind, 128, torch.float32)
    assert sp.out_of_order <= 0.125 and sp.src.numel() == g.nnz and sp.hash == (1 << 64) - 17
    assert plan.CANDIDATES == {(0, g.num_nodes, g.nnz, g.n_cols): fp.key()} and sweepplan.candidate(fp.key()[:4]) is sp
    assert sp.r == 1  # (500 rows spread over all waves of the round)
