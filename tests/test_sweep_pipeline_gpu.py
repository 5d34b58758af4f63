"""The gather ring of the sweep walk (csrc/rowsweep.h: sweep_walk): a wave keeps kSweepRing gathers in flight, waits for the
oldest alone, folds it and requests the edge kSweepRing positions ahead into the register pair it has just freed; edges are
taken in batches of 8 out of layout words held 64 at a time.  Only the time of a request moves, so every result here is
compared byte for byte with the ordinary launch on the same structure (csr_spmm_raw) and, where all values are finite, with
the CPU oracle -- through the backward layout (sweepplan.build + csr_spmm_sweep_raw) AND the forward layout
(sweepplan.build_forward + the guarded pair, hash matching).  The shapes sit on the walk's own boundaries: groups shorter than
the prologue, of exactly one, two, ... batches and of one and two 64-edge word loads, one edge either side of them, an empty
group between full ones, a wave that drains and restarts the ring between groups, register rows and LDS rows alternating
inside one batch, and a row of infinities behind a group's last edge, which the over-run requests fetch again and must never
fold."""
import numpy as np
import pytest
import torch

from cogdl_amd import _lib, plan, sweepplan, synth
from cogdl_amd.operators.spmm import csr_spmm_raw, csr_spmm_sweep_forward_raw, csr_spmm_sweep_raw
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 128
U64 = (1 << 64) - 1
N_TABLE = 300
# edges per group of r = 5 rows: every ring (4 and 8), batch (8, 16) and word-load (64, 128) boundary and one edge either side
GROUP_EDGES = [0, 1, 7, 8, 9, 15, 16, 17, 56, 57, 63, 64, 65, 71, 72, 73, 120, 127, 128, 129, 136]


def _rows():
    return int(_lib.hip().cogdl_hip_csr_spmm_sweep_group_rows())


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _table(n, seed=1):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed))


def _csr(degrees, cols, seed, n_cols=N_TABLE):
    """CSRGraph of the given row degrees and column ids, weights uniform in [0.5, 1.5)."""
    degrees = torch.as_tensor(degrees, dtype=torch.int64)
    rowptr = torch.zeros(degrees.numel() + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(degrees, 0)
    w = torch.rand(int(rowptr[-1]), generator=torch.Generator().manual_seed(seed)) + 0.5
    return synth.CSRGraph(rowptr.int(), torch.as_tensor(cols).int(), w, degrees.numel(), n_cols)


def _transposed(b):
    """The structure whose stable transpose has b's rows (columns ascending inside a row; duplicates kept)."""
    colptr, rowind, w_t, _ = oracle.csr2csc(b.rowptr, b.colind, b.weight, n_cols=b.n_cols)
    w = None if w_t is None else torch.from_numpy(np.asarray(w_t, dtype=np.float32))
    return synth.CSRGraph(torch.from_numpy(np.asarray(colptr)).int(), torch.from_numpy(np.asarray(rowind)).int(), w, b.n_cols, b.num_nodes)


def _split(total, parts, gen, cap):
    """`total` edges over `parts` rows, unevenly (empty rows included), no row above `cap`."""
    while True:
        cuts = torch.sort(torch.randint(0, total + 1, (parts - 1,), generator=gen)).values
        deg = torch.diff(torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([total])]))
        if int(deg.max()) <= cap:
            return deg.tolist()


@pytest.fixture(scope="module")
def ring_graph():
    """Consecutive groups of 5 rows holding exactly GROUP_EDGES edges; columns in random order with duplicates."""
    gen = torch.Generator().manual_seed(7)
    degrees = []
    for total in GROUP_EDGES:
        degrees += _split(total, 5, gen, cap=60)
    cols = torch.randint(0, N_TABLE, (sum(degrees),), generator=gen)
    return _csr(degrees, cols, seed=3)


class _Case:
    """One structure `b` (the rows the sweep walks), its table, and -- computed once -- the ordinary launch's and the oracle's
    product for the backward layout (rows column-sorted by the stable transpose) and the forward one (b's own edge order)."""

    def __init__(self, b, x, weighted=True):
        self.b, self.x, self.weighted = b, x, weighted
        self.xd = x.to(DEV)
        # backward: a = b^T, whose transpose plan lists b's rows
        self.a = _transposed(b)
        self.csc = plan.csr2csc(self.a.rowptr.to(DEV), self.a.colind.to(DEV), self.a.n_cols)
        self.a_w = self.a.weight.to(DEV) if weighted else None
        w_t = self.csc.transposed_values(self.a_w) if weighted else None
        self.want_bwd = csr_spmm_raw(self.csc.colptr, self.csc.rowind, w_t, self.xd, split_long_rows=False)
        # forward: b itself
        self.rowptr, self.colind = b.rowptr.to(DEV), b.colind.to(DEV)
        self.b_w = b.weight.to(DEV) if weighted else None
        self.want_fwd = csr_spmm_raw(self.rowptr, self.colind, self.b_w, self.xd)
        fp = plan.Fingerprint(self.rowptr, self.colind, b.n_cols, dev_parts=True)
        self.parts, self.hash = fp.dev, fp.key()[4] & U64

    def oracle_bwd(self):
        colptr, rowind, w_t, _ = oracle.csr2csc(self.a.rowptr, self.a.colind, self.a.weight if self.weighted else None, n_cols=self.a.n_cols)
        return oracle.csr_spmm(colptr, rowind, w_t if self.weighted else None, self.x)

    def oracle_fwd(self):
        return oracle.csr_spmm(self.b.rowptr, self.b.colind, self.b.weight if self.weighted else None, self.x)

    def backward(self, r):
        self.csc.sweep = sweepplan.build(self.csc.colptr, self.csc.rowind, self.csc.perm, self.csc.m, r)
        return self.csc.sweep, csr_spmm_sweep_raw(self.csc, self.a_w, self.xd)

    def forward(self, r, hash_delta=0):
        sp = sweepplan.build_forward(self.rowptr, self.colind, self.b.n_cols, r)
        sp.hash = (self.hash + hash_delta) & U64
        return sp, csr_spmm_sweep_forward_raw(sp, self.parts, self.rowptr, self.colind, self.b_w, self.xd)


@pytest.fixture(scope="module")
def ring_case(ring_graph):
    assert int(ring_graph.degrees().max()) <= _lib.hip().cogdl_hip_exact_row_edges(ring_graph.nnz)
    return _Case(ring_graph, _table(N_TABLE))


def _group_edges(sp):
    return torch.diff(sp.goff.cpu().long()).tolist()


def _check_both(case, r, oracle_too=True):
    sp_b, got_b = case.backward(r)
    sp_f, got_f = case.forward(r)
    assert got_b.shape == case.want_bwd.shape and got_f.shape == case.want_fwd.shape
    assert _bytes(got_b) == _bytes(case.want_bwd), "backward layout != ordinary launch"
    assert _bytes(got_f) == _bytes(case.want_fwd), "forward layout != ordinary launch"
    if oracle_too:
        assert _bytes(got_b) == case.oracle_bwd().tobytes(), "backward layout != oracle"
        assert _bytes(got_f) == case.oracle_fwd().tobytes(), "forward layout != oracle"
    return sp_b, sp_f


def test_every_ring_and_batch_boundary(ring_case):
    sp_b, sp_f = _check_both(ring_case, 5)
    assert _group_edges(sp_b) == GROUP_EDGES and _group_edges(sp_f) == GROUP_EDGES


def test_one_wave_round_drains_and_restarts_the_ring(ring_case):
    """One round capped to a single wave (tuning key 18): one workgroup, whose waves each walk several groups in turn."""
    lib = _lib.hip()
    lib.cogdl_hip_set_tuning(18, _rows())
    try:
        assert lib.cogdl_hip_csr_spmm_sweep_round_rows(F, 0) == _rows()
        sp_b, sp_f = _check_both(ring_case, 5)
    finally:
        lib.cogdl_hip_set_tuning(18, 0)
    assert _group_edges(sp_b) == GROUP_EDGES and _group_edges(sp_f) == GROUP_EDGES


def test_hash_mismatch_returns_the_ordinary_launch(ring_case):
    """The layout names ANOTHER structure's edges (columns shifted by one) under a hash the call does not match: the sweep stands
    down and the result is the ordinary launch over what the call passed -- and with the hash matching, the layout's product."""
    other = ((ring_case.colind.long() + 1) % N_TABLE).int()
    sp = sweepplan.build_forward(ring_case.rowptr, other, N_TABLE, 5)
    sp.hash = (ring_case.hash + 1) & U64
    got = csr_spmm_sweep_forward_raw(sp, ring_case.parts, ring_case.rowptr, ring_case.colind, ring_case.b_w, ring_case.xd)
    assert _bytes(got) == _bytes(ring_case.want_fwd)
    sp.hash = ring_case.hash
    got = csr_spmm_sweep_forward_raw(sp, ring_case.parts, ring_case.rowptr, ring_case.colind, ring_case.b_w, ring_case.xd)
    assert _bytes(got) == _bytes(csr_spmm_raw(ring_case.rowptr, other, ring_case.b_w, ring_case.xd)) != _bytes(ring_case.want_fwd)


@pytest.mark.parametrize("weighted", [True, False])
def test_register_and_lds_rows_alternate_inside_a_batch(weighted):
    """Groups of r = 48 rows in which local rows 31 (the last register row), 32 and 47 (the first and last LDS rows) own columns
    0, 1, 2 mod 3: in the merged order their edges follow one another, 31, 32, 47, 31, ...; every other row holds a few edges."""
    R = _rows()
    assert R == 48
    gen = torch.Generator().manual_seed(13)
    m = 2 * R + 7
    degrees, cols = [], []
    for row in range(m):
        local = row % R
        if row < 2 * R and local in (31, 32, 47):
            phase = (31, 32, 47).index(local)
            c = torch.arange(phase, 3 * 30, 3)  # ascending: the forward's running maximum is the column itself
        else:
            c = torch.sort(torch.randint(90, N_TABLE, (int(torch.randint(0, 5, (1,), generator=gen)),), generator=gen)).values
        degrees.append(c.numel())
        cols.append(c)
    case = _Case(_csr(degrees, torch.cat(cols), seed=5), _table(N_TABLE, seed=2), weighted)
    sp_b, sp_f = _check_both(case, R)
    for sp in (sp_b, sp_f):
        local = (sp.src.cpu().long() >> sweepplan.LOCAL_SHIFT)[:90].tolist()
        assert local == [31, 32, 47] * 30


def test_infinite_row_behind_a_groups_last_edge():
    """The source row of every group's last edge holds +inf (no other edge names it) and the rows no edge names hold NaN.  The
    requests past a group's end fetch that last row again; folding one of them (0 * inf) or any stray row would put a NaN into
    a row that must stay finite.  Group sizes leave 5, 3, 7, 0, 1 and 4 slots of the last batch past the end."""
    gen = torch.Generator().manual_seed(17)
    sizes = [3, 13, 17, 24, 71, 132]
    degrees, cols, owners = [], [], []
    for g, total in enumerate(sizes):
        deg = _split(total, 5, gen, cap=60)
        last_row = max(i for i in range(5) if deg[i] > 0)
        for i in range(5):
            c = torch.randint(0, 200, (deg[i],), generator=gen)
            if i == last_row:
                c[-1] = 250 + g  # the group's largest column, the row's last edge: last in both layouts
                owners.append(5 * g + i)
            cols.append(c)
        degrees += deg
    cols = torch.cat(cols)
    x = _table(N_TABLE, seed=4)
    named = torch.zeros(N_TABLE, dtype=torch.bool)
    named[cols] = True
    x[~named] = float("nan")
    x[250:250 + len(sizes)] = float("inf")
    assert int((~named).sum()) >= 50
    case = _Case(_csr(degrees, cols, seed=6), x)
    sp_b, got_b = case.backward(5)
    sp_f, got_f = case.forward(5)
    for sp in (sp_b, sp_f):
        assert _group_edges(sp) == sizes
        last = (sp.src.cpu().long() & 0xFFFFFF)[sp.goff.cpu().long()[1:] - 1].tolist()
        assert last == [250 + g for g in range(len(sizes))]
    others = torch.ones(len(degrees), dtype=torch.bool)
    others[owners] = False
    for got, want, ref in ((got_b, case.want_bwd, case.oracle_bwd()), (got_f, case.want_fwd, case.oracle_fwd())):
        got = got.cpu()
        assert bool(torch.isfinite(got[others]).all())
        assert got[others].numpy().tobytes() == np.asarray(ref)[others.numpy()].tobytes(), "a finite row != oracle"
        assert got[~others].numpy().tobytes() == want.cpu()[~others].numpy().tobytes(), "an owner row != ordinary launch"
        assert bool(torch.isinf(got[~others]).all())
