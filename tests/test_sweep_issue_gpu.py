"""The instruction stream of the sweep walk (csrc/rowsweep.h: sweep_walk): a batch of 8 edges whose slots all lie inside the
group runs without a test per edge and only the group's last, partial batch is tested; the layout words are read where a gather
is requested and rotate through the batch; a register row is added to in place through an indexed register; the gather is a
buffer load whose scalar offset is `word << 9`.  None of that may change a bit: every case runs both raw entries
(csr_spmm_sweep_raw, csr_spmm_sweep_forward_raw) and compares them bit for bit with the ordinary launch (csr_spmm_raw) and with
the host twin (cogdl_host_csr_spmm_f32, through spmm_cpu) -- never with the sweep itself."""
import pytest
import torch

from cogdl_amd import _lib, plan, sweepplan
from cogdl_amd.operators.spmm import csr_spmm_raw, csr_spmm_sweep_forward_raw, csr_spmm_sweep_raw, spmm_cpu
import _offset

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = 128
U64 = (1 << 64) - 1
GROUP_EDGES = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129)
RESIDUES = tuple(range(40, 48))  # every residue of the edge count mod 8, side by side


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _hashed(rowptr, colind, n_src):
    fp = plan.Fingerprint(rowptr, colind, n_src, dev_parts=True)
    return fp.dev, fp.key()[4] & U64


def _transpose_of(row, col, w, n_src):
    """The CSR structure A (n_src rows) whose stable transpose lists, for every output row, the edges (row, col, w) given -- in
    the order given inside an output row when its columns ascend."""
    order = torch.sort(col.long(), stable=True).indices
    rowptr = torch.zeros(n_src + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(col.long(), minlength=n_src), 0)
    return rowptr.int(), row[order].int(), w[order].float()


def _check(row, col, w, m, n_src, r, x, weighted=True):
    """Output row row[e] gathers table row col[e] with weight w[e] (CPU tensors); m output rows in groups of r; x the table on
    the device.  Both raw entries against the ordinary launch and the host twin."""
    a_rowptr, a_colind, a_w = _transpose_of(row, col, w, n_src)
    csc = plan.csr2csc(a_rowptr.to(DEV), a_colind.to(DEV), m)
    assert csc.m == n_src and csc.n_cols == m and x.shape == (n_src, F)
    wd = a_w.to(DEV) if weighted else None
    w_t = csc.transposed_values(wd) if weighted else None
    want = csr_spmm_raw(csc.colptr, csc.rowind, w_t, x, split_long_rows=False)
    # the host twin over the rows the structure names (a table of 2 GB and more stays on the device)
    uniq, inv = torch.unique(csc.rowind.long(), return_inverse=True)
    twin = spmm_cpu(csc.colptr.cpu(), inv.int().cpu(), None if w_t is None else w_t.cpu(), x[uniq].cpu())
    assert _bytes(want) == twin.numpy().tobytes(), "ordinary launch != host twin"
    csc.sweep = sweepplan.build(csc.colptr, csc.rowind, csc.perm, csc.m, r)
    got = csr_spmm_sweep_raw(csc, wd, x)
    assert got.shape == (m, F)
    assert _bytes(got) == _bytes(want), "sweep != ordinary launch"
    sp = sweepplan.build_forward(csc.colptr, csc.rowind, n_src, r)
    parts, sp.hash = _hashed(csc.colptr, csc.rowind, n_src)
    fwd = csr_spmm_sweep_forward_raw(sp, parts, csc.colptr, csc.rowind, w_t, x)
    assert _bytes(fwd) == _bytes(want), "guarded pair != ordinary launch"
    return csc, want


def _table(n, seed=1):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _edges_of_groups(group_edges, r, last_rows, n_src, seed):
    """Groups of r rows holding group_edges[g] edges each, spread at random over the group's rows, then a last group of
    last_rows < r rows (5 edges); columns at random (duplicates kept)."""
    gen = torch.Generator().manual_seed(seed)
    rows = []
    for g, n in enumerate(group_edges):
        rows.append(g * r + torch.randint(0, r, (n,), generator=gen))
    m = len(group_edges) * r
    if last_rows:
        rows.append(m + torch.randint(0, last_rows, (5,), generator=gen))
        m += last_rows
    row = torch.sort(torch.cat(rows)).values
    col = torch.randint(0, n_src, (row.numel(),), generator=gen)
    w = torch.randn(row.numel(), generator=gen)
    return row, col, w, m


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("r", [1, 31, 32, 33, 48])
def test_group_lengths(r, weighted):
    """Groups of 0 ... 129 edges (full batches, the tested tail, the 64-edge word turn and its neighbours), eight groups with
    every residue mod 8 next to one another, and a partial last group (r > 1).  (r = 1: a group is one row, 129 edges are
    beyond the exact-row bound of the default launch, so the ordinary launch is asked for its sequential rows.)"""
    n_src = 300
    row, col, w, m = _edges_of_groups(GROUP_EDGES + RESIDUES, r, r // 2, n_src, seed=r)
    csc, _ = _check(row, col, w, m, n_src, r, _table(n_src), weighted)
    goff = csc.sweep.goff.cpu().long()
    lengths = (goff[1:] - goff[:-1]).tolist()
    assert tuple(lengths[:len(GROUP_EDGES) + len(RESIDUES)]) == GROUP_EDGES + RESIDUES
    assert (m % r != 0) == (r > 1)


def _distinct_table(n):
    """Values distinct per row and column (exact in fp32), so that a fold into a neighbouring register changes bits."""
    return ((torch.arange(n * F, dtype=torch.float32).view(n, F) + 1.0) / 1024.0).to(DEV)


@pytest.mark.parametrize("weighted", [True, False])
def test_fold_indexing_every_local_row(weighted):
    """Two groups of 48 rows; local row i receives i + 1 edges in the first and 48 - i in the second: rows 0, 31 (the ends of the
    register tuples), 32 and 47 (the ends of the LDS slab) each with a count of their own."""
    R = int(_lib.hip().cogdl_hip_csr_spmm_sweep_group_rows())
    assert R == 48
    n_src = 500
    gen = torch.Generator().manual_seed(7)
    counts = torch.cat([torch.arange(1, R + 1), torch.arange(R, 0, -1)])
    row = torch.repeat_interleave(torch.arange(2 * R), counts)
    col = torch.randint(0, n_src, (row.numel(),), generator=gen)
    w = torch.randn(row.numel(), generator=gen)
    _check(row, col, w, 2 * R, n_src, R, _distinct_table(n_src), weighted)


@pytest.mark.parametrize("weighted", [True, False])
def test_fold_alternates_between_register_and_lds_rows(weighted):
    """Edge j of the group gathers table row j, so the walk visits the edges in this order: even edges go to register rows
    0 ... 31 in turn, odd edges to LDS rows 32 ... 47 in turn."""
    n = 333
    j = torch.arange(n)
    local = torch.where(j % 2 == 0, (j // 2) % 32, 32 + (j // 2) % 16)
    order = torch.sort(local, stable=True).indices  # (edges listed by output row; inside a row the columns ascend)
    w = torch.randn(n, generator=torch.Generator().manual_seed(9))
    csc, _ = _check(local[order], j[order], w[order], 48, n, 48, _distinct_table(n), weighted)
    walked = (csc.sweep.src.cpu().long() >> 24).tolist()
    assert walked == local.tolist()


def _few_rows_table(n_src, rows, seed):
    """A table of n_src rows on the device of which only `rows` are filled (the rest is never read)."""
    x = torch.zeros(n_src, F, device=DEV)
    idx = torch.tensor(rows, device=DEV)
    x[idx] = torch.randn(len(rows), F, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return x


@pytest.mark.parametrize("n_src,rows", [
    ((1 << 22) + 8, (0, 1, (1 << 21) + 3, (1 << 22) - 1, 1 << 22, (1 << 22) + 7)),
    (1 << 23, (0, (1 << 22) - 1, 1 << 22, (1 << 23) - 2, (1 << 23) - 1)),
])
def test_row_offsets_on_both_sides_of_2_31(n_src, rows):
    """`word << 9` as the load's scalar offset: rows whose byte offsets lie below 2^31, at 2^31 and beyond it, the table's last
    row among them.  The second table has 2^23 rows, the most the layout admits: its last row starts at byte 2^32 - 512 and
    takes the same request as every other (the descriptor's range check sees the lane's offset inside a row only)."""
    assert n_src <= sweepplan.MAX_TABLE_ROWS == 1 << 23 and rows[-1] == n_src - 1
    x = _few_rows_table(n_src, rows, seed=n_src % 1000)
    gen = torch.Generator().manual_seed(3)
    m, per_row = 100, 11
    row = torch.repeat_interleave(torch.arange(m), per_row)
    col = torch.tensor(rows)[torch.randint(0, len(rows), (m * per_row,), generator=gen)]
    w = torch.randn(m * per_row, generator=gen)
    _, want = _check(row, col, w, m, n_src, 48, x)
    assert bool((want != 0).any())


def test_the_entry_takes_2_23_rows_and_no_more():
    """The host side of that decision: a table of exactly 2^23 rows is launched like any other, one row more is declined."""
    lib = _lib.hip()
    goff = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    src = torch.zeros(1, dtype=torch.int32, device=DEV)
    x, out = _table(4), torch.empty(1, F, device=DEV)

    def launch(n_src):
        return lib.cogdl_hip_csr_spmm_sweep(_lib.ptr(goff), _lib.ptr(src), None, _lib.ptr(x), _lib.ptr(out), 1, n_src, 1, 1, F, 1, 0,
                                            _lib.stream_of(x))

    assert launch(1 << 23) == 0
    assert _bytes(out[0]) == _bytes(x[0])
    assert launch((1 << 23) + 1) != 0


def test_table_that_starts_8_bytes_into_its_allocation():
    n_src = 300
    row, col, w, m = _edges_of_groups((9, 64, 65, 3), 33, 4, n_src, seed=5)
    x, guard = _offset.shifted(_table(n_src), 2)
    assert x.data_ptr() % 16 == 8
    _check(row, col, w, m, n_src, 33, x)
    assert _offset.guards_intact(guard)


def test_guard_picks_the_side():
    """Which side ran, read off the outputs: a layout of ANOTHER structure's edges under this structure's hash gives that
    structure's product when the hash matches (the sweep ran) and this structure's when it does not (the ordinary launch ran)."""
    n_src, r = 300, 33
    row, col, w, m = _edges_of_groups((9, 64, 65, 3), r, 4, n_src, seed=5)
    x = _table(n_src)
    csc, ya = _check(row, col, w, m, n_src, r, x)
    rowptr, ca = csc.colptr, csc.rowind
    w_t = csc.transposed_values(_transpose_of(row, col, w, n_src)[2].to(DEV))
    cb = ((ca.long() + 1) % n_src).int()
    yb = csr_spmm_raw(rowptr, cb, w_t, x, split_long_rows=False)
    assert _bytes(ya) != _bytes(yb)
    sp = sweepplan.build_forward(rowptr, cb, n_src, r)
    parts_a, sp.hash = _hashed(rowptr, ca, n_src)
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts_a, rowptr, ca, w_t, x)) == _bytes(yb)
    sp.hash = (sp.hash + 1) & U64
    assert _bytes(csr_spmm_sweep_forward_raw(sp, parts_a, rowptr, ca, w_t, x)) == _bytes(ya)
