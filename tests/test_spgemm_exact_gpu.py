"""spgemm forward and coalesce held to the sentence in csrc/spgemm.hip: "every output value is the sum of its products in
expansion order ... the same bits ... whichever path a row takes", for canonical and non-canonical A and B.

Every case asserts (1) from ub() on the CPU that its rows take the paths it is about, (2) the pattern of the reference,
(3) valC == ref32 elementwise with NO tolerance (numerically, so -0.0 == 0.0), ref32 being the float32 sum in expansion order
(tests/_spgemm_cases.py; tests/test_spgemm_reference_cpu.py shows that reversing the order changes 31 % .. 85 % of the entries
with three or more products on the random cases), and (4) on the same pattern with values in {-4 .. 4}, valC == ref64.

Reached here and not in tests/test_spgemm_gpu.py: ub exactly at, below and above every bin boundary; A rows of more than one
chunk of THREADS entries inside each LDS bin, with empty rows of B first and last in a chunk and as a whole trailing chunk;
more rows in one bin than launch_rows has workgroups (65,536), so a workgroup reuses its LDS for a second, shorter row; more
hub rows than the 4096 workgroups of spgemm_expand_kernel / spgemm_hub_copy_kernel; duplicates and unsorted columns fed
straight to spgemm; a cancelling run on every path; column ids up to 2^31 - 2.
Not reached: the hub path with n near 2^31 (its two transposes allocate n + 1 column pointers: 8 GB); spgemm_bin_kernel's own
stride (more than 1,048,576 rows); nnz(C) beyond int32 (refused: tests/test_abi.py).
"""
import numpy as np
import pytest
import torch

import _spgemm_cases as C
from cogdl_amd.operators.spgemm import coalesce, spgemm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(A, B, n):
    rC, cC, vC = spgemm(*C.to_device(A, DEV), *C.to_device(B, DEV), n)
    return rC, cC, vC


def _compare(X, Y, n, ref):
    """spgemm(X, Y) against the canonical CSR `ref` (values float32, or float64 for integer data), on the device."""
    rC, cC, vC = _run(X, Y, n)
    assert rC.dtype == torch.int32 and cC.dtype == torch.int32 and vC.dtype == torch.float32
    assert torch.equal(rC, torch.from_numpy(ref[0].astype(np.int32)).to(DEV)), "row pointers differ"
    assert torch.equal(cC, torch.from_numpy(ref[1].astype(np.int32)).to(DEV)), "pattern differs"
    exp = torch.from_numpy(ref[2]).to(DEV)
    wrong = int((vC.to(exp.dtype) != exp).sum())
    assert wrong == 0, "%d of %d values differ from the %s reference" % (wrong, vC.numel(), ref[2].dtype)
    return rC, cC, vC


def _exact(A, B, n):
    """Against ref32, and the same pattern with integer values against ref64."""
    Ai, Bi = C.ints(A, 1), C.ints(B, 2)
    _compare(Ai, Bi, n, C.ref64(Ai, Bi, n)[:3])
    return _compare(A, B, n, C.ref32(A, B, n))


def _exact_tiled(A, B, n, m):
    """The pattern A tiled to m rows: the reference of the patterns, tiled, is the reference of the product."""
    Ai, Bi = C.ints(A, 1), C.ints(B, 2)
    _compare(C.tile(Ai, m), Bi, n, C.tile(C.ref64(Ai, Bi, n)[:3], m))
    _compare(C.tile(A, m), B, n, C.tile(C.ref32(A, B, n), m))


@pytest.mark.parametrize("shape", C.RECTANGULAR, ids=lambda s: "%dx%dx%d" % s[:3])
def test_random_rectangular_exact(shape):
    _exact(*C.rectangular(*shape))


def test_every_bin_and_the_global_path_exact():
    A, B, n = C.every_bin()
    assert set(C.bin_of(C.ub(A, B))) == {0, 1, 2, 3}
    _exact(A, B, n)


def test_hub_row_exact():
    A, B, n = C.hub_row()
    u = C.ub(A, B)
    assert u[17] > 100 * 4096 and (C.bin_of(u) == 3).all()  # ~15 entries x ~2000: every row takes the global-memory path
    _exact(A, B, n)


def test_bin_boundaries():
    """ub = 1, 2, 255 .. 257, 1023 .. 1025, 4095 .. 4098: all products in one column, in distinct columns (row_nnz == ub),
    and mixed; the first and the last row of A empty."""
    A, B, n, claims = C.boundary_case()
    u = C.ub(A, B)
    assert [int(u[r]) for r, _, _ in claims] == [w for _, w, _ in claims] and u[0] == 0 and u[-1] == 0
    rC, _, _ = _exact(A, B, n)
    nnz = (rC[1:] - rC[:-1]).cpu().numpy()
    for row, want, kind in claims:
        if kind != "mixed":
            assert nnz[row] == (1 if kind == "one" else want)
    assert nnz[0] == 0 and nnz[-1] == 0


def test_more_than_one_chunk_per_row_in_every_lds_bin():
    """A rows of 65 / 128 / 129, 257 / 513 and 513 / 1025 entries in the bins of 64, 256 and 512 threads; the rows of B have
    0 .. 3 entries, with empty ones first and last in every chunk ('edges') and as the whole last chunk ('trail')."""
    A, B, n, claims = C.chunk_case()
    u, la = C.ub(A, B), np.diff(A[0])
    for row, entries, b, _, _ in claims:
        assert la[row] == entries > C.THREADS[b] and C.bin_of(u[row]) == b
    _exact(A, B, n)


@pytest.mark.parametrize("b", [0, 1, 2])
def test_a_workgroup_takes_a_second_row(b):
    """66,037 rows, all in bin b: 501 workgroups of the 65,536 go on to a second row, among them (with the bin's list in
    row order) the row of ub = CAP followed by the row of the bin's smallest ub.  53 row patterns tiled: the reference of
    the patterns, tiled, is the reference of the product."""
    A, B, n, m, _ = C.multirow_case(b)
    At = C.tile(A, m)
    assert ((C.bin_of(C.ub(At, B)) == b).sum() == m) and m > 65536
    _exact_tiled(A, B, n, m)


def test_more_hub_rows_than_hub_workgroups():
    """4,121 rows of ub in (4096, 4800): spgemm_expand_kernel and spgemm_hub_copy_kernel (4096 workgroups) stride on."""
    A, B, n, m = C.hub_stride_case()
    At = C.tile(A, m)
    assert (C.ub(At, B) > 4096).all() and m > 4096
    _exact_tiled(A, B, n, m)


@pytest.mark.parametrize("which", ["A", "B", "AB"])
def test_noncanonical_operands_on_every_path(which):
    """Duplicate entries and unsorted columns in A, in B, in both, given to spgemm as they are."""
    A, B, n = C.noncanonical_case(which)
    assert list(C.bin_of(C.ub(A, B))) == [0, 1, -1, 2, 3]
    _exact(A, B, n)


def test_structural_zero_on_every_path():
    """x y + (-x) y in column n - 1 of a row of each path: the entry stays and is 0.0."""
    A, B, n = C.zero_case()
    assert list(C.bin_of(C.ub(A, B))) == [0, 1, 2, 3]
    for X, Y in ((A, B), (C.ints(A, 1), C.ints(B, 2))):
        if X is not A:  # keep the cancelling pair in the integer variant
            X[2][X[0][:-1] + 1] = -X[2][X[0][:-1]]
            Y[2][Y[0][2] - 1] = Y[2][Y[0][1] - 1]
        ref = C.ref32(X, Y, n)
        rC, cC, vC = _run(X, Y, n)
        assert torch.equal(rC.cpu(), torch.from_numpy(ref[0].astype(np.int32)))
        assert torch.equal(cC.cpu(), torch.from_numpy(ref[1].astype(np.int32)))
        assert bool((vC.cpu() == torch.from_numpy(ref[2])).all())
        last = (rC[1:] - 1).long()
        assert cC[last].tolist() == [n - 1] * 4 and vC[last].tolist() == [0.0] * 4


def test_column_ids_up_to_2_pow_31():
    """n = 2^31 - 1 with columns 0, 1, 2^30, 2^31 - 3, 2^31 - 2 in the 64-bit sort key and the multiplicative hash of
    the LDS bins.  The hub path is not reached: its transposes allocate n + 1 column pointers."""
    A, B, n = C.bigcol_case()
    assert n == 2 ** 31 - 1 and set(C.bin_of(C.ub(A, B))) == {0, 1, 2} and B[1].max() == n - 1
    _, cC, _ = _exact(A, B, n)
    assert set(C.BIG_SPECIAL) <= set(cC.cpu().tolist())


# ---- coalesce ----------------------------------------------------------------------------------------------------------
def _coalesce_exact(row, col, val, m, n, index_dtype):
    for v in (val, np.random.default_rng(7).integers(-4, 5, len(val)).astype(np.float32)):
        integer = v is not val
        want = C.coalesce_ref(row, col, v, m, n, np.float64 if integer else np.float32)
        acc = np.zeros(len(want[1]), dtype=np.float32)
        np.add.at(acc, want[3], v)  # the duplicates in input order
        assert np.array_equal(acc, want[2].astype(np.float32))
        got = coalesce(torch.from_numpy(row).to(index_dtype).to(DEV), torch.from_numpy(col).to(index_dtype).to(DEV),
                       torch.from_numpy(v).to(DEV), m, n, return_map=True)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
        assert np.array_equal(got[2].cpu().numpy().astype(want[2].dtype), want[2])
        assert np.array_equal(got[3].cpu().numpy(), want[3])
        rows = np.repeat(np.arange(m), np.diff(want[0]))
        assert np.array_equal((rows * n + want[1])[got[3].cpu().numpy()], row * n + col)


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_coalesce_sums_duplicates_in_input_order(index_dtype):
    rng = np.random.default_rng(11)
    m, n, e = 40, 70, 4000  # ~1.4 entries per cell: runs of 1 .. 7
    _coalesce_exact(rng.integers(0, m, e), rng.integers(0, n, e), rng.standard_normal(e).astype(np.float32), m, n, index_dtype)
    # every entry in one cell: one run of 3000
    _coalesce_exact(np.full(3000, 5), np.full(3000, 9), rng.standard_normal(3000).astype(np.float32), 8, 12, index_dtype)
    # a single entry
    _coalesce_exact(np.array([2]), np.array([3]), np.array([1.5], dtype=np.float32), 4, 5, index_dtype)
    # empty first and last rows
    e = 500
    _coalesce_exact(rng.integers(3, 17, e), rng.integers(0, 9, e), rng.standard_normal(e).astype(np.float32), 20, 9, index_dtype)
