"""The references of the SpGEMM GPU tests (tests/_spgemm_cases.py) held to account on the CPU, and every case builder held
to the bins, boundaries and chunk layouts it claims: the GPU tests are only as good as these.

  (a) ref32 equals a literal triple loop over float32 scalars, bit for bit;
  (b) |ref32 - ref64| <= gamma_t sum|a b| per entry (t products: t - 1 additions and one product rounding each);
  (c) on integer data ref32 == ref64 exactly;
  (d) the order condition: with every row's products reversed, ref32 changes in at least a tenth of the entries with 3 or
      more products, on every random case of the exact comparison -- so "equal to ref32" is a test of summation order;
  (e) grad_ref equals float64 autograd of torch.sparse.mm, and coalesce_ref float64 torch coalesce.
"""
import numpy as np
import pytest
import torch

import _spgemm_cases as C


def _literal(A, B, n):
    """ref32 as the sentence reads: dictionaries and numpy float32 scalars, one rounding per operation."""
    (rA, cA, vA), (rB, cB, vB) = A, B
    rowptr, col, val = [0], [], []
    for i in range(len(rA) - 1):
        acc = {}
        for e in range(rA[i], rA[i + 1]):
            for q in range(rB[cA[e]], rB[cA[e] + 1]):
                p = np.float32(vA[e]) * np.float32(vB[q])
                acc[cB[q]] = np.float32(acc[cB[q]] + p) if cB[q] in acc else p
        for j in sorted(acc):
            col.append(j)
            val.append(acc[j])
        rowptr.append(len(col))
    return np.array(rowptr), np.array(col, dtype=np.int64), np.array(val, dtype=np.float32)


def _same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x[:2], y[:2])) and x[2].tobytes() == y[2].tobytes()


@pytest.mark.parametrize("case", ["rect", "noncanonical", "chunk-rows"])
def test_ref32_is_the_literal_loop(case):
    if case == "rect":
        A, B, n = C.rectangular(*C.RECTANGULAR[2])  # ~45 products per entry
    elif case == "noncanonical":
        A, B, n = C.noncanonical_case("AB")
    else:
        A, B, n, _ = C.chunk_case()
        A = (A[0][:4], A[1][:A[0][3]], A[2][:A[0][3]])
    assert _same(C.ref32(A, B, n), _literal(A, B, n))
    # reversed expansion = the literal loop over A and B with every row's entries reversed
    assert _same(C.ref32(A, B, n, reverse=True), _literal(*_reversed_rows(A, B), n))


def _reversed_rows(A, B):
    """A with every row's entries reversed and B with every row's entries reversed: the same products, every row's in
    the opposite order."""
    def flip(X):
        rows = [(X[1][a:b][::-1], X[2][a:b][::-1]) for a, b in zip(X[0][:-1], X[0][1:])]
        return C.csr_of_rows(rows)
    return flip(A), flip(B)


def _all_cases():
    out = list(C.random_cases())
    A, B, n, _ = C.boundary_case()
    out.append(("boundary", A, B, n))
    A, B, n, _ = C.chunk_case()
    out.append(("chunk", A, B, n))
    for which in ("A", "B", "AB"):
        out.append(("noncanonical-" + which,) + C.noncanonical_case(which))
    out.append(("zero",) + C.zero_case())
    out.append(("bigcol",) + C.bigcol_case())
    for b in range(3):
        A, B, n, _, _ = C.multirow_case(b)
        out.append(("multirow-%d" % b, A, B, n))
    out.append(("hub_stride",) + C.hub_stride_case()[:3])
    return out


@pytest.fixture(scope="module")
def cases():
    return _all_cases()


def test_ref32_within_the_classical_bound_of_ref64(cases):
    for name, A, B, n in cases:
        r32, r64 = C.ref32(A, B, n), C.ref64(A, B, n)
        assert np.array_equal(r32[0], r64[0]) and np.array_equal(r32[1], r64[1]), name
        err = np.abs(r32[2].astype(np.float64) - r64[2])
        assert (err <= C.gamma(r64[4]) * r64[3]).all(), name
        assert r64[4].sum() == C.ub(A, B).sum(), name


def test_integer_data_is_exact_in_float32(cases):
    for name, A, B, n in cases:
        Ai, Bi = C.ints(A, 1), C.ints(B, 2)
        r32, r64 = C.ref32(Ai, Bi, n), C.ref64(Ai, Bi, n)
        assert np.array_equal(r32[2].astype(np.float64), r64[2]), name
        assert np.array_equal(C.ref32(Ai, Bi, n, reverse=True)[2], r32[2]), name


def test_order_condition_on_every_random_case():
    seen = 0
    for name, A, B, n in C.random_cases():
        fwd, rev, terms = C.ref32(A, B, n)[2], C.ref32(A, B, n, reverse=True)[2], C.ref64(A, B, n)[4]
        many = terms >= 3
        differ = int(((fwd != rev) & many).sum())
        print("%s: %d of %d entries with >= 3 products differ under reversal" % (name, differ, int(many.sum())))
        assert 10 * differ >= int(many.sum()), name
        assert np.array_equal(fwd[terms == 1], rev[terms == 1]) and np.array_equal(fwd[terms == 2], rev[terms == 2]), name
        seen += int(many.sum())
    assert seen > 100000


def test_structural_zero_of_the_reference():
    A, B, n = C.zero_case()
    rowptr, col, val = C.ref32(A, B, n)
    for i in range(len(C.PATH_ENTRIES)):
        assert col[rowptr[i + 1] - 1] == n - 1 and val[rowptr[i + 1] - 1] == 0.0
    assert list(C.bin_of(C.ub(A, B))) == [0, 1, 2, 3]


# ---- the builders' claims -----------------------------------------------------------------------------------------------
def test_boundary_case_has_the_exact_ub_values():
    A, B, n, claims = C.boundary_case()
    u, nnz = C.ub(A, B), np.diff(C.ref32(A, B, n)[0])
    assert u[0] == 0 and u[-1] == 0 and len(claims) == 3 * len(C.BOUNDARY_UB) == len(u) - 2
    for row, want, kind in claims:
        assert u[row] == want
        assert nnz[row] == {"one": 1, "distinct": want}.get(kind, nnz[row])
    assert sorted(set(u[1:-1])) == sorted(C.BOUNDARY_UB)
    got = C.bin_of(u[1:-1:3])
    assert list(got) == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3]


def test_chunk_case_layout():
    A, B, n, claims = C.chunk_case()
    u = C.ub(A, B)
    lens_b = np.diff(B[0])
    assert set(lens_b) == {0, 1, 2, 3}
    assert len(claims) == len(C.CHUNK_ROWS) * len(C.CHUNK_VARIANTS)
    for row, entries, b, variant, lens in claims:
        cols = A[1][A[0][row]:A[0][row + 1]]
        t = C.THREADS[b]
        assert len(cols) == entries > t and (np.diff(cols) > 0).all()
        assert np.array_equal(lens_b[cols], lens)
        assert C.bin_of(u[row]) == b and u[row] == lens.sum()
        if variant == "edges":
            for c in range(0, entries, t):
                assert lens[c] == 0 and lens[min(c + t, entries) - 1] == 0
        if variant == "trail":
            assert lens[(entries - 1) // t * t:].sum() == 0 and lens[:(entries - 1) // t * t].sum() > 0
    assert any(v == "trail" and e == 128 for _, e, _, v, _ in claims)  # a whole trailing chunk of 64 empty rows


@pytest.mark.parametrize("b", [0, 1, 2])
def test_multirow_case_fills_one_bin_beyond_its_grid(b):
    A, B, n, m, targets = C.multirow_case(b)
    u = C.ub(A, B)
    assert np.array_equal(u, targets) and (C.bin_of(u) == b).all() and len(u) == C.P_TILE
    assert u.min() == (C.CAPS[b - 1] if b else 0) + 1 and u.max() == C.CAPS[b]
    in_bin = (C.bin_of(C.ub(C.tile(A, m), B)) == b).sum()
    assert in_bin == m > 66000 and in_bin > 65536  # launch_rows caps the grid at 65,536 workgroups
    step = 65536 % C.P_TILE
    assert u[0] == C.CAPS[b] and u[step] == u.min()  # the CAP row is followed by the shortest one in its workgroup
    if b == 0:
        assert (np.diff(A[0]) == 16).all() and 16 * m > 65536 * 16  # spgemm_grad_a_kernel's stride


def test_tile_is_the_tiled_product():
    A, B, n, _, _ = C.multirow_case(0)
    m = 2 * C.P_TILE + 7
    assert _same(C.ref32(C.tile(A, m), B, n), C.tile(C.ref32(A, B, n), m))


def test_hub_stride_case():
    A, B, n, m = C.hub_stride_case()
    u = C.ub(A, B)
    assert (u > 4096).all() and u.max() < 4800 and m > 4100
    assert 16e6 < u.mean() * m < 20e6


def test_paths_of_the_small_cases():
    for which in ("A", "B", "AB"):
        A, B, n = C.noncanonical_case(which)
        assert list(C.bin_of(C.ub(A, B))) == [0, 1, -1, 2, 3]
        for X, messy in ((A, "A" in which), (B, "B" in which)):
            for a, b in zip(X[0][:-1], X[0][1:]):
                cols = X[1][a:b]
                if messy and len(cols) >= 3:
                    assert len(set(cols)) < len(cols) and (np.diff(cols) < 0).any()
                if not messy:
                    assert (np.diff(cols) > 0).all()
    A, B, n = C.bigcol_case()
    assert n == 2 ** 31 - 1 and set(C.bin_of(C.ub(A, B))) == {0, 1, 2}
    assert set(C.BIG_SPECIAL) <= set(B[1]) and B[1].max() == 2 ** 31 - 2
    assert set(C.BIG_SPECIAL) <= set(C.ref32(A, B, n)[1])
    A, B, n = C.stride_b_case()
    assert len(B[1]) > 65536 * 16 and (C.bin_of(C.ub(A, B)) == 2).all()
    assert np.diff(B[0]).min() == 16 and A[1].max() == len(B[0]) - 2


def test_group_tail_case_lengths():
    A, B, n = C.group_tail_case()
    k = len(B[0]) - 1
    assert [int(x) for x in np.diff(B[0])] == [C.GROUP_LENGTHS_B[r % 7] for r in range(k)]
    assert [int(x) for x in np.bincount(A[1], minlength=k)] == [C.GROUP_LENGTHS_A[c % 6] for c in range(k)]
    A, B, n = C.empty_ends_case()
    for X in (A, B):
        lens = np.diff(X[0])
        assert lens[:3].sum() == 0 and lens[-3:].sum() == 0 and lens[3] > 0 and lens[-4] > 0


# ---- the gradient and coalesce references against torch in float64 --------------------------------------------------------
def _coo64(X, shape, vals):
    rows = torch.from_numpy(np.repeat(np.arange(len(X[0]) - 1), np.diff(X[0])))
    return torch.sparse_coo_tensor(torch.stack([rows, torch.from_numpy(X[1])]), vals, shape)


@pytest.mark.parametrize("builder", [C.group_tail_case, C.empty_ends_case, lambda: C.rectangular(*C.RECTANGULAR[1])])
def test_grad_ref_is_float64_autograd(builder):
    A, B, n = builder()
    m, k = len(A[0]) - 1, len(B[0]) - 1
    rowptr, col, val = C.ref64(A, B, n)[:3]
    G = np.random.default_rng(3).standard_normal(len(col))
    a64 = torch.from_numpy(A[2].astype(np.float64)).requires_grad_()
    b64 = torch.from_numpy(B[2].astype(np.float64)).requires_grad_()
    prod = torch.sparse.mm(_coo64(A, (m, k), a64), _coo64(B, (k, n), b64)).coalesce()
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    assert np.array_equal(prod.indices().numpy(), np.stack([rows, col]))
    np.testing.assert_allclose(prod.values().detach().numpy(), val, rtol=1e-12, atol=1e-14)
    (prod.values() * torch.from_numpy(G)).sum().backward()
    gA, gB, bA, bB, tA, tB = C.grad_ref(A, B, n, G)
    np.testing.assert_allclose(gA, a64.grad.numpy(), rtol=0, atol=1e-13 * max(1.0, bA.max()))
    np.testing.assert_allclose(gB, b64.grad.numpy(), rtol=0, atol=1e-13 * max(1.0, bB.max()))
    assert (np.abs(gA) <= bA).all() and (np.abs(gB) <= bB).all()
    assert np.array_equal(tA, np.diff(B[0])[A[1]])  # one term per entry of B's row


def test_grad_ref_row_weight_is_tiling():
    A, B, n, _, _ = C.multirow_case(0)
    m = 2 * C.P_TILE + 7
    Ai, Bi = C.ints(A, 1), C.ints(B, 2)
    nnz = len(C.ref32(A, B, n)[1])
    G = np.random.default_rng(4).integers(-4, 5, nnz).astype(np.float64)
    rowptr = C.ref32(A, B, n)[0]
    Gt = C.tile((rowptr, G, G), m)[1]
    full = C.grad_ref(C.tile(Ai, m), Bi, n, Gt)
    reps = np.bincount(np.arange(m) % C.P_TILE)
    pat = C.grad_ref(Ai, Bi, n, G, row_weight=reps)
    assert np.array_equal(full[1], pat[1]) and np.array_equal(full[5], pat[5])
    assert np.array_equal(full[0], C.tile((A[0], pat[0], pat[0]), m)[1])


def test_coalesce_ref_is_torch_coalesce():
    rng = np.random.default_rng(11)
    m, n, e = 40, 70, 900
    row, col, val = rng.integers(0, m, e), rng.integers(0, n, e), rng.standard_normal(e).astype(np.float32)
    rowptr, colu, valu, mp = C.coalesce_ref(row, col, val, m, n, np.float64)
    want = torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col])), torch.from_numpy(val.astype(np.float64)), (m, n)).coalesce()
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    assert np.array_equal(np.stack([rows, colu]), want.indices().numpy())
    np.testing.assert_allclose(valu, want.values().numpy(), rtol=1e-13, atol=1e-14)
    assert np.array_equal((rows * n + colu)[mp], row * n + col)
    acc = np.zeros(len(colu), dtype=np.float32)  # the same sum as an unbuffered scatter-add in input order
    np.add.at(acc, mp, val)
    assert np.array_equal(acc, C.coalesce_ref(row, col, val, m, n)[2])
