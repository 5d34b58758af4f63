"""References and case builders for the SpGEMM tests (CPU only: numpy + torch).

A CSR here is a tuple (rowptr int64 [rows+1], col int64 [nnz], val float32 [nnz]) of numpy arrays; it need not be
canonical.  The contract of cogdl_amd/csrc/spgemm.hip in plain code:

  ref32   every product float32(a) * float32(b) rounded once; the products of one output entry added left to right in
          float32 in EXPANSION order (A_i's entries in CSR order, for each of them B_k's entries in CSR order), starting from
          the first product.  The kernel must return these bits on every path.
  ref64   the same in float64, with sum |a b| and the number of products of every entry: the yardstick of ref32 itself.
  grad_ref  the closed forms of the kernel header in float64, product by product, so duplicates and unsorted columns in A
          or B need nothing special: gA[e] = sum over the products of entry e of G[c] b, gB[q] = sum of a G[c].

The builders return cases whose rows provably take the path they are meant for: every test asserts that from ub() first.
"""
import numpy as np
import torch

CAPS = (256, 1024, 4096)  # kSpgCap0..2: a row with ub products goes to the first bin whose cap holds it, else to the hub path
THREADS = (64, 256, 512)  # workgroup size of the three LDS bins = the chunk of A entries expanded at a time
U = 2.0 ** -24            # unit roundoff of float32
P_TILE = 53               # distinct row patterns of a tiled case (prime: i -> i + 65536 walks through all of them)


def gamma(t):
    """The classical constant of t roundings: t u / (1 - t u)."""
    t = np.asarray(t, dtype=np.float64)
    return t * U / (1.0 - t * U)


# ---- the product, product by product ---------------------------------------------------------------------------------
def expand(A, B):
    """The products of A . B in expansion order -> (row, col, ea, eb): the row of A and the column of B of every product,
    and the positions of its two factors in A's and B's entry arrays."""
    rA, cA, _ = A
    rB, cB, _ = B
    lens = rB[cA + 1] - rB[cA]
    ea = np.repeat(np.arange(len(cA), dtype=np.int64), lens)
    first = np.cumsum(lens) - lens
    eb = rB[cA][ea] + (np.arange(len(ea), dtype=np.int64) - first[ea])
    row = np.repeat(np.arange(len(rA) - 1, dtype=np.int64), np.diff(rA))[ea]
    return row, cB[eb], ea, eb


def ub(A, B):
    """Products per row of A . B (the kernel's ub_i)."""
    rA, cA, _ = A
    rB = B[0]
    rows = np.repeat(np.arange(len(rA) - 1), np.diff(rA))
    return np.bincount(rows, weights=(rB[cA + 1] - rB[cA]).astype(np.float64), minlength=len(rA) - 1).astype(np.int64)


def bin_of(u):
    """-1 for a row without products, 0..2 for the LDS bins, 3 for the global-memory (hub) path."""
    u = np.asarray(u)
    return np.where(u == 0, -1, np.where(u <= CAPS[0], 0, np.where(u <= CAPS[1], 1, np.where(u <= CAPS[2], 2, 3))))


def _runs(row, col, n, reverse=False):
    """Products grouped by output entry, each group in expansion order (reverse=True: every row's products reversed).
    -> (order, start, length, key): order[t] = the product at sorted position t; run r is order[start[r] : + length[r]]
    and belongs to entry key[r] = row * n + col."""
    key = row * np.int64(n) + col
    idx = np.arange(len(key), dtype=np.int64)
    if reverse:
        idx = idx[::-1]
    order = idx[np.argsort(key[idx], kind="stable")]
    ks = key[order]
    head = np.ones(len(ks), dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(head)
    length = np.diff(np.append(start, len(ks)))
    return order, start, length, ks[start]


def seq_sum(vals, start, length):
    """Per run vals[start] + vals[start + 1] + .. added left to right, every addition rounded in vals' dtype.  Step t adds
    the t-th element of every run that has one (no reliance on the order in which a scatter-add visits its indices)."""
    acc = vals[start].copy()
    if len(length) == 0:
        return acc
    by_len = np.argsort(-length, kind="stable")
    neg = -length[by_len]
    for t in range(1, int(length.max())):
        live = by_len[:np.searchsorted(neg, -t, side="left")]  # the runs longer than t
        acc[live] = acc[live] + vals[start[live] + t]
    return acc


def _product(A, B, n, dtype, reverse=False):
    row, col, ea, eb = expand(A, B)
    prod = A[2].astype(dtype)[ea] * B[2].astype(dtype)[eb]
    order, start, length, key = _runs(row, col, n, reverse)
    m = len(A[0]) - 1
    rowptr = np.zeros(m + 1, dtype=np.int64)
    if len(key):
        np.cumsum(np.bincount(key // n, minlength=m), out=rowptr[1:])
    colC = key % n if len(key) else key
    return rowptr, colC, prod[order], start, length


def ref32(A, B, n, reverse=False):
    """The stated float32 contract -> canonical CSR (rowptr, col, val float32) with the structural pattern."""
    rowptr, col, prod, start, length = _product(A, B, n, np.float32, reverse)
    return rowptr, col, seq_sum(prod, start, length)


def ref64(A, B, n):
    """-> (rowptr, col, val float64, sum |a b| per entry, products per entry)."""
    rowptr, col, prod, start, length = _product(A, B, n, np.float64)
    return rowptr, col, seq_sum(prod, start, length), seq_sum(np.abs(prod), start, length), length


def grad_ref(A, B, n, G, row_weight=None):
    """Closed-form gradients in float64 for the upstream gradient G (one value per entry of C, canonical order):
    -> (gA, gB, boundA, boundB, tA, tB) with bound = the same sums over absolute values and t = the terms per entry.
    row_weight[i] (optional) counts row i of A that many times in gB: a tiled A against one pattern of it."""
    row, col, ea, eb = expand(A, B)
    order, start, length, _ = _runs(row, col, n)
    c = np.empty(len(row), dtype=np.int64)
    c[order] = np.repeat(np.arange(len(start), dtype=np.int64), length)
    a, b, g = A[2].astype(np.float64)[ea], B[2].astype(np.float64)[eb], np.asarray(G, dtype=np.float64)[c]
    w = 1.0 if row_weight is None else np.asarray(row_weight, dtype=np.float64)[row]
    na, nb = len(A[1]), len(B[1])
    return (np.bincount(ea, g * b, na), np.bincount(eb, a * g * w, nb),
            np.bincount(ea, np.abs(g * b), na), np.bincount(eb, np.abs(a * g) * w, nb),
            np.bincount(ea, minlength=na), np.bincount(eb, w * np.ones(len(eb)), nb))


def coalesce_ref(row, col, val, m, n, dtype=np.float32):
    """COO -> canonical CSR with the duplicates summed in INPUT order in `dtype` -> (rowptr, col, val, map)."""
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    order, start, length, key = _runs(row, col, n)
    mp = np.empty(len(row), dtype=np.int64)
    mp[order] = np.repeat(np.arange(len(start), dtype=np.int64), length)
    rowptr = np.zeros(m + 1, dtype=np.int64)
    if len(key):
        np.cumsum(np.bincount(key // n, minlength=m), out=rowptr[1:])
    return rowptr, (key % n if len(key) else key), seq_sum(np.asarray(val).astype(dtype)[order], start, length), mp


# ---- CSR plumbing ----------------------------------------------------------------------------------------------------
def csr_of_rows(rows):
    """[(cols, vals), ..] -> CSR, the entries of every row in the order given."""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(c) for c, _ in rows], out=rowptr[1:])
    if rows:
        return (rowptr, np.concatenate([np.asarray(c, dtype=np.int64) for c, _ in rows]),
                np.concatenate([np.asarray(v, dtype=np.float32) for _, v in rows]))
    return rowptr, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)


def csr_of_dense(d):
    d = np.asarray(d, dtype=np.float32)
    r, c = np.nonzero(d)
    rowptr = np.zeros(d.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=d.shape[0]), out=rowptr[1:])
    return rowptr, c.astype(np.int64), d[r, c]


def ints(X, seed):
    """The same pattern with values drawn from {-4 .. 4}: every product and every partial sum is an integer far below 2^24,
    so float32 and float64 agree exactly whatever the order."""
    return X[0], X[1], np.random.default_rng(seed).integers(-4, 5, len(X[1])).astype(np.float32)


def tile(X, m):
    """The CSR with m rows whose row i is row i % P of X."""
    rowptr, col, val = X
    p = len(rowptr) - 1
    reps, rem = divmod(m, p)
    lens = np.concatenate([np.tile(np.diff(rowptr), reps), np.diff(rowptr)[:rem]])
    out = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(lens, out=out[1:])
    return (out, np.concatenate([np.tile(col, reps), col[:rowptr[rem]]]), np.concatenate([np.tile(val, reps), val[:rowptr[rem]]]))


def to_device(X, dev):
    return (torch.from_numpy(X[0].astype(np.int32)).to(dev), torch.from_numpy(X[1].astype(np.int32)).to(dev),
            torch.from_numpy(np.asarray(X[2], dtype=np.float32)).to(dev))


def _vals(rng, count):
    return rng.standard_normal(count).astype(np.float32)


def _sorted_choice(rng, pool, count):
    return np.sort(rng.choice(pool, size=count, replace=False))


# ---- the suite's random shapes -----------------------------------------------------------------------------------------
def _random(m, n, density, seed):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(m, n, generator=g) < density
    return torch.where(mask, torch.randn(m, n, generator=g), torch.zeros(()))


RECTANGULAR = [(37, 53, 29, 0.1, 0), (200, 150, 300, 0.05, 1), (64, 500, 7, 0.3, 2), (300, 40, 900, 0.2, 3), (1, 1, 1, 1.0, 4)]


def rectangular(m, k, n, d, seed):
    return csr_of_dense(_random(m, k, d, seed).numpy()), csr_of_dense(_random(k, n, d, seed + 100).numpy()), n


def every_bin():
    """test_every_bin_and_the_global_path's matrices: rows with ~1 .. 20 k products."""
    g = torch.Generator().manual_seed(5)
    k, n = 400, 3000
    b = _random(k, n, 0.02, 6)
    rows = []
    for nnz_row in (1, 3, 10, 40, 60, 150, 330):
        r = torch.zeros(k)
        r[torch.randperm(k, generator=g)[:nnz_row]] = torch.randn(nnz_row, generator=g)
        rows.append(r)
    return csr_of_dense(torch.stack(rows).numpy()), csr_of_dense(b.numpy()), n


def hub_row():
    """test_hub_row_forces_the_global_path's shape: one A row references every row of a dense-ish B."""
    a = _random(50, 300, 0.05, 7)
    a[17] = torch.randn(300, generator=torch.Generator().manual_seed(17))
    return csr_of_dense(a.numpy()), csr_of_dense(_random(300, 2500, 0.8, 8).numpy()), 2500


def random_cases():
    """(name, A, B, n) of every random case of the exact comparison; the order condition is asserted on each."""
    out = [("rect-%dx%dx%d" % c[:3],) + rectangular(*c) for c in RECTANGULAR]
    return out + [("every_bin",) + every_bin(), ("hub_row",) + hub_row()]


# ---- bin boundaries ----------------------------------------------------------------------------------------------------
BOUNDARY_UB = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4098)


def boundary_case(seed=0):
    """One A whose rows have ub exactly BOUNDARY_UB, three rows per value:
      'one'       all products in one column (ub unit rows of B that all hold column 7): one run of length ub;
      'distinct'  all products in distinct columns (row_nnz == ub: the count kernel's hash set at load factor 1/2);
      'mixed'     32-entry rows of B over 256 columns: runs of ~ub/256.
    First and last row of A are empty.  -> (A, B, n, claims) with claims[i] = (row, ub, kind)."""
    rng = np.random.default_rng(seed)
    n = 8192
    rows_b = [(np.array([7]), _vals(rng, 1)) for _ in range(4098)]  # unit rows 0 .. 4097
    perm = rng.permutation(8191)
    dist0, at = len(rows_b), 0
    for bit in range(13):  # row dist0 + bit: 2^bit columns shared with no other 'distinct' row
        rows_b.append((np.sort(perm[at:at + (1 << bit)]), _vals(rng, 1 << bit)))
        at += 1 << bit
    mix0 = len(rows_b)
    for _ in range(130):  # rows mix0 .. mix0 + 129: 32 entries
        rows_b.append((_sorted_choice(rng, 256, 32), _vals(rng, 32)))
    small0 = len(rows_b)
    for bit in range(5):  # row small0 + bit: 2^bit entries
        rows_b.append((_sorted_choice(rng, 256, 1 << bit), _vals(rng, 1 << bit)))
    rows_a, claims = [(np.zeros(0), np.zeros(0))], []
    for u in BOUNDARY_UB:
        for kind in ("one", "distinct", "mixed"):
            if kind == "one":
                cols = np.arange(u)
            elif kind == "distinct":
                cols = dist0 + np.array([bit for bit in range(13) if u >> bit & 1])
            else:
                cols = np.concatenate([mix0 + _sorted_choice(rng, 130, u // 32),
                                       small0 + np.array([bit for bit in range(5) if (u % 32) >> bit & 1], dtype=np.int64)])
            claims.append((len(rows_a), u, kind))
            rows_a.append((cols, _vals(rng, len(cols))))
    rows_a.append((np.zeros(0), np.zeros(0)))
    return csr_of_rows(rows_a), csr_of_rows(rows_b), n, claims


# ---- more than one chunk of A entries inside an LDS bin ---------------------------------------------------------------------
CHUNK_ROWS = [(65, 0), (128, 0), (129, 0), (257, 1), (513, 1), (513, 2), (1025, 2)]  # (A entries, bin)
CHUNK_VARIANTS = ("plain", "edges", "trail")


def _chunk_lens(entries, threads, lo, hi, variant, rng):
    """B-row lengths in {0..3} for the `entries` entries of an A row with lo < sum <= hi.  'edges': the first and the last
    entry of every chunk of `threads` entries reference an empty row; 'trail': the whole last chunk does."""
    lens = rng.integers(0, 4, entries)
    fixed = np.zeros(entries, dtype=bool)
    if variant == "edges":
        for c in range(0, entries, threads):
            fixed[c] = fixed[min(c + threads, entries) - 1] = True
    elif variant == "trail":
        fixed[(entries - 1) // threads * threads:] = True
    lens[fixed] = 0
    free = np.flatnonzero(~fixed)
    while lens.sum() > hi:
        lens[rng.choice(free[lens[free] > 0])] -= 1
    while lens.sum() <= lo:
        lens[rng.choice(free[lens[free] < 3])] += 1
    return lens


def chunk_case(seed=0):
    """A rows longer than their bin's workgroup whose ub still fits the bin: row r of B has r % 4 entries over 48 columns,
    and an A row takes ascending rows of B with the lengths _chunk_lens chose (A stays canonical).
    -> (A, B, n, claims) with claims[i] = (row, entries, bin, variant, lens)."""
    rng = np.random.default_rng(seed)
    n, k = 48, 4 * 1025 + 8
    rows_b = [(_sorted_choice(rng, n, r % 4), _vals(rng, r % 4)) for r in range(k)]
    rows_a, claims = [], []
    for entries, b in CHUNK_ROWS:
        for variant in CHUNK_VARIANTS:
            lens = _chunk_lens(entries, THREADS[b], CAPS[b - 1] if b else 0, CAPS[b], variant, rng)
            cols, at = np.empty(entries, dtype=np.int64), 0
            for p, want in enumerate(lens):  # the next row of B at or after `at` with this length
                at += (want - at) % 4
                cols[p] = at
                at += 1
            claims.append((len(rows_a), entries, b, variant, lens))
            rows_a.append((cols, _vals(rng, entries)))
    return csr_of_rows(rows_a), csr_of_rows(rows_b), n, claims


# ---- tiled cases: more rows in one bin than its launch has workgroups -----------------------------------------------------
def _orbit_targets(rng, lo, hi, step):
    """P_TILE values in (lo, hi] such that pattern p and pattern (p + step) % P_TILE -- two rows that one workgroup
    processes one after the other when the bin's list is in row order -- alternate between the larger and the smaller
    half; the orbit starts with hi (the bin's CAP) followed by lo + 1 (its minimum)."""
    rest = np.sort(rng.integers(lo + 1, hi + 1, P_TILE - 2))[::-1]
    big, small = [hi] + list(rest[:P_TILE // 2]), [lo + 1] + list(rest[P_TILE // 2:][::-1])
    out = np.zeros(P_TILE, dtype=np.int64)
    for j in range(P_TILE):
        out[(j * step) % P_TILE] = big[j // 2] if j % 2 == 0 else small[j // 2]
    return out


def multirow_case(b, seed=0, m=66037):
    """Bin b: P_TILE row patterns with ub in (CAPS[b-1], CAPS[b]], the minimum and the CAP among them, tiled to m rows.
    B has rows of every length 0 .. L over n = 64 columns; a pattern with ub = u has max(16, ceil(u / L)) entries whose
    B rows' lengths differ by at most one (bin 0: exactly 16 entries per row, so nnz(A) = 16 m).
    -> (A pattern, B, n, m, targets)."""
    rng = np.random.default_rng(seed + 10 * b)
    n, longest, per = 64, (16, 16, 32)[b], (16, 64, 128)[b]
    rows_b = []
    for length in range(longest + 1):  # rows per * length .. per * length + per - 1 have `length` entries
        for _ in range(per):
            rows_b.append((_sorted_choice(rng, n, length), _vals(rng, length)))
    targets = _orbit_targets(rng, CAPS[b - 1] if b else 0, CAPS[b], 65536 % P_TILE)
    rows_a = []
    for u in targets:
        entries = max(16, -(-int(u) // longest))
        lens = np.full(entries, u // entries)
        lens[:u % entries] += 1
        cols = np.concatenate([per * length + _sorted_choice(rng, per, int((lens == length).sum())) for length in np.unique(lens)])
        rows_a.append((np.sort(cols), _vals(rng, entries)))
    return csr_of_rows(rows_a), csr_of_rows(rows_b), n, m, targets


def hub_stride_case(seed=0, m=4121):
    """More hub rows than the 4096 workgroups of the hub kernels: P_TILE patterns of 69 .. 74 entries against rows of B
    with 60 .. 64 entries over n = 96 columns (ub just above 4096), tiled to m rows.  -> (A pattern, B, n, m)."""
    rng = np.random.default_rng(seed + 77)
    n, k = 96, 100
    rows_b = [(_sorted_choice(rng, n, length), _vals(rng, length)) for length in rng.integers(60, 65, k)]
    rows_a = [(_sorted_choice(rng, k, entries), _vals(rng, entries)) for entries in rng.integers(69, 75, P_TILE)]
    return csr_of_rows(rows_a), csr_of_rows(rows_b), n, m


# ---- non-canonical inputs, structural zeros, large column ids -------------------------------------------------------------
PATH_ENTRIES = (3, 20, 80, 200)  # A entries against ~30-entry rows of B: ub ~ 90, 600, 2400, 6000 = bins 0, 1, 2 and the hub path


def noncanonical_case(which, seed=0):
    """which in 'A', 'B', 'AB': that operand has unsorted columns with at least one duplicate in every row of two or more
    entries; one row of A on each of the four paths, and an empty one.  -> (A, B, n)."""
    rng = np.random.default_rng(seed + {"A": 1, "B": 2, "AB": 3}[which])
    n, k = 100, 200

    def row(count, bound, messy):
        if not messy:
            return _sorted_choice(rng, bound, count)
        while True:
            cols = rng.integers(0, bound, count)
            if count > 1:
                cols[-1] = cols[0]
            if count < 3 or (np.diff(cols) < 0).any():
                return cols

    rows_b = [(row(length, n, "B" in which), _vals(rng, length)) for length in rng.integers(25, 36, k)]
    rows_a = [(row(e, k, "A" in which), _vals(rng, e)) for e in PATH_ENTRIES[:2]] + [(np.zeros(0), np.zeros(0))]
    rows_a += [(row(e, k, "A" in which), _vals(rng, e)) for e in PATH_ENTRIES[2:]]
    return csr_of_rows(rows_a), csr_of_rows(rows_b), n


def zero_case(seed=0):
    """One row of A per path; in each, column n - 1 of C is x y + (-x) y and nothing else: rows 0 and 1 of B hold column
    n - 1 with the same y, no other row of B does, and A holds x and -x on them.  -> (A, B, n)."""
    rng = np.random.default_rng(seed + 5)
    n, k = 100, 200
    y = np.float32(1.2345678)
    rows_b = []
    for r in range(k):
        cols = _sorted_choice(rng, n - 1, int(rng.integers(25, 36)))
        vals = _vals(rng, len(cols))
        if r < 2:
            cols, vals = np.append(cols, n - 1), np.append(vals, y)
        rows_b.append((cols, vals))
    rows_a = []
    for e in PATH_ENTRIES:
        vals = _vals(rng, e)
        vals[1] = -vals[0]
        rows_a.append((np.concatenate([[0, 1], 2 + _sorted_choice(rng, k - 2, e - 2)]), vals))
    return csr_of_rows(rows_a), csr_of_rows(rows_b), n


BIG_N = 2 ** 31 - 1
BIG_SPECIAL = (0, 1, 2 ** 30, 2 ** 31 - 3, 2 ** 31 - 2)


def bigcol_case(seed=0):
    """n = 2^31 - 1: B's columns come from BIG_SPECIAL and 200 random ids, ~40 per row, so columns repeat across rows;
    A rows of 2, 12 and 60 entries (bins 0, 1, 2).  -> (A, B, n)."""
    rng = np.random.default_rng(seed + 9)
    k = 64
    pool = np.unique(np.concatenate([np.array(BIG_SPECIAL, dtype=np.int64), rng.integers(0, BIG_N, 200)]))
    rows_b = []
    for r in range(k):
        cols = np.unique(np.concatenate([rng.choice(pool, size=38, replace=False), rng.choice(np.array(BIG_SPECIAL), size=2)]))
        rows_b.append((cols, _vals(rng, len(cols))))
    rows_a = [(_sorted_choice(rng, k, e), _vals(rng, e)) for e in (2, 12, 60, 12, 2)]
    return csr_of_rows(rows_a), csr_of_rows(rows_b), BIG_N


# ---- gradient cases ------------------------------------------------------------------------------------------------------
GROUP_LENGTHS_B = (0, 1, 15, 16, 17, 33, 100)  # B rows: one 16-lane group walks row k of B for gA
GROUP_LENGTHS_A = (0, 1, 15, 16, 17, 33)       # A columns: one group walks column k of A for gB


def group_tail_case(seed=0):
    """Row r of B has GROUP_LENGTHS_B[r % 7] entries and column r of A GROUP_LENGTHS_A[r % 6] (k = 42 covers every pair).
    -> (A, B, n)."""
    rng = np.random.default_rng(seed + 21)
    m, k, n = 40, 42, 128
    rows_b = [(_sorted_choice(rng, n, GROUP_LENGTHS_B[r % 7]), _vals(rng, GROUP_LENGTHS_B[r % 7])) for r in range(k)]
    dense = np.zeros((m, k), dtype=np.float32)
    for c in range(k):
        rows = rng.choice(m, size=GROUP_LENGTHS_A[c % 6], replace=False)
        dense[rows, c] = _vals(rng, len(rows)) + np.float32(3.0)  # (never 0: the pattern is the point)
    return csr_of_dense(dense), csr_of_rows(rows_b), n


def empty_ends_case(seed=0):
    """A and B with their first three and last three rows empty (row_of's binary search over leading and trailing
    empties).  -> (A, B, n)."""
    rng = np.random.default_rng(seed + 22)
    m, k, n = 19, 23, 31
    a = np.where(rng.random((m, k)) < 0.4, rng.standard_normal((m, k)), 0)
    b = np.where(rng.random((k, n)) < 0.4, rng.standard_normal((k, n)), 0)
    a[:3] = a[-3:] = 0
    b[:3] = b[-3:] = 0
    return csr_of_dense(a), csr_of_dense(b), n


def stride_b_case(seed=0):
    """nnz(B) = 70,000 x 16 above the 65,536 x 16 gradient entries of one launch of spgemm_grad_b_kernel: B over n = 64
    columns, A 32 rows of 200 entries each (ub = 3200).  Integer values.  -> (A, B, n)."""
    rng = np.random.default_rng(seed + 23)
    m, k, n = 32, 70000, 64
    col_b = np.sort(np.argsort(rng.random((k, n)), axis=1)[:, :16], axis=1).reshape(-1).astype(np.int64)
    B = (np.arange(k + 1, dtype=np.int64) * 16, col_b, np.zeros(len(col_b), dtype=np.float32))
    rows_a = [(_sorted_choice(rng, k, 200), np.zeros(200)) for _ in range(m)]
    rows_a[-1][0][-1] = k - 1  # the last row of B has a product
    return ints(csr_of_rows(rows_a), seed + 1), ints(B, seed + 2), n
