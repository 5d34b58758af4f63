"""Shared cases of the NetSMF tests (test_netsmf_host.py, test_netsmf_gpu.py): the graphs, the exact expectation of the count
matrix, a pure-Python restatement of the sampling law (csrc/netsmf_law.h) with its own Philox4x32-10, and the checks that run
unchanged on a CPU graph (host twin) and on a GPU graph (HIP kernel).  Nothing here imports library code but the operators
under test and the synthetic-graph helpers."""
import functools
import os

import numpy as np
import torch

from cogdl_amd import embedding, synth
from cogdl_amd.operators import netsmf as ns

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netsmf.npz")

RING_CHORDS = [(i, (i + 1) % 12) for i in range(12)] + [(0, 5), (2, 9), (3, 7), (1, 6), (4, 10), (0, 2), (8, 11)]
TRIANGLE = [(12, 13), (13, 14), (12, 14)]


def csr_of_dense(a):
    r, c = np.nonzero(a)
    indptr = np.zeros(a.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=a.shape[0]), out=indptr[1:])
    return torch.from_numpy(indptr), torch.from_numpy(c.astype(np.int64))


def symmetric_dense(pairs, n):
    a = np.zeros((n, n), dtype=np.float64)
    for u, v in pairs:
        a[u, v] = a[v, u] = 1.0
    return a


@functools.lru_cache(None)
def g15():
    """A 12-ring plus seven chords, and a separate triangle 12-13-14: symmetric, 44 CSR entries.  -> (indptr, indices, A)"""
    a = symmetric_dense(RING_CHORDS + TRIANGLE, 15)
    assert int(a.sum()) == 44
    return csr_of_dense(a) + (a,)


@functools.lru_cache(None)
def ring_chords():
    """The 12-node component of G15 alone (what the golden file was recorded on).  -> (indptr, indices, A)"""
    a = symmetric_dense(RING_CHORDS, 12)
    return csr_of_dense(a) + (a,)


@functools.lru_cache(None)
def gd():
    """A directed R-MAT multigraph of 300 nodes (duplicates kept, rows in drawing order) with a row longer than 64, a
    reachable node without out-neighbours and an empty row before a non-empty one.  -> (indptr, indices, n)"""
    n = 300
    src, dst = synth.rmat_pairs(n, 2500, seed=3)
    indptr, perm = synth.coo_to_csr_stable(src, dst, n)
    indices = dst[perm].contiguous()
    deg = (indptr[1:] - indptr[:-1]).numpy()
    assert deg.max() > 64
    sinks = np.nonzero(deg == 0)[0]
    assert np.isin(indices.numpy(), sinks).any(), "no reachable node without out-neighbours"
    assert (deg[:-1] == 0).any() and deg[np.nonzero(deg == 0)[0][0]:].max() > 0
    return indptr, indices, n


def expected_counts(a, window, passes):
    """mu = passes * sum_{r <= T} D P^r in float64: one pass over the entries of a symmetric unit-weight graph has
    E[C_r] = D P^r for every split k, because (P^T)^(k-1) A P^(r-k) = D P^r (P^T D = A)."""
    deg = a.sum(1)
    p = a / deg[:, None]
    d = np.diag(deg)
    return passes * sum(d @ np.linalg.matrix_power(p, r) for r in range(1, window + 1))


def dense_counts(rowptr, col, count, n):
    rowptr, col, count = rowptr.cpu().numpy(), col.cpu().numpy(), count.cpu().numpy()
    c = np.zeros((n, n), dtype=np.int64)
    c[np.repeat(np.arange(n), np.diff(rowptr)), col] = count
    return c


def dense_of_csr(rowptr, col, val, n):
    rowptr, col, val = rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
    m = np.zeros((n, n), dtype=np.float64)
    m[np.repeat(np.arange(n), np.diff(rowptr)), col] = val
    return m


def assert_canonical(rowptr, col, n):
    rowptr, col = rowptr.cpu().numpy(), col.cpu().numpy()
    assert rowptr[0] == 0 and rowptr[-1] == col.size and (np.diff(rowptr) >= 0).all()
    keys = np.repeat(np.arange(n), np.diff(rowptr)).astype(np.int64) * n + col
    assert (np.diff(keys) > 0).all(), "columns are not ascending and distinct per row"


# ------------------------------------------------------------------------------------------------ the law, restated
M32 = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers."""
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw_below(seed, s, r, i, n):
    """The draw of (seed, sample s, length r, step i), reduced to [0, n): the high 64 bits of ((y << 32) | z) * n."""
    _, y, z, _ = philox4x32_10(s & M32, (s >> 32) & M32, r, i, seed & M32, (seed >> 32) & M32)
    return (((y << 32) | z) * n) >> 64


def split_k(seed, s, r):
    return 1 + draw_below(seed, s, r, 0, r)


def restated_pairs(indptr, indices, window, first, count, seed):
    """path_pairs, sample by sample, in Python."""
    indptr, indices = indptr.tolist(), indices.tolist()
    n, e_total = len(indptr) - 1, len(indices)
    row, col = [0] * (window * count), [0] * (window * count)
    for s in range(first, first + count):
        e = s % e_total
        u0 = max(x for x in range(n) if indptr[x] <= e)  # the last row that starts at or before e: empty rows skipped
        for r in range(1, window + 1):
            u, v = u0, indices[e]
            k = split_k(seed, s, r)
            for i in range(1, r):
                x = u if i <= k - 1 else v
                beg, deg = indptr[x], indptr[x + 1] - indptr[x]
                if deg:
                    x = indices[beg + draw_below(seed, s, r, i, deg)]
                if i <= k - 1:
                    u = x
                else:
                    v = x
            row[(r - 1) * count + (s - first)], col[(r - 1) * count + (s - first)] = u, v
    return np.asarray(row, dtype=np.int32), np.asarray(col, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ checks for both devices
LAW_WINDOW, LAW_PASSES, LAW_SEED = 3, 4096, 20241


def check_law(device):
    """G15, T = 3, 4096 passes: count 0 wherever mu = 0 (every ring <-> triangle cell), |C - mu| <= 6 sqrt(mu) + 1 elsewhere
    (a count is a sum of independent indicators: variance <= mu)."""
    indptr, indices, a = g15()
    rowptr, col, count = ns.path_counts(indptr.to(device), indices.to(device), LAW_WINDOW, LAW_PASSES, seed=LAW_SEED)
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and count.dtype == torch.int64
    assert count.device.type == torch.device(device).type
    assert_canonical(rowptr, col, 15)
    c = dense_counts(rowptr, col, count, 15)
    mu = expected_counts(a, LAW_WINDOW, LAW_PASSES)
    assert c.sum() == LAW_WINDOW * LAW_PASSES * 44
    assert (mu[:12, 12:] == 0).all() and (mu[12:, :12] == 0).all()
    assert (c[mu == 0] == 0).all(), "a pair where no path can end"
    dev = np.abs(c - mu)[mu > 0] / np.sqrt(mu[mu > 0])
    print("largest deviation: %.2f sigma" % dev.max())
    assert (np.abs(c - mu) <= 6.0 * np.sqrt(mu) + 1.0).all()


def block_diagonal():
    """5 all-ones blocks of sizes 7, 11, 13, 17, 19 scaled 5, 4, 3, 2, 1, as CSR: rank 5, singular values scale * size
    (35, 44, 39, 34, 19).  -> (rowptr, col, val, n, blocks, singular values descending)"""
    sizes, scales = (7, 11, 13, 17, 19), (5.0, 4.0, 3.0, 2.0, 1.0)
    n = sum(sizes)
    m = np.zeros((n, n), dtype=np.float32)
    block = np.zeros(n, dtype=np.int64)
    at = 0
    for b, (size, scale) in enumerate(zip(sizes, scales)):
        m[at:at + size, at:at + size] = scale
        block[at:at + size] = b
        at += size
    r, c = np.nonzero(m)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    sv = np.sort(np.asarray(sizes) * np.asarray(scales))[::-1]
    return (torch.from_numpy(rowptr).int(), torch.from_numpy(c.astype(np.int32)), torch.from_numpy(m[r, c]), n, block, sv, m)


def svd_deviations(device):
    """-> (largest relative deviation of S, largest deviation of |<row_i, row_j>| from 0 / 1) on the block-diagonal case,
    against numpy.linalg.svd in float64."""
    rowptr, col, val, n, block, sv, m = block_diagonal()
    u, s = ns.randomized_svd(rowptr.to(device), col.to(device), val.to(device), n, 5, seed=5)
    assert tuple(u.shape) == (n, 5) and tuple(s.shape) == (5,) and u.dtype == torch.float32 and s.dtype == torch.float32
    assert u.device.type == torch.device(device).type
    exact = np.linalg.svd(m.astype(np.float64), compute_uv=False)[:5]
    assert np.allclose(exact, sv, rtol=1e-12)
    dev_s = float(np.max(np.abs(s.cpu().numpy().astype(np.float64) - exact) / exact))
    emb = (u * s.sqrt()).cpu().numpy().astype(np.float64)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    gram = np.abs(emb @ emb.T)
    want = (block[:, None] == block[None, :]).astype(np.float64)  # +- one unit vector per block, blocks orthogonal
    return dev_s, float(np.max(np.abs(gram - want)))


def golden():
    return np.load(GOLDEN)


def check_sparsifier_reproduces_golden(device):
    """sparsifier on the integer counts behind the reference's `matrix` reproduces the reference's M: the same pattern up to
    entries whose pre-log value is within 1e-6 of 1, values within 1e-5."""
    g = golden()
    indptr, indices, _ = ring_chords()
    window, rounds = int(g["window"]), int(g["num_round"])
    counts = g["matrix"] * window * rounds  # every reference sample adds 1 / (window * num_round)
    c = np.rint(counts).astype(np.int64)
    assert np.abs(counts - c).max() < 1e-6 and c.sum() == window * rounds * 19
    r, cc = np.nonzero(c)
    rowptr = np.zeros(13, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=12), out=rowptr[1:])
    # rounds of the reference = rounds / 2 passes: the scale 1 / (2 * window * passes) is 1 / (window * rounds)
    assert rounds % 2 == 0
    m_rowptr, m_col, m_val = ns.sparsifier(indptr.to(device), torch.from_numpy(rowptr).int().to(device),
                                           torch.from_numpy(cc.astype(np.int32)).to(device),
                                           torch.from_numpy(c[r, cc]).to(device), window, rounds // 2, int(g["negative"]))
    assert m_val.dtype == torch.float32 and m_rowptr.dtype == torch.int32 and m_col.dtype == torch.int32
    assert_canonical(m_rowptr, m_col, 12)
    got, want = dense_of_csr(m_rowptr, m_col, m_val, 12), g["M"]
    differ = (got != 0) != (want != 0)
    assert (np.maximum(got, want)[differ] < 1e-6).all(), "pattern differs beyond entries at the threshold"
    print("largest deviation from the golden M: %.2e" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-5


GOLDEN_PASSES = 1000


def check_own_estimate_agrees_with_golden(device):
    """The library's W = C / (2 T passes), passes = 1000, and the reference's `matrix` (2000 rounds) both estimate
    (1 / 2T) sum_r D P^r: cell by cell within 6 combined standard errors plus one count."""
    g = golden()
    indptr, indices, a = ring_chords()
    window = int(g["window"])
    assert int(g["num_round"]) == 2 * GOLDEN_PASSES
    rowptr, col, count = ns.path_counts(indptr.to(device), indices.to(device), window, GOLDEN_PASSES, seed=99)
    unit = 1.0 / (2.0 * window * GOLDEN_PASSES)
    w = dense_counts(rowptr, col, count, 12) * unit
    mu = expected_counts(a, window, GOLDEN_PASSES)  # of either count matrix; each has variance <= mu
    bound = 6.0 * np.sqrt(2.0 * mu) * unit + unit
    print("largest difference / bound: %.3f" % np.max(np.abs(w - g["matrix"]) / bound))
    assert (np.abs(w - g["matrix"]) <= bound).all()


def sbm_graph():
    """The SBM of the golden file: 4 blocks of 32 nodes.  -> (indptr, indices, block)"""
    g = golden()
    a = symmetric_dense(g["sbm_edges"].tolist(), 128)
    return csr_of_dense(a) + (np.arange(128) // 32,)


def purity(emb, block):
    """The fraction of nodes whose nearest neighbour by cosine lies in their own block."""
    emb = np.asarray(emb, dtype=np.float64)
    emb = emb / np.maximum(np.linalg.norm(emb, axis=1, keepdims=True), 1e-30)
    sim = emb @ emb.T
    np.fill_diagonal(sim, -np.inf)
    return float(np.mean(block[sim.argmax(1)] == block))


def check_end_to_end(device):
    g = golden()
    p = float(g["sbm_purity"])
    assert p >= 0.9
    indptr, indices, block = sbm_graph()
    emb = embedding.netsmf((indptr.to(device), indices.to(device)), dim=8, window=5, rounds=100, seed=4)
    assert tuple(emb.shape) == (128, 8) and emb.dtype == torch.float32 and emb.device.type == torch.device(device).type
    norms = emb.norm(dim=1).cpu().numpy()
    assert np.allclose(norms, 1.0, atol=1e-5)
    got = purity(emb.cpu().numpy(), block)
    print("purity %.4f, the reference's %.4f" % (got, p))
    assert got >= p - 3.0 * np.sqrt(p * (1.0 - p) / 128.0)
