"""Shared cases of the ProNE / spectral-filter tests (test_prone_cpu.py, test_prone_gpu.py, test_prone_install_cpu.py and
the recorder tests/golden/make_golden_prone.py): the two graphs, the operand subsets of a filter step, a literal float32
loop for one step, a float32 numpy restatement of the reference's unfused filter sequences, and the bound both sides share.
Nothing here imports library code: the graphs are numpy's."""
import functools
import itertools
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prone")
WIDTHS = (1, 3, 8, 33, 64, 128, 200)
KINDS = ("prone", "gaussian", "heat", "ppr")
LONG = 128          # pick_long_thresh for graphs of this size: rows of more edges take the chunk-parallel path on the GPU
EPS = 2.0 ** -24


def csr_of_pairs(pairs, n):
    """Undirected pairs -> symmetric simple CSR (int32 rowptr, int32 colind ascending), no self loops."""
    p = np.asarray(sorted(set((min(u, v), max(u, v)) for u, v in pairs if u != v)), dtype=np.int64).reshape(-1, 2)
    r = np.concatenate([p[:, 0], p[:, 1]])
    c = np.concatenate([p[:, 1], p[:, 0]])
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return rowptr.astype(np.int32), c.astype(np.int32)


@functools.lru_cache(None)
def ragged():
    """300 nodes, symmetric, no self loops; node i of the first eight has exactly the degree DEGS[i], built explicitly: its
    neighbours are the first DEGS[i] nodes of 100 .. 299, which otherwise only link among themselves in a sparse ring.
    Nodes 8 .. 99 stay isolated except node 8 .. 19, which hang on a path."""
    degs = (0, 1, 63, 64, 65, 127, 128, 129)
    pairs = []
    for i, d in enumerate(degs):
        pairs += [(i, 100 + j) for j in range(d)]
    pairs += [(j, j + 1) for j in range(8, 19)]
    pairs += [(100 + j, 100 + (j + 7) % 200) for j in range(0, 200, 3)]
    rowptr, colind = csr_of_pairs(pairs, 300)
    deg = np.diff(rowptr)
    assert tuple(deg[:8]) == degs
    return rowptr, colind


@functools.lru_cache(None)
def hub():
    """2,000 nodes, about 20,000 entries; node 0 is adjacent to about 1,500 nodes (several long-row chunks at threshold
    128), node 1 to 300, the rest a random sparse graph (numpy default_rng(11))."""
    rng = np.random.default_rng(11)
    n = 2000
    pairs = [(0, int(v)) for v in rng.choice(np.arange(2, n), 1500, replace=False)]
    pairs += [(1, int(v)) for v in rng.choice(np.arange(2, n), 300, replace=False)]
    pairs += [(int(u), int(v)) for u, v in rng.integers(2, n, size=(8200, 2))]
    rowptr, colind = csr_of_pairs(pairs, n)
    deg = np.diff(rowptr)
    assert deg[0] >= 1500 and 19000 <= colind.size <= 21000
    return rowptr, colind


GRAPHS = {"ragged": ragged, "hub": hub}


def scipy_of(rowptr, colind):
    import scipy.sparse as sp

    n = rowptr.size - 1
    return sp.csr_matrix((np.ones(colind.size), colind.astype(np.int64), rowptr.astype(np.int64)), shape=(n, n))


def embedding_input(n, f, seed=5):
    """The [n, f] float64 matrix the filters are recorded on; values are float32-representable."""
    return np.random.default_rng(seed).standard_normal((n, f)).astype(np.float32).astype(np.float64)


# every subset of the optional operands (b, z1, z2, dst_scale, acc), val present or not
SUBSETS = [dict(zip(("b", "z1", "z2", "dst_scale", "acc", "val"), bits)) for bits in itertools.product((False, True), repeat=6)]


def step_operands(rowptr, colind, f, seed=0):
    """float32 operands of one filter step on the graph, all present; a test drops what its subset leaves out."""
    rng = np.random.default_rng(1000 + seed + f)
    n, nnz = rowptr.size - 1, colind.size
    g = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return dict(x=g(n, f), z1=g(n, f), z2=g(n, f), acc=g(n, f), val=(rng.random(nnz).astype(np.float32) + np.float32(0.5)),
                dst_scale=(rng.random(n).astype(np.float32) + np.float32(0.25)),
                a=-0.7, b=0.3, c1=-2.0, c2=-1.0, d=0.62)


def step_literal(rowptr, colind, val, x, a, b=0.0, z1=None, c1=0.0, z2=None, c2=0.0, dst_scale=None, acc=None, d=0.0,
                 dtype=np.float32):
    """The contract of cogdl_hip_csr_filter_step as a literal loop: edges in CSR order, every product and sum rounded to
    `dtype` separately, absent operands skipped.  -> (out, acc after) without touching the inputs.  dtype=float64 is the
    oracle of the long rows."""
    t_ = dtype
    n, f = x.shape
    xs = x.astype(t_)
    out = np.empty((n, f), dtype=t_)
    acc_out = None if acc is None else acc.astype(t_).copy()
    a, b, c1, c2, d = (t_(np.float32(v)) for v in (a, b, c1, c2, d))
    for i in range(n):
        t = np.zeros(f, dtype=t_)
        for e in range(rowptr[i], rowptr[i + 1]):
            row = xs[colind[e]]
            t = t + (t_(val[e]) * row if val is not None else row)
        s = t_(dst_scale[i]) * t if dst_scale is not None else t
        y = a * s
        if b != 0:
            y = y + b * xs[i]
        if z1 is not None:
            y = y + c1 * z1[i].astype(t_)
        if z2 is not None:
            y = y + c2 * z2[i].astype(t_)
        out[i] = y
        if acc_out is not None:
            acc_out[i] = acc_out[i] + d * y
    return out, acc_out


def restate_f32(kind, rowptr, colind, emb, bessel, dtype=np.float32, **params):
    """The reference's UNFUSED sequence (prone_utils.py; default parameters unless `params` gives them) restated in float32
    numpy / scipy: the matrix is assembled as the reference assembles it (in float64, then rounded to float32 once), every
    product and elementwise pass runs in float32.  Its distance from the float64 golden is what float32 costs this
    computation: err_ref of the bound.  dtype=float64 is the reference's own computation (the truth where nothing is
    recorded)."""
    import scipy.sparse as sp
    from sklearn import preprocessing

    f32 = dtype
    n = emb.shape[0]
    a = emb.astype(f32)
    mx = scipy_of(rowptr, colind)
    iv = lambda i, s: f32(bessel(i, s))
    if kind == "ppr":
        alpha, k = params.get("alpha", 0.5), params.get("k", 10)
        mx_norm = preprocessing.normalize(mx, "l1").astype(f32)
        lx = a
        conv = f32(alpha) * lx
        for _ in range(1, k):
            lx = f32(1 - alpha) * mx_norm.dot(lx)
            conv = conv + lx
        return conv
    if kind == "heat":
        t, k = params.get("t", 0.2), params.get("k", 5)
        lap = (sp.eye(n) - preprocessing.normalize(mx + sp.eye(n), "l1")).astype(f32)
        conv = iv(0, t) * a
        lx0, lx1 = a, lap.dot(a)
        conv = conv - f32(2) * iv(1, t) * lx1
        for i in range(2, k):
            lx2 = f32(2) * lap.dot(lx1) - lx0
            conv = conv + f32((-1) ** i * 2) * iv(i, t) * lx2
            lx0, lx1 = lx1, lx2
        return conv
    if kind == "gaussian":
        mu, s, order = params.get("mu", 0.5), params.get("theta", 1.0), params.get("k", 3)
    else:
        mu, s, order = params.get("mu", 0.1), params.get("s", 0.5), params.get("order", 10)
    big = sp.eye(n) + mx
    m = ((1 - mu) * sp.eye(n) - preprocessing.normalize(big, "l1")).astype(f32)
    lx0 = a
    lx1 = m.dot(a)
    lx1 = f32(0.5) * m.dot(lx1) - a
    conv = iv(0, s) * lx0
    conv = conv - f32(2) * iv(1, s) * lx1
    for i in range(2, order):
        lx2 = m.dot(lx1)
        lx2 = (m.dot(lx2) - f32(2) * lx1) - lx0
        conv = conv + f32((-1) ** i * 2) * iv(i, s) * lx2
        lx0, lx1 = lx1, lx2
    if kind == "gaussian":
        return conv
    return big.astype(f32).dot(a - conv)


def bound(err_ref, golden):
    """The bound of tests/test_disen_gpu.py: four times what the float32 restatement of the reference's own sequence
    loses, plus eight float32 roundings of the largest value."""
    return 4.0 * err_ref + 8.0 * EPS * float(np.abs(golden).max())


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))


def dense_input():
    """The fixed full-rank [300, 8] matrix of the dense-embedding golden (columns of decreasing scale)."""
    rng = np.random.default_rng(21)
    return rng.standard_normal((300, 8)) * np.array([8.0, 5.0, 3.0, 2.0, 1.5, 1.0, 0.7, 0.4])


def cosine(e):
    return e @ e.T
