"""NetSMF (Qiu et al., WWW'19) on the graph's device: path sampling, the sparsifier and a randomized SVD -- what the reference
does with an interpreted loop into a scipy lil_matrix, networkx dictionaries and sklearn (cogdl/models/emb/netsmf.py).

    path_pairs(indptr, indices, window, first, count, seed)          -> int32 (row, col), window * count pairs
    path_counts(indptr, indices, window, passes, seed, batch)        -> canonical CSR (rowptr, col, count) of the count matrix C
    sparsifier(indptr, rowptr, col, count, window, passes, negative) -> CSR float32 M = log max(1, ...) (netsmf.py:90-106)
    randomized_svd(rowptr, col, val, n, k, n_iter, oversample, seed) -> U [n, k], S [k]

A graph on the GPU goes to the HIP kernel (cogdl_hip_netsmf_sample, csrc/netsmf.hip) and to the library's device operators
(coalesce = csr2csc twice + coo_dupsum, csr2csc, csrspmm); a graph on the CPU goes to the host twin in libcogdl_host.so
(OpenMP), to the host SpMM and to a torch composition, and libcogdl_hip.so is not loaded.  Both sides sample by
csrc/netsmf_law.h: for equal inputs and seed they return the same pairs, so the same counts.

The law (include/cogdl_hip.h has the contract): sample s takes CSR entry e = s mod E as (u, v) and, for each r = 1 .. window,
draws k uniform on 1 .. r, walks u for k - 1 uniform steps and v for r - k, and counts the pair where they end.  One PASS is
s = 0 .. E - 1.  On a simple symmetric graph `num_round` rounds of the reference (each undirected edge once, orientation
flipped with probability 1/2) have the law of num_round / 2 passes; with unit weights every reference sample adds the same
constant, so its matrix is C / (2 * window * passes).

Differences from the reference: the draws are Philox's, not numpy's; at a node without out-neighbours the walker stays; rows
and columns of nodes of degree 0 are empty in the sparsifier (the reference divides by zero there: inf / nan).
"""
import torch

from .. import _lib
from .walk import _graph_checks, _seed, raise_for_flags

__all__ = ["path_pairs", "path_counts", "sparsifier", "randomized_svd"]

_I32_MAX = 2 ** 31 - 1
_SEGMENT_MAX_EDGES = 2 ** 31 - 2 ** 20  # COGDL_HIP_SEGMENT_MAX_EDGES: what one canonicalisation takes
MAX_WINDOW = 256
DEFAULT_BATCH = 2 ** 27  # pairs per batch when `batch` is None: 1 GiB of int32 pairs
_F32_EXACT = 2 ** 24     # float32 holds every integer up to here


def _graph(name, indptr, indices, window):
    _graph_checks(name, indptr, indices)
    if indptr.numel() - 1 > _I32_MAX:
        raise _lib.BackendError("%s: %d nodes; the pairs are int32 (limit 2^31 - 1)" % (name, indptr.numel() - 1))
    window = int(window)
    if window < 1 or window > MAX_WINDOW:
        raise ValueError("%s: window must be in [1, %d] (got %d)" % (name, MAX_WINDOW, window))
    return indptr.contiguous(), indices.contiguous(), window


def _pairs(indptr, indices, window, first, count, seed):
    """The call itself; arguments checked by the caller."""
    dev, n, e = indptr.device, indptr.numel() - 1, indices.numel()
    row = torch.empty(window * count, dtype=torch.int32, device=dev)
    col = torch.empty(window * count, dtype=torch.int32, device=dev)
    if count == 0:
        return row, col
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.twin_call("netsmf_sample", dev, _lib.ptr(indptr), _lib.ptr(indices), n, e, first, count, window, seed, _lib.ptr(row),
                   _lib.ptr(col), _lib.ptr(flags))
    raise_for_flags("netsmf_sample", flags.item(), n)  # the one synchronisation
    return row, col


def path_pairs(indptr, indices, window, first, count, seed=None):
    """The pairs of samples first .. first + count - 1 -> int32 (row, col), each of length window * count, on the graph's
    device: sample s with path length r sits at (r - 1) * count + (s - first).  A pair depends on (graph, seed, s, r) alone,
    not on how a range is cut into calls."""
    indptr, indices, window = _graph("path_pairs", indptr, indices, window)
    first, count = int(first), int(count)
    if first < 0 or count < 0:
        raise ValueError("path_pairs: first and count must be >= 0 (got %d, %d)" % (first, count))
    if count > 0 and indices.numel() == 0:
        raise ValueError("path_pairs: the graph has no edges to sample from")
    if window * count > _SEGMENT_MAX_EDGES:
        raise _lib.BackendError("path_pairs: %d pairs in one call (limit COGDL_HIP_SEGMENT_MAX_EDGES = %d)"
                                % (window * count, _SEGMENT_MAX_EDGES))
    return _pairs(indptr, indices, window, first, count, _seed(seed))


def _batch_keys(row, col, n):
    """One batch of pairs -> (sorted distinct keys row * n + col as int64, their int64 counts)."""
    if row.device.type != "cuda":
        return torch.unique(row.long() * n + col.long(), return_counts=True)
    from .spgemm import coalesce

    ones = torch.ones(row.numel(), dtype=torch.float32, device=row.device)
    rowptr_u, col_u, val_u = coalesce(row, col, ones, n, n)
    if val_u.numel() and float(val_u.max()) >= _F32_EXACT:
        raise _lib.BackendError("path_counts: a cell of the count matrix reached 2^24 within one batch (the duplicate sum "
                                "runs in float32); pass a smaller `batch`")
    rows = torch.repeat_interleave(torch.arange(n, device=row.device), (rowptr_u[1:] - rowptr_u[:-1]).long())
    return rows * n + col_u.long(), val_u.long()


def _merge(keys_a, cnt_a, keys_b, cnt_b):
    """Two sorted distinct key lists with integer counts -> their union with the counts added.  Each side writes distinct
    positions: plain indexed adds, no atomics."""
    if keys_a is None:
        return keys_b, cnt_b
    keys = torch.unique(torch.cat([keys_a, keys_b]))
    cnt = torch.zeros(keys.numel(), dtype=torch.long, device=keys.device)
    cnt[torch.searchsorted(keys, keys_a)] = cnt_a
    pos_b = torch.searchsorted(keys, keys_b)
    cnt[pos_b] = cnt[pos_b] + cnt_b
    return keys, cnt


def path_counts(indptr, indices, window, passes, seed=None, batch=None):
    """The count matrix C of S = passes * E samples (each with window pairs) -> canonical CSR (rowptr int32 [N + 1],
    col int32, count int64) on the graph's device: columns ascending and distinct per row, C[i, j] = the number of pairs
    that ended at (i, j).

    The samples are drawn in batches of at most `batch` pairs (None: DEFAULT_BATCH), never more than
    COGDL_HIP_SEGMENT_MAX_EDGES; each batch is made canonical (GPU: coalesce, i.e. csr2csc twice and coo_dupsum on a vector
    of ones; CPU: torch.unique) and merged into the running result.  The result is a function of (graph, window, passes,
    seed) alone: equal for every `batch`, from run to run, and between GPU and CPU.

    Exactness: counts run in integers.  The merge adds int64.  Inside one GPU batch the duplicate sum is a float32 sum of
    ones, exact below 2^24; a batch in which a cell reaches 2^24 is refused with BackendError (a batch of at most 2^24
    pairs cannot).  A count matrix of more than 2^31 - 1 cells is refused: the CSR is int32."""
    indptr, indices, window = _graph("path_counts", indptr, indices, window)
    passes = int(passes)
    if passes < 0:
        raise ValueError("path_counts: passes must be >= 0 (got %d)" % passes)
    limit = DEFAULT_BATCH if batch is None else int(batch)
    if limit < 1:
        raise ValueError("path_counts: batch must be >= 1 pair (got %d)" % limit)
    per_batch = max(1, min(limit, _SEGMENT_MAX_EDGES) // window)  # samples
    seed = _seed(seed)
    dev, n, e = indptr.device, indptr.numel() - 1, indices.numel()
    total = passes * e
    keys = cnt = None
    for first in range(0, total, per_batch):
        row, col = _pairs(indptr, indices, window, first, min(per_batch, total - first), seed)
        keys, cnt = _merge(keys, cnt, *_batch_keys(row, col, n))
    if keys is None:
        return (torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.long, device=dev))
    if keys.numel() > _I32_MAX:
        raise _lib.BackendError("path_counts: the count matrix has %d cells; its CSR is int32 (limit 2^31 - 1)" % keys.numel())
    return _rowptr(keys // n, n), (keys % n).int(), cnt


def _rowptr(rows, n):
    rowptr = torch.zeros(n + 1, dtype=torch.long, device=rows.device)
    torch.cumsum(torch.bincount(rows, minlength=n), 0, out=rowptr[1:])
    return rowptr.int()


def _csr_args(name, rowptr, col, val, val_dtypes):
    for t in (rowptr, col, val):
        if not torch.is_tensor(t):
            raise _lib.BackendError("%s: rowptr / col / values must be tensors" % name)
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or val.dtype not in val_dtypes:
        raise _lib.BackendError("%s: rowptr / col must be int32 and the values one of %s (got %s / %s / %s)"
                                % (name, val_dtypes, rowptr.dtype, col.dtype, val.dtype))
    if rowptr.dim() != 1 or rowptr.numel() < 1 or col.dim() != 1 or val.shape != col.shape:
        raise _lib.BackendError("%s: not a CSR (rowptr [rows + 1], col [nnz], values [nnz])" % name)
    if col.device != rowptr.device or val.device != rowptr.device:
        raise _lib.BackendError("%s: tensors on different devices" % name)


def sparsifier(indptr, rowptr, col, count, window, passes, negative=1):
    """The NetSMF matrix of cogdl/models/emb/netsmf.py:90-106 from the count matrix C (canonical CSR, integer counts) of
    `passes` passes -> CSR (rowptr int32, col int32, val float32), columns ascending.  In closed form, with deg_i the length
    of row i of the graph and vol = E:
        W = C / (2 * window * passes),  colsum_j = sum_i W_ij
        X_ij = W_ij (i != j),  X_ii = deg_i - (colsum_i - W_ii)      (what `degree - laplacian(matrix)` is in scipy)
        M_ij = log max(1, X_ij * vol / (negative * deg_i * deg_j)),  entries equal to 0 dropped
    Row i and column i of a node with deg_i = 0 are empty; the reference divides by zero there (inf / nan).
    Elementwise work on the matrix's device in float64 (column sums are integer sums: equal from run to run); the result is
    rounded to float32 once."""
    if not torch.is_tensor(indptr) or indptr.dtype != torch.long or indptr.dim() != 1 or indptr.numel() < 1:
        raise _lib.BackendError("sparsifier: indptr must be a 1-D int64 tensor")
    _csr_args("sparsifier", rowptr, col, count, (torch.int64, torch.int32))
    n = indptr.numel() - 1
    if rowptr.numel() != n + 1 or rowptr.device != indptr.device:
        raise _lib.BackendError("sparsifier: the count matrix must have the graph's %d rows and live on its device" % n)
    window, passes, negative = int(window), int(passes), float(negative)
    if window < 1 or passes < 1 or not negative > 0:
        raise ValueError("sparsifier: window and passes must be >= 1 and negative > 0 (got %d, %d, %r)"
                         % (window, passes, negative))
    dev = indptr.device
    deg = indptr[1:] - indptr[:-1]
    vol = float(int(indptr[-1]) - int(indptr[0]))
    scale = 1.0 / (2.0 * window * passes)
    cnt = count.long()
    rows = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).long())
    cols = col.long()
    colsum = torch.zeros(n, dtype=torch.long, device=dev).index_add_(0, cols, cnt)
    # the pattern of X: the cells of C and the diagonal of every node that has a degree; sorted by (row, column)
    diag = torch.nonzero(deg > 0).flatten()
    keys_c = rows * n + cols
    keys = torch.unique(torch.cat([keys_c, diag * (n + 1)]))
    x = torch.zeros(keys.numel(), dtype=torch.float64, device=dev)
    x[torch.searchsorted(keys, keys_c)] = cnt.double() * scale
    pos_d = torch.searchsorted(keys, diag * (n + 1))
    x[pos_d] = deg[diag].double() - (colsum[diag].double() * scale - x[pos_d])
    r, c = keys // n, keys % n
    dr, dc = deg[r].double(), deg[c].double()
    pre = x * vol / (negative * dr * dc)
    keep = (dr > 0) & (dc > 0) & (pre > 1.0)
    r, c, pre = r[keep], c[keep], pre[keep]
    return _rowptr(r, n), c.int(), torch.log(pre).float()


def _transpose(rowptr, col, val, n):
    """CSR of the transpose of an [n, n] CSR."""
    if val.device.type == "cuda":
        from ..plan import csr2csc, gather_rows

        t = csr2csc(rowptr, col, n)
        return t.colptr, t.rowind, gather_rows(t.perm, val)
    rows = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).long())
    order = torch.sort(col.long(), stable=True).indices
    return _rowptr(col.long(), n), rows[order].int(), val[order].contiguous()


def _product(rowptr, col, val, x):
    if x.device.type == "cuda":
        from .spmm import csrspmm

        return csrspmm(rowptr, col, x, val)
    # (the host SpMM behind operators/spmm.py::spmm_cpu, called directly: importing that module loads libcogdl_hip.so)
    x = x.contiguous()
    out = torch.empty((rowptr.numel() - 1, x.shape[1]), dtype=torch.float32)
    rc = _lib.host().cogdl_host_csr_spmm_f32(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(x), _lib.ptr(out),
                                             rowptr.numel() - 1, x.shape[1], torch.get_num_threads())
    _lib.check_host(rc, "csr_spmm_cpu")
    return out


def _gram(y):
    """y^T y in float64: the matmul on y's device, the small result on the host."""
    yd = y.double()
    return (yd.t() @ yd).cpu()


def _cholesky_qr2(y):
    """CholeskyQR2: twice, y <- y R^-1 with R the Cholesky factor of the Gram matrix (float64, host; shifted by 1e-12 of
    its largest diagonal entry so that a rank-deficient y factors too: the second pass then sees a well-conditioned basis
    and leaves it orthonormal).  The [n, l] x [l, l] products run on y's device."""
    for _ in range(2):
        g = _gram(y)
        top = float(g.diagonal().max()) if g.numel() else 0.0
        if not top > 0.0:
            return y
        g = g + 1e-12 * top * torch.eye(g.shape[0], dtype=torch.float64)
        r = torch.linalg.cholesky(g).t()
        r_inv = torch.linalg.solve_triangular(r, torch.eye(g.shape[0], dtype=torch.float64), upper=True)
        y = y @ r_inv.float().to(y.device)
    return y


def randomized_svd(rowptr, col, val, n, k, n_iter=5, oversample=10, seed=None):
    """The k leading left singular vectors and singular values of the [n, n] CSR matrix M (int32 rowptr / col, float32 val)
    by the randomized range finder of Halko, Martinsson and Tropp (what sklearn's randomized_svd runs for the reference,
    netsmf.py:128) -> U float32 [n, k], S float32 [k] (descending) on the matrix's device.

    A Gaussian [n, l] test matrix, l = min(n, k + oversample), from a torch.Generator seeded with `seed` (drawn on the host,
    so GPU and CPU start from the same matrix); n_iter rounds of Q <- orth(M Q), Q <- orth(M^T Q), then Q <- orth(M Q).
    The products run through csrspmm on M and on its csr2csc transpose (the host SpMM and a sorted transpose on the CPU).  orth
    is CholeskyQR2 (sklearn uses LU there, a normalisation of the same purpose): the [l, l] Gram matrix by a matmul on the
    device, its Cholesky factor in float64 on the host -- no device solver library.  The final problem B = Q^T M, [l, n],
    is solved from its small side: torch.linalg.svd of the [l, l] matrix B B^T = (M^T Q)^T (M^T Q) on the host in float64,
    after an eigen-decomposition of Q^T Q that drops directions below 1e-6 of the largest (a matrix of rank < l leaves
    such), so U = Q (W V) has orthonormal columns.  Singular values beyond the rank come out as 0 with zero columns of U."""
    _csr_args("randomized_svd", rowptr, col, val, (torch.float32,))
    n, k, n_iter, oversample = int(n), int(k), int(n_iter), int(oversample)
    if rowptr.numel() != n + 1:
        raise _lib.BackendError("randomized_svd: rowptr has %d entries for n = %d" % (rowptr.numel(), n))
    if not 1 <= k <= n:
        raise ValueError("randomized_svd: k must be in [1, n = %d] (got %d)" % (n, k))
    if n_iter < 0 or oversample < 0:
        raise ValueError("randomized_svd: n_iter and oversample must be >= 0 (got %d, %d)" % (n_iter, oversample))
    dev = val.device
    rowptr, col, val = rowptr.contiguous(), col.contiguous(), val.contiguous()
    ell = min(n, k + oversample)
    gen = torch.Generator().manual_seed(_seed(seed) % (2 ** 63))
    with torch.no_grad():
        t_rowptr, t_col, t_val = _transpose(rowptr, col, val, n)
        q = torch.randn(n, ell, generator=gen, dtype=torch.float32).to(dev)
        for _ in range(n_iter):
            q = _cholesky_qr2(_product(rowptr, col, val, q))
            q = _cholesky_qr2(_product(t_rowptr, t_col, t_val, q))
        q = _cholesky_qr2(_product(rowptr, col, val, q))
        z = _product(t_rowptr, t_col, t_val, q)  # B^T
        lam, v = torch.linalg.eigh(_gram(q))
        u = torch.zeros(n, k, dtype=torch.float32, device=dev)
        s = torch.zeros(k, dtype=torch.float32, device=dev)
        good = lam > 1e-6 * max(float(lam.max()), 0.0) if lam.numel() else lam > 0
        if bool(good.any()) and float(lam.max()) > 0.0:
            w = v[:, good] / lam[good].sqrt()  # Q W has orthonormal columns
            small = w.t() @ _gram(z) @ w
            uu, ss, _ = torch.linalg.svd((small + small.t()) / 2)
            p = min(k, ss.numel())
            u[:, :p] = q @ (w @ uu[:, :p]).float().to(dev)
            s[:p] = ss[:p].clamp_min(0).sqrt().float().to(dev)
            dead = s <= 0
            u[:, dead] = 0
    return u, s
