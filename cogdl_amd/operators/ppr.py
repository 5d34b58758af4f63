"""Top-k personalised PageRank by forward push on a CSR graph: `topk_ppr` (the contract of calc_ppr_topk_parallel,
cogdl/utils/ppr_utils.py:38-48, made deterministic) and `full_ppr` (every touched entry per source, for tests and for
callers that want the whole vector).

A graph on the GPU goes to the HIP kernel (cogdl_hip_ppr_topk, csrc/ppr.hip) and the result stays there; a graph on the CPU
goes to the host twin in libcogdl_host.so (OpenMP over the sources), and libcogdl_hip.so is not loaded.  Both run the
fixed-point arithmetic of csrc/ppr_fixed.h in the same synchronous rounds: for equal inputs they return the same arrays.

What the reference leaves open (include/cogdl_hip.h has the full contract):
  * the reference pushes in LIFO order and its values depend on that order; here round t pushes exactly the nodes whose
    residual is at or above alpha * eps * deg at the start of the round, and residuals are 64-bit fixed point, so the
    result is a function of the inputs alone.  Both lie in (pi - eps * deg, pi] on a symmetric structure;
  * the topk largest scores come first, ties go to the smaller node id (np.argsort leaves ties open);
  * deg[u] is the length of u's row: duplicate entries count, and receive, separately -- coalesce first if the reference's
    csr_matrix semantics are wanted (cogdl_amd/ppr_compat.py does);
  * (alpha, eps) whose rounding loss is not provably below 2^-24 raise ValueError (alpha * eps < 2^-20, mainly);
  * an id or a row of indptr outside its range raises BackendError; nothing is read out of bounds.
The workspace of the GPU call does not grow with the number of sources (a persistent grid owns one table per workgroup),
so a long source list needs no chunking; `full_ppr` cuts it only to bound its own output.
"""
import torch

from .. import _lib
from .walk import _graph_args

_FLAG_TEXT = ((1, "a source id lies outside [0, %d)"), (2, "a neighbour id lies outside [0, %d)"),
              (4, "indptr does not describe rows inside indices (%d nodes)"),
              (8, "a table overflowed: max_source_degree is below the degree of a source (%d nodes)"),
              (16, "the round bound was reached (%d nodes)"))


def raise_for_flags(name, flags, num_nodes):
    """BackendError for a non-zero flags word of a PPR call (an int, or the 1-element tensor the call filled)."""
    flags = int(flags)
    if flags:
        raise _lib.BackendError("%s: %s" % (name, "; ".join(t % num_nodes for bit, t in _FLAG_TEXT if flags & bit)))


def plan(num_nodes, num_edges, max_source_degree, alpha, eps):
    """What both twins derive from (alpha, eps) for a graph of this size: dict(budget, table_slots, max_rounds, lds).
    ValueError for parameters that are not accepted."""
    out = (_lib.ctypes.c_int64 * 4)()
    rc = _lib.host().cogdl_host_ppr_plan(int(num_nodes), int(num_edges), int(max_source_degree), float(alpha), float(eps),
                                         _lib.ctypes.addressof(out))
    if rc == 1:
        raise ValueError("ppr: alpha must be in (0, 1) and eps positive (got alpha=%r, eps=%r)" % (alpha, eps))
    if rc != 0:
        raise ValueError("ppr: (alpha=%r, eps=%r) is not accepted for %d edges: alpha * eps must be at least 2^-20, the "
                         "rounding loss 4 (E + 1 / (alpha eps)) / alpha * 2^-62 below 2^-24 and the table within 2^23 slots"
                         % (alpha, eps, num_edges))
    return {"budget": out[0], "table_slots": out[1], "max_rounds": out[2], "lds": bool(out[3])}


def _max_source_degree(indptr, sources, n, e):
    """An upper bound of deg[s] over the sources that is safe for any input (ids are clamped, the value too)."""
    if sources.numel() == 0 or n == 0:
        return 0
    s = sources.clamp(0, n - 1)
    return int((indptr[s + 1] - indptr[s]).max().clamp(0, e).item())


def topk_ppr(indptr, indices, sources, alpha, eps, topk, check=True, max_source_degree=None, return_stats=False):
    """-> (nbr int64 [S, topk], val float32 [S, topk], count int32 [S]) on the graph's device; unused slots are -1 / 0.
    `check=False` skips the read-back of the flags word; `max_source_degree` (an upper bound of the sources' degrees) saves
    the one read-back that sizes the tables.  return_stats=True adds an int32 [S, 2] tensor: rounds and touched nodes."""
    if int(topk) < 1:
        raise ValueError("topk_ppr: topk must be at least 1 (got %r)" % (topk,))
    indptr, indices, sources, topk = _graph_args("topk_ppr", indptr, indices, sources, topk)
    alpha, eps = float(alpha), float(eps)
    dev, n, e, s = indptr.device, indptr.numel() - 1, indices.numel(), sources.numel()
    if max_source_degree is None:
        max_source_degree = _max_source_degree(indptr, sources, n, e)
    max_source_degree = int(max_source_degree)
    plan(n, e, max_source_degree, alpha, eps)  # ValueError for rejected parameters
    nbr = torch.empty((s, topk), dtype=torch.long, device=dev)
    val = torch.empty((s, topk), dtype=torch.float32, device=dev)
    count = torch.empty(s, dtype=torch.int32, device=dev)
    stats = torch.empty((s, 2), dtype=torch.int32, device=dev) if return_stats else None
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    if dev.type == "cuda":
        with _lib.on_device(dev):
            ws_bytes = _lib.hip().cogdl_hip_ppr_topk_workspace_bytes(n, e, max_source_degree, alpha, eps, s)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            rc = _lib.hip().cogdl_hip_ppr_topk(_lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(sources), s, max_source_degree,
                                               alpha, eps, topk, _lib.ptr(nbr), _lib.ptr(val), _lib.ptr(count), _lib.ptr(stats),
                                               _lib.ptr(flags), _lib.ptr(ws), ws_bytes, _lib.stream_of(indptr))
        _lib.check(rc, "topk_ppr")
    else:
        rc = _lib.host().cogdl_host_ppr_topk(_lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(sources), s, max_source_degree,
                                             alpha, eps, topk, _lib.ptr(nbr), _lib.ptr(val), _lib.ptr(count), _lib.ptr(stats),
                                             _lib.ptr(flags))
        _lib.check_host(rc, "topk_ppr")
    if check:
        raise_for_flags("topk_ppr", flags.item(), n)
    return (nbr, val, count, stats) if return_stats else (nbr, val, count)


_FULL_ENTRIES = 1 << 24  # full_ppr: output entries per call of the operator


def full_ppr(indptr, indices, sources, alpha, eps):
    """Every entry with a positive score per source, in the order of `topk_ppr`, as a CSR triple
    (rowptr int64 [S + 1], nbr int64, val float32) on the graph's device.  A test and debugging facility: the selection
    costs O(entries^2 / 256) per source on the GPU, and sizes are read back."""
    indptr, indices, sources, _ = _graph_args("full_ppr", indptr, indices, sources, 1)
    n, e = indptr.numel() - 1, indices.numel()
    maxdeg = _max_source_degree(indptr, sources, n, e)
    width = max(1, min(n, plan(n, e, maxdeg, alpha, eps)["table_slots"] // 2))
    step = max(1, _FULL_ENTRIES // width)
    counts, nbrs, vals = [], [], []
    for lo in range(0, sources.numel(), step):
        nbr, val, count = topk_ppr(indptr, indices, sources[lo:lo + step], alpha, eps, width, max_source_degree=maxdeg)
        keep = torch.arange(width, device=nbr.device)[None, :] < count[:, None]
        counts.append(count.long())
        nbrs.append(nbr[keep])
        vals.append(val[keep])
    rowptr = torch.zeros(sources.numel() + 1, dtype=torch.long, device=indptr.device)
    if counts:
        rowptr[1:] = torch.cumsum(torch.cat(counts), 0)
        return rowptr, torch.cat(nbrs), torch.cat(vals)
    return rowptr, torch.empty(0, dtype=torch.long, device=indptr.device), torch.empty(0, dtype=torch.float32, device=indptr.device)
