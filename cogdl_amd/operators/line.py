"""Edge-sampled skip-gram training with negative sampling: the trainer of the LINE model, orders 1 and 2
(cogdl/models/emb/line.py:127-158, `_train_line`).

An edge table on the GPU goes to the HIP kernel (cogdl_hip_line_train, csrc/line.hip) and the tables stay there; an edge
table on the CPU goes to the host twin in libcogdl_host.so, and libcogdl_hip.so is not loaded.  Both run the law of
csrc/line_law.h: per sample an edge drawn in proportion to its weight, oriented by a fair coin, the positive target and
`negative` targets drawn in proportion to node_weight^0.75, the error applied to the input row at the end, a learning rate
that falls linearly to a floor of 1e-4 * alpha.

  * The update is the original LINE program's, not the reference's: target rows ARE updated (the reference's `_update`
    receives fancy-indexed copies, so its `vec_v += g * vec_u` changes a temporary), and for order 2 the context table is a
    table of its own that starts at zero (the reference's emb_context is the same array as emb_vertex, which makes its
    orders 1 and 2 one computation).  A negative equal to either endpoint is skipped (word2vec's rule; the original program
    trains it with label 0), and outside |f| < 6 the update still applies with the sigmoid at 0 or 1 (the original
    program's rule; word2vec skips).
  * `workers=1` is the serial mode: samples in order on one wave (GPU) or one thread (host); both return the same tables,
    bit for bit, and the same from run to run.  Slow by construction.  Any other value is the throughput mode: samples run
    concurrently and update the tables without locks, so results differ from run to run.  On the GPU, samples go in
    launches of SAMPLES_IN_FLIGHT samples, in sample order.
  * The edge table (float64 cumulative weights scaled to 2^52) and the node noise table (sgns.build_tables) are built here,
    once, on the CPU, so both sides read the same tables.
  * An endpoint outside [0, num_nodes), or a malformed table, raises BackendError and the tables are not touched; nothing
    is read out of bounds.
  * `seed=None` draws the seed from torch's default generator, as the walk operators do.
"""
import numpy as np
import torch

from .. import _lib
from . import sgns
from .walk import _seed

# Samples per launch of the GPU's throughput mode (0 = the library's default, 262144; profiles/line_bench.txt).
SAMPLES_IN_FLIGHT = 0

MAX_DIM, MAX_NEGATIVE = 512, 16
EDGE_TOTAL = 2 ** 52
_FLAG_TEXT = ((1, "an edge endpoint lies outside [0, %d)"),
              (2, "the node noise table is not non-decreasing with a positive last entry (%d ids)"),
              (4, "the edge table is not non-decreasing from >= 0 to a last entry in [1, 2^52] (%d ids)"))


def edge_table(edge_weight):
    """ecum as an int64 CPU tensor: round(cumsum(w) / sum(w) * 2^52) in float64, the last entry forced to 2^52."""
    w = np.asarray(edge_weight, dtype=np.float64)
    total = w.sum()
    ecum = np.round(np.cumsum(w) / total * float(EDGE_TOTAL)).astype(np.int64)
    ecum[-1] = EDGE_TOTAL
    return torch.from_numpy(ecum)


def weighted_degree(edges, num_nodes, edge_weight=None):
    """float64 numpy [num_nodes]: every edge adds its weight (1 without weights) to both endpoints, a self-loop twice."""
    e = edges.detach().cpu().numpy()
    w = np.ones(e.shape[0], dtype=np.float64) if edge_weight is None else np.asarray(edge_weight, dtype=np.float64)
    inside = ((e >= 0) & (e < num_nodes)).all(axis=1)  # (an endpoint outside the range is the backend's to flag)
    deg = np.zeros(num_nodes, dtype=np.float64)
    np.add.at(deg, e[inside, 0], w[inside])
    np.add.at(deg, e[inside, 1], w[inside])
    return deg


def line_train(edges, num_nodes, dim, order, samples, negative=5, alpha=0.025, edge_weight=None, node_weight=None, seed=None,
               workers=0, init=None, trace=None, tables=None):
    """-> emb (order 1) or (emb, ctx) (order 2), float32 [num_nodes, dim] on the device of `edges` (int64 [M, 2], the
    undirected edges).  `edge_weight` ([M], finite, >= 0, positive sum) weights the edge draw; `node_weight` ([num_nodes],
    default: the weighted degree) is raised to 0.75 for the negatives.  `init` (a tensor for order 1, a pair for order 2)
    continues from tables of the caller's (they are copied, not modified).  `trace=n` (CPU edges, workers=1 only) appends the
    float64 [applied targets, 5] records (sample, u, target, label, lr), which must number at most n.  `tables=(ecum or None,
    ncum)` replaces the tables built from the weights (int64 tensors; ncum holds uint32 values)."""
    if not torch.is_tensor(edges) or edges.dtype != torch.long or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("line_train: edges must be an int64 [M, 2] tensor")
    num_nodes, dim, order, samples, negative, workers = int(num_nodes), int(dim), int(order), int(samples), int(negative), int(workers)
    alpha = float(alpha)
    m = edges.shape[0]
    if m < 1:
        raise ValueError("line_train: edges must hold at least one edge")
    if num_nodes < 1 or num_nodes > 2 ** 31 - 1:
        raise ValueError("line_train: num_nodes must be in [1, 2^31) (got %d)" % num_nodes)
    sgns.check_range("line_train", "dim", dim, MAX_DIM)
    if order not in (1, 2):
        raise ValueError("line_train: order must be 1 or 2 (got %d)" % order)
    if samples < 0:
        raise ValueError("line_train: samples must be >= 0 (got %d)" % samples)
    sgns.check_range("line_train", "negative", negative, MAX_NEGATIVE)
    if not (np.isfinite(alpha) and alpha > 0):
        raise ValueError("line_train: alpha must be positive (got %r)" % alpha)
    sgns.check_workers("line_train", workers)
    in_flight = int(SAMPLES_IN_FLIGHT)
    if in_flight < 0:
        raise ValueError("line_train: SAMPLES_IN_FLIGHT must be >= 0 (got %d)" % in_flight)
    dev = edges.device
    if trace is not None and (dev.type != "cpu" or workers != 1):
        raise ValueError("line_train: trace needs CPU edges and workers=1")
    if edge_weight is not None:
        edge_weight = torch.as_tensor(edge_weight).detach().cpu().double().numpy()
        if edge_weight.shape != (m,) or not np.isfinite(edge_weight).all() or (edge_weight < 0).any() or not edge_weight.sum() > 0:
            raise ValueError("line_train: edge_weight must be %d finite weights >= 0 with a positive sum" % m)
    if node_weight is not None:
        node_weight = torch.as_tensor(node_weight).detach().cpu().double().numpy()
        if node_weight.shape != (num_nodes,) or not np.isfinite(node_weight).all() or (node_weight < 0).any():
            raise ValueError("line_train: node_weight must be %d finite weights >= 0" % num_nodes)
    if init is not None:
        init = (init,) if torch.is_tensor(init) else tuple(init)
        if len(init) != order:
            raise ValueError("line_train: init must hold %d table(s) for order %d" % (order, order))
        sgns.check_init(init, (num_nodes,) * order, dim, dev, "line_train: init must be float32 [%d, %d] on %s" % (num_nodes, dim, dev))
    if tables is not None:
        if (len(tables) != 2 or not torch.is_tensor(tables[1]) or tables[1].dtype != torch.long or tuple(tables[1].shape) != (num_nodes,)
                or (tables[0] is not None and (not torch.is_tensor(tables[0]) or tables[0].dtype != torch.long
                                               or tuple(tables[0].shape) != (m,)))):
            raise ValueError("line_train: tables must be (None or int64 [%d], int64 [%d])" % (m, num_nodes))
    seed = _seed(seed)
    eu, ev = edges[:, 0].contiguous(), edges[:, 1].contiguous()
    if tables is None:
        ecum = None if edge_weight is None else edge_table(edge_weight)
        if node_weight is None:
            node_weight = weighted_degree(edges, num_nodes, edge_weight)
        ncum = sgns.build_tables(node_weight, sample=0, ns_exponent=0.75)[1]
    else:
        ecum, ncum = tables
    ecum = None if ecum is None else ecum.to(dev).contiguous()
    ncum = sgns._u32(ncum, dev)
    table = sgns.exp_table().to(dev)
    if init is None:
        emb, ctx = sgns.init_tables(num_nodes, dim, seed, dev)
    else:
        emb = init[0].clone().contiguous()
        ctx = init[1].clone().contiguous() if order == 2 else None
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    records = None
    if dev.type == "cuda":
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_line_train(_lib.ptr(eu), _lib.ptr(ev), _lib.ptr(ecum), m, num_nodes, _lib.ptr(ncum),
                                                 _lib.ptr(table), dim, negative, order, samples, alpha, seed, workers, in_flight,
                                                 _lib.ptr(emb), _lib.ptr(ctx) if order == 2 else None, _lib.ptr(flags),
                                                 _lib.stream_of(edges))
        _lib.check(rc, "line_train")
    else:
        records, n_rec = sgns.trace_buffer(trace, 5)
        rc = _lib.host().cogdl_host_line_train(_lib.ptr(eu), _lib.ptr(ev), _lib.ptr(ecum), m, num_nodes, _lib.ptr(ncum),
                                               _lib.ptr(table), dim, negative, order, samples, alpha, seed, workers, _lib.ptr(emb),
                                               _lib.ptr(ctx) if order == 2 else None, _lib.ptr(flags), _lib.ptr(records),
                                               0 if records is None else records.shape[0], _lib.ptr(n_rec))
        _lib.check_host(rc, "line_train")
        records = sgns.trace_records("line_train", records, n_rec)
    sgns.raise_flags("line_train", flags, _FLAG_TEXT, num_nodes)
    out = emb if order == 1 else (emb, ctx)
    if trace is None:
        return out
    return (emb, records) if order == 1 else (emb, ctx, records)
