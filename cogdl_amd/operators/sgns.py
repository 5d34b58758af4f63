"""Skip-gram training with negative sampling (SGNS) over rows of token ids: the trainer behind
`gensim.models.Word2Vec(walks, sg=1, negative=K)` as the reference's deepwalk / node2vec call it
(cogdl/models/emb/deepwalk.py:54-80, node2vec.py:72-103).

Walks on the GPU go to the HIP kernel (cogdl_hip_sgns_train, csrc/sgns.hip) and the tables stay there; walks on the CPU go
to the host twin in libcogdl_host.so, and libcogdl_hip.so is not loaded.  Both run the law of csrc/sgns_law.h.

  * `workers=1` is the serial mode: rows in order on one wave (GPU) or one thread (host); both return the same tables, bit
    for bit, and the same from run to run.  It is slow by construction, like gensim, which is reproducible only with one
    worker.  Any other value is the throughput mode: rows run concurrently and update the tables without locks, so results
    differ from run to run.  On the GPU, rows go in launches of ROWS_IN_FLIGHT rows, in row order.
  * The subsampling thresholds and the noise table follow gensim's formulas and are built here, once, in float64 on the
    CPU from the token counts, so both sides read the same tables.
  * An id >= num_nodes, or a malformed noise table, raises BackendError and the tables are not touched; nothing is read
    out of bounds.  Negative ids are padding.
  * `seed=None` draws the seed from torch's default generator, as the walk operators do.
"""
import numpy as np
import torch

from .. import _lib
from .walk import _seed

# Rows per launch of the GPU's throughput mode (0 = the library's default, 8192; profiles/sgns_bench.txt).
ROWS_IN_FLIGHT = 0

MAX_DIM, MAX_WINDOW, MAX_NEGATIVE, MAX_LENGTH = 512, 32, 16, 1024
_FLAG_TEXT = ((1, "an id lies outside [0, %d)"), (2, "the noise table is not non-decreasing with a positive last entry (%d ids)"))
_EXP_TABLE = None


def exp_table():
    """word2vec.c's 1000-entry sigmoid table over [-6, 6), built in double and rounded once."""
    global _EXP_TABLE
    if _EXP_TABLE is None:
        e = np.exp((np.arange(1000, dtype=np.float64) / 1000.0 * 2.0 - 1.0) * 6.0)
        _EXP_TABLE = torch.from_numpy((e / (e + 1.0)).astype(np.float32))
    return _EXP_TABLE


def build_tables(counts, sample=1e-3, ns_exponent=0.75):
    """(keep, cum) as int64 CPU tensors holding uint32 values, from the per-id token counts (float64 throughout).
    keep_prob = min(1, (sqrt(f / sample) + 1) * sample / f), f = count / total; cum[i] = round(sum_{<=i} count^ns_exponent /
    total * (2^31 - 1)), the last entry forced to 2^31 - 1."""
    c = np.asarray(counts, dtype=np.float64)
    total = c.sum()
    keep = np.full(c.shape, 2 ** 32 - 1, dtype=np.int64)
    if sample > 0 and total > 0:
        f = c / total
        with np.errstate(divide="ignore", invalid="ignore"):
            prob = np.where(c > 0, (np.sqrt(f / sample) + 1.0) * sample / f, 1.0)
        drop = prob < 1.0
        keep[drop] = np.floor(prob[drop] * 2.0 ** 32).astype(np.int64)
    p = c ** ns_exponent
    z = p.sum()
    cum = np.round(np.cumsum(p) / z * (2.0 ** 31 - 1)).astype(np.int64) if z > 0 else np.zeros(c.shape, dtype=np.int64)
    if z > 0:
        cum[-1] = 2 ** 31 - 1
    return torch.from_numpy(keep), torch.from_numpy(cum)


def _u32(t, dev):
    """int64 values in [0, 2^32) -> the same bits as an int32 tensor on `dev` (torch has no uint32 arithmetic)."""
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).to(dev).contiguous()


# ---- the checks and the bookkeeping the three trainers share (skipgram here, operators/pvdbow.py, operators/line.py)

def check_range(name, what, value, hi):
    if not 1 <= value <= hi:
        raise ValueError("%s: %s must be in [1, %d] (got %d)" % (name, what, hi, value))


def check_schedule(name, epochs, alpha, min_alpha, sample):
    if epochs < 1:
        raise ValueError("%s: epochs must be >= 1 (got %d)" % (name, epochs))
    if not (np.isfinite(alpha) and np.isfinite(min_alpha) and alpha > 0 and min_alpha >= 0):
        raise ValueError("%s: alpha must be positive and min_alpha non-negative (got %r, %r)" % (name, alpha, min_alpha))
    if not (np.isfinite(sample) and sample >= 0):
        raise ValueError("%s: sample must be >= 0 (got %r)" % (name, sample))


def check_workers(name, workers):
    if workers < 0:
        raise ValueError("%s: workers must be >= 0 (got %d)" % (name, workers))


def check_args(name, dim, window, negative, epochs, alpha, min_alpha, sample, workers, length):
    check_range(name, "dim", dim, MAX_DIM)
    check_range(name, "window", window, MAX_WINDOW)
    check_range(name, "negative", negative, MAX_NEGATIVE)
    check_schedule(name, epochs, alpha, min_alpha, sample)
    check_workers(name, workers)
    if length > MAX_LENGTH:
        raise ValueError("%s: rows of more than %d tokens are not supported (got %d)" % (name, MAX_LENGTH, length))


def check_init(init, rows, dim, dev, message):
    """Every table of `init` is a float32 [rows[i], dim] tensor on `dev`, or ValueError(message)."""
    for t, n in zip(init, rows):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (n, dim) or t.device != dev:
            raise ValueError(message)


def noise_tables(ids, num_ids, tables, sample, ns_exponent, dev):
    """(keep, cum) on `dev` in the kernels' uint32 format: the caller's `tables` (checked), or built from the counts of the
    valid `ids`."""
    if tables is None:
        valid = ids[(ids >= 0) & (ids < num_ids)]
        tables = build_tables(torch.bincount(valid, minlength=num_ids).cpu().numpy(), sample, ns_exponent)
    return _u32(tables[0], dev), _u32(tables[1], dev)


def check_tables(name, tables, num_ids):
    for t in tables or ():
        if not torch.is_tensor(t) or t.dtype != torch.long or tuple(t.shape) != (num_ids,):
            raise ValueError("%s: tables must be two int64 [%d] tensors" % (name, num_ids))


def trace_buffer(trace, width):
    """(records or None, the host twin's counter of applied targets) for `trace=n` records of `width` fields."""
    return (None if trace is None else torch.zeros((int(trace), width), dtype=torch.float64)), torch.zeros(1, dtype=torch.long)


def trace_records(name, records, n_rec):
    if records is None:
        return None
    if int(n_rec) > records.shape[0]:
        raise ValueError("%s: trace=%d is too small for %d applied targets" % (name, records.shape[0], int(n_rec)))
    return records[:int(n_rec)]


def raise_flags(name, flags, flag_text, num_ids):
    """The error word of a training call -> BackendError naming every raised flag.  Reading it is the call's one
    synchronisation."""
    bits = int(flags.item())
    if bits:
        raise _lib.BackendError("%s: %s" % (name, "; ".join(t % num_ids for bit, t in flag_text if bits & bit)))


def init_tables(num_nodes, dim, seed, device):
    """(syn0, syn1) float32 [V, dim]: syn0[v][d] = (u24(seed; v, d) / 2^24 - 0.5) / dim, syn1 = 0; equal on both sides."""
    device = torch.device(device)
    syn0 = torch.empty((num_nodes, dim), dtype=torch.float32, device=device)
    syn1 = torch.empty((num_nodes, dim), dtype=torch.float32, device=device)
    if device.type == "cuda":
        with _lib.on_device(device):
            rc = _lib.hip().cogdl_hip_sgns_init(_lib.ptr(syn0), _lib.ptr(syn1), num_nodes, dim, seed, _lib.stream_of(syn0))
        _lib.check(rc, "skipgram (init)")
    else:
        _lib.check_host(_lib.host().cogdl_host_sgns_init(_lib.ptr(syn0), _lib.ptr(syn1), num_nodes, dim, seed), "skipgram (init)")
    return syn0, syn1


def skipgram(walks, num_nodes, dim=128, window=5, negative=5, epochs=5, alpha=0.025, min_alpha=1e-4, sample=1e-3,
             ns_exponent=0.75, seed=None, workers=0, init=None, tables=None, trace=None):
    """-> (syn0, syn1) float32 [num_nodes, dim] on the device of `walks` (int64 [W, L]; negative ids are padding).
    `init=(syn0, syn1)` continues from tables of the caller's (they are copied, not modified).  `tables=(keep, cum)`
    replaces the tables built from the counts (int64 tensors of uint32 values).  `trace=n` (CPU walks, workers=1 only)
    returns a third value: the float64 [applied targets, 6] records (epoch, row, input id, target id, label, lr), which
    must number at most n."""
    if not torch.is_tensor(walks) or walks.dtype != torch.long or walks.dim() != 2:
        raise ValueError("skipgram: walks must be an int64 [W, L] tensor")
    num_nodes, dim, window, negative, epochs, workers = int(num_nodes), int(dim), int(window), int(negative), int(epochs), int(workers)
    alpha, min_alpha, sample, ns_exponent = float(alpha), float(min_alpha), float(sample), float(ns_exponent)
    w, length = walks.shape
    if num_nodes < 1 or num_nodes > 2 ** 31 - 1:
        raise ValueError("skipgram: num_nodes must be in [1, 2^31) (got %d)" % num_nodes)
    if length < 1:
        raise ValueError("skipgram: walks must have at least one column")
    check_args("skipgram", dim, window, negative, epochs, alpha, min_alpha, sample, workers, length)
    rows_in_flight = int(ROWS_IN_FLIGHT)
    if rows_in_flight < 0:
        raise ValueError("skipgram: ROWS_IN_FLIGHT must be >= 0 (got %d)" % rows_in_flight)
    dev = walks.device
    if trace is not None and (dev.type != "cpu" or workers != 1):
        raise ValueError("skipgram: trace needs CPU walks and workers=1")
    if init is not None:
        check_init(init, (num_nodes, num_nodes), dim, dev, "skipgram: init must be two float32 [%d, %d] tensors on %s" % (num_nodes, dim, dev))
    check_tables("skipgram", tables, num_nodes)
    seed = _seed(seed)
    walks = walks.contiguous()
    keep, cum = noise_tables(walks, num_nodes, tables, sample, ns_exponent, dev)
    table = exp_table().to(dev)
    if init is None:
        syn0, syn1 = init_tables(num_nodes, dim, seed, dev)
    else:
        syn0, syn1 = init[0].clone().contiguous(), init[1].clone().contiguous()
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    records = None
    if dev.type == "cuda":
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_sgns_train(_lib.ptr(walks), w, length, num_nodes, dim, window, negative, epochs, alpha,
                                                 min_alpha, _lib.ptr(keep), _lib.ptr(cum), _lib.ptr(table), seed, workers,
                                                 rows_in_flight, _lib.ptr(syn0), _lib.ptr(syn1), _lib.ptr(flags),
                                                 _lib.stream_of(walks))
        _lib.check(rc, "skipgram")
    else:
        records, n_rec = trace_buffer(trace, 6)
        rc = _lib.host().cogdl_host_sgns_train(_lib.ptr(walks), w, length, num_nodes, dim, window, negative, epochs, alpha,
                                               min_alpha, _lib.ptr(keep), _lib.ptr(cum), _lib.ptr(table), seed, workers,
                                               _lib.ptr(syn0), _lib.ptr(syn1), _lib.ptr(flags), _lib.ptr(records),
                                               0 if records is None else records.shape[0], _lib.ptr(n_rec))
        _lib.check_host(rc, "skipgram")
        records = trace_records("skipgram", records, n_rec)
    raise_flags("skipgram", flags, _FLAG_TEXT, num_nodes)
    return (syn0, syn1) if trace is None else (syn0, syn1, records)
