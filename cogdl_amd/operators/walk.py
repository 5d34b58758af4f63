"""Random walks on a CSR graph: `random_walk` (first order, with restart: the contract of RandomWalker.walk,
cogdl/utils/sampling.py:46-67) and `node2vec_walk` (second order with return parameter p and in-out parameter q on an
unweighted graph: the transition weights of cogdl/models/emb/node2vec.py:143-156).

A graph on the GPU goes to the HIP kernels (cogdl_hip_random_walk / cogdl_hip_node2vec_walk, csrc/walk.hip) and the walks
stay there; a graph on the CPU goes to the host twin in libcogdl_host.so (OpenMP over the walkers), and libcogdl_hip.so is
not loaded.  Both read their draws from csrc/walk_draw.h: for equal inputs and seed they return the same array.

Rules the reference leaves open or that are easy to get wrong (include/cogdl_hip.h has the full contract):
  * a restart lands on a uniformly drawn out-neighbour of the START node, not on the start itself (as in the reference);
  * at a node without out-neighbours the walker stays and the node is repeated (the reference is undefined there);
  * node2vec ignores edge weights; its membership test needs rows sorted by column -- unsorted rows are sorted once per
    structure here and the result is cached;
  * a start or neighbour id outside [0, N) raises BackendError; nothing is read out of bounds;
  * `seed=None` draws the seed from torch's default generator: `torch.manual_seed` makes a run reproducible, successive
    calls differ.
"""
import collections
import weakref

import torch

from .. import _lib

# node2vec: rejection trials per step before the exact pass over the row (0 = the library's default, 256).  A tuning
# constant, not a semantic one: the law sampled is the same for every value >= 1.
NODE2VEC_TRIALS = 0

_FLAG_TEXT = ((1, "a start id lies outside [0, %d)"), (2, "a neighbour id lies outside [0, %d)"),
              (4, "indptr does not describe rows inside indices (%d nodes)"))


def _graph_args(name, indptr, indices, start, length):
    if not (torch.is_tensor(indptr) and torch.is_tensor(indices)):
        raise _lib.BackendError("%s: indptr / indices must be tensors" % name)
    if indptr.dtype != torch.long or indices.dtype != torch.long:
        raise _lib.BackendError("%s: indptr / indices must be int64 (got %s / %s)" % (name, indptr.dtype, indices.dtype))
    if indptr.dim() != 1 or indices.dim() != 1 or indptr.numel() < 1:
        raise _lib.BackendError("%s: indptr / indices must be 1-D (indptr non-empty)" % name)
    if indices.device != indptr.device:
        raise _lib.BackendError("%s: tensors on different devices: %s vs %s" % (name, indptr.device, indices.device))
    if not torch.is_tensor(start):
        start = torch.as_tensor(start, dtype=torch.long, device=indptr.device)
    if start.dtype != torch.long:
        raise _lib.BackendError("%s: start must be int64 (got %s)" % (name, start.dtype))
    if start.device != indptr.device:
        raise _lib.BackendError("%s: tensors on different devices: %s vs %s" % (name, indptr.device, start.device))
    if start.dim() != 1:
        raise _lib.BackendError("%s: start must be 1-D" % name)
    length = int(length)
    if length < 1 or length > 2 ** 31 - 1:
        raise ValueError("%s: length must be in [1, 2^31) (got %d)" % (name, length))
    return indptr.contiguous(), indices.contiguous(), start.contiguous(), length


def _seed(seed):
    if seed is None:
        return int(torch.randint(0, 2 ** 62, (1,)).item())
    return int(seed) & (2 ** 64 - 1)


def raise_for_flags(name, flags, num_nodes):
    """BackendError for a non-zero flags word of a walk (an int, or the 1-element tensor the call filled)."""
    flags = int(flags)
    if flags:
        raise _lib.BackendError("%s: %s" % (name, "; ".join(t % num_nodes for bit, t in _FLAG_TEXT if flags & bit)))


def _out(name, out, w, length, dev):
    if out is None:
        return torch.empty((w, length), dtype=torch.long, device=dev)
    if (not torch.is_tensor(out) or out.dtype != torch.long or out.device != dev or tuple(out.shape) != (w, length)
            or not out.is_contiguous()):
        raise _lib.BackendError("%s: out must be a contiguous int64 [%d, %d] tensor on %s" % (name, w, length, dev))
    return out


def random_walk(indptr, indices, start, length, restart_p=0.0, seed=None, out=None, check=True, flags=None):
    """-> int64 [len(start), length] on the graph's device.  `out` (preallocated result), `check=False` (no read-back of
    the flags word: nothing synchronises, so the call can be captured in a hipGraph) and `flags` (a 1-element int32 tensor
    on the device to receive the flags word; check it later with raise_for_flags) are for captured steps."""
    indptr, indices, start, length = _graph_args("random_walk", indptr, indices, start, length)
    restart_p = float(restart_p)
    if not 0.0 <= restart_p <= 1.0:
        raise ValueError("random_walk: restart_p must be in [0, 1] (got %r)" % restart_p)
    seed = _seed(seed)
    dev, n, e, w = indptr.device, indptr.numel() - 1, indices.numel(), start.numel()
    walks = _out("random_walk", out, w, length, dev)
    if flags is None:
        flags = torch.empty(1, dtype=torch.int32, device=dev)
    elif not torch.is_tensor(flags) or flags.dtype != torch.int32 or flags.device != dev or flags.numel() != 1:
        raise _lib.BackendError("random_walk: flags must be a 1-element int32 tensor on %s" % dev)
    if dev.type == "cuda":
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_random_walk(_lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(start), w, length,
                                                  restart_p, seed, _lib.ptr(walks), _lib.ptr(flags), _lib.stream_of(indptr))
        _lib.check(rc, "random_walk")
    else:
        rc = _lib.host().cogdl_host_random_walk(_lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(start), w, length,
                                                restart_p, seed, _lib.ptr(walks), _lib.ptr(flags))
        _lib.check_host(rc, "random_walk")
    if check:
        raise_for_flags("random_walk", flags.item(), n)  # the one synchronisation
    return walks


# Rows sorted by column, once per structure: keyed on the two tensor OBJECTS (weak references) and vouched for by their
# version counters, data pointers and sizes, like the identity memo of cogdl_amd/plan.py.  The value is the sorted indices
# tensor, or None when the rows were sorted already.
_SORTED = collections.OrderedDict()
_SORTED_MAX = 8


def _state(indptr, indices):
    return (indptr._version, indices._version, indptr.data_ptr(), indices.data_ptr(), indptr.numel(), indices.numel())


def sorted_rows(indptr, indices):
    """`indices` with every row sorted by column (the same tensor if it already is)."""
    key = (id(indptr), id(indices))
    hit = _SORTED.get(key)
    if hit is not None:
        if hit[0]() is indptr and hit[1]() is indices and hit[2] == _state(indptr, indices):
            _SORTED.move_to_end(key)
            return indices if hit[3] is None else hit[3]
        del _SORTED[key]
    n, e = indptr.numel() - 1, indices.numel()
    result = None
    if e > 1 and n > 0:
        if int(indptr[0]) != 0 or int(indptr[-1]) != e or bool((indptr[1:] < indptr[:-1]).any()):
            raise _lib.BackendError("node2vec_walk: indptr is not a row pointer over indices")
        row = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
        if bool(((row[1:] == row[:-1]) & (indices[1:] < indices[:-1])).any()):
            by_col = torch.sort(indices, stable=True).indices
            result = indices[by_col[torch.sort(row[by_col], stable=True).indices]].contiguous()
    try:
        _SORTED[key] = (weakref.ref(indptr), weakref.ref(indices), _state(indptr, indices), result)
    except TypeError:
        pass
    while len(_SORTED) > _SORTED_MAX:
        _SORTED.popitem(last=False)
    return indices if result is None else result


def node2vec_walk(indptr, indices, start, length, p=1.0, q=1.0, seed=None, return_fallback=False):
    """-> int64 [len(start), length] on the graph's device; with return_fallback=True also the int32 [len(start)] count of
    steps per walker that the exact pass decided (the rejection loop ran out of trials)."""
    indptr, indices, start, length = _graph_args("node2vec_walk", indptr, indices, start, length)
    p, q = float(p), float(q)
    if not (0.0 < p < 1e300) or not (0.0 < q < 1e300):
        raise ValueError("node2vec_walk: p and q must be positive and finite (got p=%r, q=%r)" % (p, q))
    trials = int(NODE2VEC_TRIALS)
    if trials < 0 or trials > 2 ** 20:
        raise ValueError("node2vec_walk: NODE2VEC_TRIALS must be in [0, 2^20] (got %d)" % trials)
    seed = _seed(seed)
    indices = sorted_rows(indptr, indices)
    dev, n, e, w = indptr.device, indptr.numel() - 1, indices.numel(), start.numel()
    walks = torch.empty((w, length), dtype=torch.long, device=dev)
    fallback = torch.empty(w, dtype=torch.int32, device=dev) if return_fallback else None
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    if dev.type == "cuda":
        with _lib.on_device(dev):
            rc = _lib.hip().cogdl_hip_node2vec_walk(_lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(start), w, length, p, q,
                                                    trials, seed, _lib.ptr(walks), _lib.ptr(fallback), _lib.ptr(flags),
                                                    _lib.stream_of(indptr))
        _lib.check(rc, "node2vec_walk")
    else:
        rc = _lib.host().cogdl_host_node2vec_walk(_lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(start), w, length, p, q,
                                                  trials, seed, _lib.ptr(walks), _lib.ptr(fallback), _lib.ptr(flags))
        _lib.check_host(rc, "node2vec_walk")
    raise_for_flags("node2vec_walk", flags.item(), n)
    return (walks, fallback) if return_fallback else walks
