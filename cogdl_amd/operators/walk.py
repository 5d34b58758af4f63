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

`metapath_walk` follows a node-type schema (the step of cogdl/models/emb/metapath2vec.py:87-106; gatne.py and hin2vec.py use
the same one) on the typed row layout of `typed_rows`: every row reordered by the type of the neighbour, so "a uniform neighbour
of the wanted type" is two dependent loads whatever the degree.  Same twins (cogdl_hip_metapath_walk /
cogdl_host_metapath_walk, step_metapath of csrc/walk_draw.h), same draws: with one type and no dead ends it returns
random_walk's array.  Unlike the walks above it ENDS where no neighbour has the wanted type, as the reference does: the rest of
the row holds -1.
"""
import collections
import weakref

import torch

from .. import _lib

# node2vec: rejection trials per step before the exact pass over the row (0 = the library's default, 256).  A tuning
# constant, not a semantic one: the law sampled is the same for every value >= 1.
NODE2VEC_TRIALS = 0

_FLAG_TEXT = ((1, "a start id lies outside [0, %d)"), (2, "a neighbour id lies outside [0, %d)"),
              (4, "indptr does not describe rows inside indices (%d nodes)"),
              (8, "a start node's type is not the first type of its metapath (%d nodes)"),
              (16, "a wanted type or a metapath id lies outside its range (%d nodes)"))


def _graph_checks(name, indptr, indices):
    """What every operator on an int64 CSR graph checks first (operators/netsmf.py too)."""
    if not (torch.is_tensor(indptr) and torch.is_tensor(indices)):
        raise _lib.BackendError("%s: indptr / indices must be tensors" % name)
    if indptr.dtype != torch.long or indices.dtype != torch.long:
        raise _lib.BackendError("%s: indptr / indices must be int64 (got %s / %s)" % (name, indptr.dtype, indices.dtype))
    if indptr.dim() != 1 or indices.dim() != 1 or indptr.numel() < 1:
        raise _lib.BackendError("%s: indptr / indices must be 1-D (indptr non-empty)" % name)
    if indices.device != indptr.device:
        raise _lib.BackendError("%s: tensors on different devices: %s vs %s" % (name, indptr.device, indices.device))


def _graph_args(name, indptr, indices, start, length):
    _graph_checks(name, indptr, indices)
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
    _lib.twin_call("random_walk", dev, _lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(start), w, length, restart_p, seed,
                   _lib.ptr(walks), _lib.ptr(flags))
    if check:
        raise_for_flags("random_walk", flags.item(), n)  # the one synchronisation
    return walks


class _StructureMemo:
    """Something derived from a graph's structure, once per structure: keyed on two or three tensor OBJECTS (weak references,
    plus a hashable `extra`) and vouched for by their version counters, data pointers and sizes, like the identity memo of
    cogdl_amd/plan.py.  The `limit` most recently used entries are kept.  A value holds None in place of the caller's own
    tensors: the memo must not keep them alive."""

    def __init__(self, limit=8):
        self._entries, self._limit = collections.OrderedDict(), limit

    def find(self, a, b, c=None, extra=None):
        """-> (True, the value put for these tensor objects in their present state) or (False, the ticket to hand to put).
        Runs in front of every launch, hence the unrolled compares."""
        key = (id(a), id(b), id(c), extra)
        state = (a._version, a.data_ptr(), a.numel(), b._version, b.data_ptr(), b.numel(),
                 None if c is None else (c._version, c.data_ptr(), c.numel()))
        hit = self._entries.get(key)
        if hit is not None:
            if hit[0] == state and hit[1]() is a and hit[2]() is b and (c is None or hit[3]() is c):
                self._entries.move_to_end(key)
                return True, hit[4]
            del self._entries[key]
        return False, (key, state, a, b, c)

    def put(self, ticket, value):
        key, state, a, b, c = ticket
        try:
            self._entries[key] = (state, weakref.ref(a), weakref.ref(b), None if c is None else weakref.ref(c), value)
        except TypeError:
            pass
        while len(self._entries) > self._limit:
            self._entries.popitem(last=False)

    def clear(self):
        self._entries.clear()


_SORTED = _StructureMemo()  # (indptr, indices) -> the sorted indices tensor, or None when the rows were sorted already


def sorted_rows(indptr, indices):
    """`indices` with every row sorted by column (the same tensor if it already is)."""
    found, memo = _SORTED.find(indptr, indices)
    if found:
        return indices if memo is None else memo
    n, e = indptr.numel() - 1, indices.numel()
    result = None
    if e > 1 and n > 0:
        if int(indptr[0]) != 0 or int(indptr[-1]) != e or bool((indptr[1:] < indptr[:-1]).any()):
            raise _lib.BackendError("node2vec_walk: indptr is not a row pointer over indices")
        row = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
        if bool(((row[1:] == row[:-1]) & (indices[1:] < indices[:-1])).any()):
            by_col = torch.sort(indices, stable=True).indices
            result = indices[by_col[torch.sort(row[by_col], stable=True).indices]].contiguous()
    _SORTED.put(memo, result)
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
    _lib.twin_call("node2vec_walk", dev, _lib.ptr(indptr), _lib.ptr(indices), n, e, _lib.ptr(start), w, length, p, q, trials,
                   seed, _lib.ptr(walks), _lib.ptr(fallback), _lib.ptr(flags))
    raise_for_flags("node2vec_walk", flags.item(), n)
    return (walks, fallback) if return_fallback else walks


# ---------------------------------------------------------------------------------------------------- metapath walk
MAX_TYPES = 64
_TYPED = _StructureMemo()  # (indptr, indices, node_type), T -> (seg, indices_t, int32 types)


def _typed_layout(indptr, indices, node_type, num_types=None):
    name = "typed_rows"
    if not (torch.is_tensor(indptr) and torch.is_tensor(indices) and torch.is_tensor(node_type)):
        raise _lib.BackendError("%s: indptr / indices / node_type must be tensors" % name)
    if indptr.dtype != torch.long or indices.dtype != torch.long:
        raise _lib.BackendError("%s: indptr / indices must be int64 (got %s / %s)" % (name, indptr.dtype, indices.dtype))
    if node_type.dtype not in (torch.int32, torch.long):
        raise _lib.BackendError("%s: node_type must be int32 or int64 (got %s)" % (name, node_type.dtype))
    if indptr.dim() != 1 or indices.dim() != 1 or node_type.dim() != 1 or indptr.numel() < 1:
        raise _lib.BackendError("%s: indptr / indices / node_type must be 1-D (indptr non-empty)" % name)
    if indices.device != indptr.device or node_type.device != indptr.device:
        raise _lib.BackendError("%s: tensors on different devices: %s, %s, %s" % (name, indptr.device, indices.device, node_type.device))
    if not (indptr.is_contiguous() and indices.is_contiguous() and node_type.is_contiguous()):
        raise _lib.BackendError("%s: indptr / indices / node_type must be contiguous" % name)
    n, e = indptr.numel() - 1, indices.numel()
    if node_type.numel() != n:
        raise _lib.BackendError("%s: node_type must have one entry per node (%d, got %d)" % (name, n, node_type.numel()))
    if num_types is None:
        num_types = int(node_type.max()) + 1 if n else 1
    t = int(num_types)
    if t < 1 or t > MAX_TYPES:
        raise _lib.BackendError("%s: the number of node types must be in [1, %d] (got %d)" % (name, MAX_TYPES, t))
    if n * t > 2 ** 31 - 2:
        raise _lib.BackendError("%s: nodes x types = %d exceeds 2^31 - 2" % (name, n * t))
    found, memo = _TYPED.find(indptr, indices, node_type, t)
    if found:
        seg, indices_t, types32 = memo  # (None: the caller's own tensor)
        return (indptr if seg is None else seg, indices if indices_t is None else indices_t,
                node_type if types32 is None else types32)
    if n and (int(node_type.min()) < 0 or int(node_type.max()) >= t):
        raise _lib.BackendError("%s: a node type lies outside [0, %d)" % (name, t))
    if int(indptr[0]) != 0 or int(indptr[-1]) != e or (n and bool((indptr[1:] < indptr[:-1]).any())):
        raise _lib.BackendError("%s: indptr is not a row pointer over indices" % name)
    if e and (int(indices.min()) < 0 or int(indices.max()) >= n):
        raise _lib.BackendError("%s: a neighbour id lies outside [0, %d)" % (name, n))
    types32 = node_type if node_type.dtype == torch.int32 else node_type.to(torch.int32)
    if t == 1:
        value = (indptr, indices, types32)
    else:
        from ..graph_build import coo2csr_index

        row = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
        seg, perm = coo2csr_index(row * t + node_type[indices].long(), None, n * t)  # stable: the order inside a type is kept
        value = (seg, indices[perm].contiguous(), types32)
    _TYPED.put(memo, (None if t == 1 else value[0], None if t == 1 else value[1], None if types32 is node_type else types32))
    return value


def typed_rows(indptr, indices, node_type, num_types=None):
    """-> (seg int64 [N * T + 1], indices_t): `indices` with every row reordered by the type of the neighbour (stable inside a
    type), indices_t[seg[v * T + t] : seg[v * T + t + 1]] the neighbours of v that have type t; seg[v * T] == indptr[v].
    T = num_types (default: max(node_type) + 1), at most 64.  With T == 1 the result is (indptr, indices) itself.  Built once
    per structure with coo2csr_index on the key row * T + node_type[col] and cached on the three tensor objects (weak
    references, vouched for by version counters and data pointers)."""
    return _typed_layout(indptr, indices, node_type, num_types)[:2]


def parse_schema(schema):
    """The reference's schema string ("0-1-0,0-2-0,1-0-2-0-1") or a list of integer lists -> list of integer lists.  Every
    metapath needs at least two items and must end on the type it starts with."""
    if isinstance(schema, str):
        try:
            paths = [[int(item) for item in path.split("-")] for path in schema.split(",")]
        except ValueError:
            raise ValueError("metapath_walk: schema items must be integers (got %r)" % schema) from None
    else:
        paths = []
        for path in schema:
            items = list(path)
            if any(isinstance(item, bool) or int(item) != item for item in items):
                raise ValueError("metapath_walk: schema items must be integers (got %r)" % (path,))
            paths.append([int(item) for item in items])
    if not paths:
        raise ValueError("metapath_walk: the schema holds no metapath")
    for path in paths:
        if len(path) < 2:
            raise ValueError("metapath_walk: a metapath needs at least two items (got %r)" % (path,))
        if path[0] != path[-1]:
            raise ValueError("metapath_walk: a metapath must end on the type it starts with (got %r)" % (path,))
    return paths


def metapath_walk(indptr, indices, node_type, start, schema, length, walker_path=None, seed=None, return_lengths=False):
    """Walks that follow a node-type schema (the rule of cogdl/models/emb/metapath2vec.py:87-106) -> int64 [len(start), length]
    on the graph's device.  Walker w follows metapath walker_path[w] of `schema` (one metapath: walker_path may be None); at
    position i it moves to a uniformly drawn neighbour of type items[i % (len(items) - 1)].  Where there is none the walk
    ends and the rest of the row holds -1 (padding for `skipgram`).  A start node must have the first type of its metapath.
    return_lengths=True also returns the int32 [len(start)] number of positions that hold a node."""
    name = "metapath_walk"
    paths = parse_schema(schema)
    indptr, indices, start, length = _graph_args(name, indptr, indices, start, length)
    if torch.is_tensor(node_type):
        node_type = node_type if node_type.is_contiguous() else node_type.contiguous()
    else:
        node_type = torch.as_tensor(node_type, device=indptr.device)
    seg, indices_t, types32 = _typed_layout(indptr, indices, node_type)
    dev, n, e, w = indptr.device, indptr.numel() - 1, indices.numel(), start.numel()
    t = (seg.numel() - 1) // n if n else 1
    for path in paths:
        if min(path) < 0 or max(path) >= t:
            raise ValueError("%s: a schema item lies outside [0, %d) (metapath %r)" % (name, t, path))
    if walker_path is None:
        if len(paths) != 1:
            raise ValueError("%s: walker_path is needed with %d metapaths" % (name, len(paths)))
        walker_path = torch.zeros(w, dtype=torch.int32, device=dev)
    else:
        if not torch.is_tensor(walker_path):
            walker_path = torch.as_tensor(walker_path, device=dev)
        if walker_path.dtype not in (torch.int32, torch.long) or walker_path.dim() != 1 or walker_path.numel() != w:
            raise _lib.BackendError("%s: walker_path must be an int32 or int64 [%d] tensor" % (name, w))
        if walker_path.device != dev:
            raise _lib.BackendError("%s: tensors on different devices: %s vs %s" % (name, dev, walker_path.device))
        if walker_path.dtype != torch.int32:
            if w and (int(walker_path.min()) < -2 ** 31 or int(walker_path.max()) >= 2 ** 31):
                raise _lib.BackendError("%s: a metapath id lies outside [0, %d)" % (name, len(paths)))
            walker_path = walker_path.to(torch.int32)
        walker_path = walker_path.contiguous()
    pattern = torch.tensor([item for path in paths for item in path[:-1]], dtype=torch.int32).to(dev)
    off = [0]
    for path in paths:
        off.append(off[-1] + len(path) - 1)
    path_off = torch.tensor(off, dtype=torch.int32).to(dev)
    seed = _seed(seed)
    walks = torch.empty((w, length), dtype=torch.long, device=dev)
    lengths = torch.empty(w, dtype=torch.int32, device=dev) if return_lengths else None
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.twin_call(name, dev, _lib.ptr(seg), _lib.ptr(indices_t), n, t, e, _lib.ptr(types32), _lib.ptr(start),
                   _lib.ptr(walker_path), w, length, _lib.ptr(pattern), _lib.ptr(path_off), len(paths), seed, _lib.ptr(walks),
                   _lib.ptr(lengths), _lib.ptr(flags))
    raise_for_flags(name, flags.item(), n)
    return (walks, lengths) if return_lengths else walks
