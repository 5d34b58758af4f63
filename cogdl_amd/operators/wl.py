"""Weisfeiler-Lehman subtree relabelling on a batch of graphs: the refinement of the reference's
`Graph2Vec.wl_iterations` (cogdl/models/emb/graph2vec.py:63-78) as integers, without an md5 per node and round.

    wl_labels(indptr, indices, label0, rounds) -> (labels int32 [rounds + 1, N], classes int64 [rounds + 1])

`indptr` int32 [N + 1] / `indices` int32 [E] are the CSR of the disjoint union of the batch's graphs, taken as given:
multiplicity counts and a self-loop is a neighbour.  `label0` is an int32 or int64 [N] of arbitrary values.  The law
(csrc/wl_law.h): sig_0(v) = (label0[v]); sig_{r+1}(v) = (labels[r][v]; the neighbours' labels[r] in ascending order);
labels[r][v] numbers the classes of equal signatures by first occurrence over the whole batch, classes[r] counts them.

A CSR on the GPU goes to the HIP kernels (cogdl_hip_wl_labels, csrc/wl.hip): per round a gather-and-sort inside every row,
a salted 128-bit hash per node, a hash table that keeps the smallest node id per hash, and a verification of every node
against its representative element for element, so the result is exact; a hash collision raises BackendError, it is never
a wrong label.  A CSR on the CPU goes to the host twin (libcogdl_host.so; libcogdl_hip.so is not loaded), which compares
signatures outright.  Both return the same bytes.

  * A malformed indptr, an index outside [0, N) and a row of more than MAX_DEGREE = 32768 neighbours raise BackendError;
    nothing is read out of bounds.
  * `hash_bits` (1..128) is a test hook: the hash is cut to that many bits before it is used, which makes collisions
    happen.  The host twin emulates it: it raises where two different signatures share the truncated hash.  SALT is the
    hash's salt (any 64-bit value; the result does not depend on it).
  * One read-back of the flags word ends the call; it is not capturable in a hipGraph.
"""
import torch

from .. import _lib

MAX_DEGREE = 32768
SALT = 0
_FLAG_TEXT = ((1, "indptr does not run from 0 to the number of indices without decreasing"),
              (2, "an index lies outside [0, N)"),
              (4, "row too long: more than %d neighbours" % MAX_DEGREE),
              (8, "hash collision: two different signatures share a hash (hash_bits too small?)"),
              (16, "the hash table's probe bound was reached"))


def wl_labels(indptr, indices, label0, rounds, *, hash_bits=128):
    for name, t in (("indptr", indptr), ("indices", indices)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError("wl_labels: %s must be a 1-D int32 tensor" % name)
    if not torch.is_tensor(label0) or label0.dtype not in (torch.int32, torch.long) or label0.dim() != 1:
        raise ValueError("wl_labels: label0 must be a 1-D int32 or int64 tensor")
    rounds, hash_bits = int(rounds), int(hash_bits)
    if rounds < 0:
        raise ValueError("wl_labels: rounds must be >= 0 (got %d)" % rounds)
    if not 1 <= hash_bits <= 128:
        raise ValueError("wl_labels: hash_bits must be in [1, 128] (got %d)" % hash_bits)
    n, e, dev = indptr.numel() - 1, indices.numel(), indptr.device
    if n < 0 or label0.numel() != n:
        raise ValueError("wl_labels: indptr must have N + 1 entries and label0 N (got %d and %d)" % (n + 1, label0.numel()))
    if indices.device != dev or label0.device != dev:
        raise ValueError("wl_labels: indptr, indices and label0 must be on one device")
    indptr, indices, label0 = indptr.contiguous(), indices.contiguous(), label0.long().contiguous()
    labels = torch.empty((rounds + 1, n), dtype=torch.int32, device=dev)
    classes = torch.zeros(rounds + 1, dtype=torch.long, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    salt = int(SALT) & (2 ** 64 - 1)
    if dev.type == "cuda":
        lib = _lib.hip()
        ws, ws_bytes = _lib.workspace("cogdl_hip_wl_workspace_bytes", dev, n, e)
        with _lib.on_device(dev):
            rc = lib.cogdl_hip_wl_labels(_lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(label0), n, e, rounds, hash_bits, salt,
                                         _lib.ptr(labels), _lib.ptr(classes), _lib.ptr(flags), _lib.ptr(ws), ws_bytes,
                                         _lib.stream_of(indptr))
        _lib.check(rc, "wl_labels")
    else:
        rc = _lib.host().cogdl_host_wl_labels(_lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(label0), n, e, rounds, hash_bits, salt,
                                              _lib.ptr(labels), _lib.ptr(classes), _lib.ptr(flags))
        _lib.check_host(rc, "wl_labels")
    bits = int(flags.item())  # the one synchronisation
    if bits:
        raise _lib.BackendError("wl_labels: %s (flags %d)" % ("; ".join(t for bit, t in _FLAG_TEXT if bits & bit), bits))
    return labels, classes
