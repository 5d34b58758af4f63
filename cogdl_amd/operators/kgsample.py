"""One training batch of a knowledge-graph embedding model: positives, filtered negatives and subsampling weights.

    negative_batch(tables, mode, order, K, seed, first_sid, *, index_dtype=torch.int64, check=True)
                                                                                    -> (positive, negative, weight)
        tables     cogdl_amd.kgsample.train_tables(triples, num_entities): the true lists of every (relation, tail) and
                   (head, relation) group, the group of every triple and its subsampling weight, on one device
        mode       "head-batch" (the negatives replace the head) or "tail-batch"
        order      int32 / int64 [B]: the ids, in [0, T), of the batch's triples
        K          negatives per positive
        seed       any integer (taken modulo 2^64)
        first_sid  the ordinal, in this mode's stream, of the batch's first positive: row b is positive first_sid + b
        positive   int64 [B, 3]   triples[order]
        negative   index_dtype [B, K]: uniform, with repetition, over the entities that are NOT in the positive's true list
        weight     float32 [B]    tables.weight[order]

The reference makes this batch on the host, one positive at a time: 2 K numpy draws, np.in1d against the true list, repeated
until K survive, three tensors per positive, a collate of the batch and a copy to the device (cogdl/datasets/kg_data.py:98-135).
Here it is one launch.  The law is csrc/kgsample_law.h: negative j of positive sid is the r-th entity missing from the sorted
true list, r = mulhi64(Philox(seed, mode, sid, j), N - L), found by one binary search -- the reference's distribution without
its rejection loop, and a pure function of (seed, mode, sid, j), so a positive's negatives do not depend on how the stream is
cut into batches.  Tables on the GPU run the HIP kernel (csrc/kgsample.hip: one wave per positive, lists of at most LDS_LIST
ids searched in LDS, longer ones in global memory); tables on the CPU run the OpenMP host twin; the results are equal bit for
bit.

B == 0 or K == 0 returns empty tensors without a launch.  check=True reads the status word back once and raises BackendError
for an order id outside [0, T) or a list that leaves no entity free (such a row is written as -1); check=False skips the
read-back: nothing synchronises and nothing is allocated beyond the three outputs.
"""
import torch

from .. import _lib

LDS_LIST = 1024  # cogdl_kgsample::kLdsList: the longest true list the kernel stages in LDS
MODES = ("head-batch", "tail-batch")
TAGS = {"head-batch": 0x4B474E48, "tail-batch": 0x4B474E54}  # cogdl_kgsample::kTagHead / kTagTail

_STATUS_TEXT = ((1, "an order id lies outside [0, T)"), (2, "a true list leaves no entity free"),
                (4, "a group id or list bounds lie outside the tables"))


def raise_for_status(status):
    status = int(status)
    if status:
        raise _lib.BackendError("negative_batch: %s" % "; ".join(t for bit, t in _STATUS_TEXT if status & bit))


def negative_batch(tables, mode, order, K, seed, first_sid, *, index_dtype=torch.int64, check=True):
    """-> (positive int64 [B, 3], negative index_dtype [B, K], weight float32 [B]) on the tables' device; see the module
    docstring."""
    if mode not in MODES:
        raise ValueError("negative_batch: mode %s not supported" % (mode,))
    if index_dtype not in (torch.int32, torch.int64):
        raise ValueError("negative_batch: index_dtype must be torch.int32 or torch.int64 (got %s)" % (index_dtype,))
    if not torch.is_tensor(order) or order.dim() != 1 or order.dtype not in (torch.int32, torch.int64):
        raise ValueError("negative_batch: order must be an int32 / int64 [B] tensor")
    dev = tables.device
    if order.device != dev:
        raise _lib.BackendError("negative_batch: tensors on different devices: %s vs %s" % (dev, order.device))
    if dev.type not in ("cuda", "cpu"):
        raise _lib.BackendError("negative_batch: no implementation for device %s" % dev)
    K, b = int(K), order.shape[0]
    if K < 0:
        raise ValueError("negative_batch: K must not be negative (got %d)" % K)
    if max(b, K) >= 2 ** 31 - 1:
        raise _lib.BackendError("negative_batch: sizes beyond int32 indexing")
    positive = torch.empty((b, 3), dtype=torch.int64, device=dev)
    negative = torch.empty((b, K), dtype=index_dtype, device=dev)
    weight = torch.empty((b,), dtype=torch.float32, device=dev)
    if b == 0:
        return positive, negative, weight
    if order.dtype != torch.int32:  # (ids beyond int32 are outside any table: keep them so)
        order = order.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    order = order.contiguous()
    if K == 0:  # nothing is drawn: the gathers are torch's, the refusal is the kernel's
        bad = (order < 0) | (order >= tables.num_triples)
        if check and bool(bad.any()):
            raise_for_status(1)
        if tables.num_triples == 0:
            return positive.fill_(-1), negative, weight.zero_()
        rows = order.long().clamp(0, tables.num_triples - 1)
        positive = torch.where(bad[:, None], positive.new_full((), -1), tables.triples[rows].long())
        return positive, negative, torch.where(bad, weight.new_zeros(()), tables.weight[rows])
    m = tables.modes[mode]
    status = tables.status
    _lib.twin_call("kg_train_batch", dev, _lib.ptr(tables.triples), _lib.ptr(tables.weight), _lib.ptr(m.group), _lib.ptr(m.list_ptr),
                   _lib.ptr(m.list_idx), tables.num_triples, m.list_ptr.numel() - 1, m.list_idx.numel(), _lib.ptr(order), b, K,
                   tables.num_entities, int(seed) & (2 ** 64 - 1), TAGS[mode], int(first_sid) & (2 ** 64 - 1),
                   1 if index_dtype == torch.int64 else 0, _lib.ptr(positive), _lib.ptr(negative), _lib.ptr(weight),
                   _lib.ptr(status))
    if check:
        raise_for_status(status.item())  # the one synchronisation
    return positive, negative, weight
