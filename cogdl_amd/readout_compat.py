"""The reference's graph readout on this library's readout operators (cogdl_amd/operators/readout.py):
`install(readout=True)` binds `batch_sum_pooling`, `batch_mean_pooling` and `batch_max_pooling` (signatures of
cogdl/utils/utils.py:192-221) in every module that holds them by name, and `GIN.forward` / `SortPool.forward`.

What changes: the pooled rows come from a segment reduction over the sorted `batch` vector -- on the GPU without float
atomics, so equal from run to run, and for sum and mean bit for bit the reference's CPU result; max pooling no longer builds a
CSR per call and runs on the CPU as well (the reference needs torch_scatter there); SortPool's pad + sort + gather + mask is
one top-k kernel.  Equal keys in SortPool go in increasing row order (torch's descending sort leaves ties open).

What does not: a call the operators do not cover goes to the reference's own function (cogdl_amd/_rebind.original) --
`batch` unsorted or empty, x not float32 or not 2-D, and a mean over a batch with absent graph ids, where the reference
returns len(unique(batch)) rows.  Sum and max over such a batch return max id + 1 rows, as the reference's do.
"""
import sys

import torch
import torch.nn.functional as F

from . import _lib, _rebind
from .operators.readout import segment_pool, segment_ptr, sort_pool

_UTILS = "cogdl.utils.utils"


def _segments(x, batch):
    """ptr of `batch` if the operators cover this call, else None."""
    if not (torch.is_tensor(x) and torch.is_tensor(batch)):
        return None
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] < 1 or x.device.type not in ("cuda", "cpu"):
        return None
    if batch.dim() != 1 or batch.dtype != torch.int64 or batch.numel() == 0 or batch.numel() != x.shape[0]:
        return None
    if batch.device != x.device:
        return None
    try:
        return segment_ptr(batch)[0]
    except _lib.BackendError:  # unsorted, or a negative id
        return None


def _reference(name):
    fn = _rebind.original(sys.modules.get(_UTILS), name)
    if fn is None:
        raise _lib.BackendError("%s: this call needs the reference's function (batch unsorted or empty, x not 2-D float32, or a "
                                "mean over absent graph ids) and cogdl.utils.utils does not hold one" % name)
    return fn


def batch_sum_pooling(x, batch):
    ptr = _segments(x, batch)
    return _reference("batch_sum_pooling")(x, batch) if ptr is None else segment_pool(x, ptr, "sum")


def batch_mean_pooling(x, batch):
    ptr = _segments(x, batch)
    if ptr is None or bool((ptr[1:] == ptr[:-1]).any()):
        return _reference("batch_mean_pooling")(x, batch)
    return segment_pool(x, ptr, "mean")


def batch_max_pooling(x, batch):
    ptr = _segments(x, batch)
    return _reference("batch_max_pooling")(x, batch) if ptr is None else segment_pool(x, ptr, "max")


def _reference_forward(modname, clsname):
    return _rebind.original(getattr(sys.modules[modname], clsname), "forward")


def gin_forward(self, batch):
    """GIN.forward: the layers as the reference runs them, then per layer representation sum readout -> linear -> dropout,
    added up; one ptr serves every layer."""
    h = batch.x
    ptr = _segments(h, batch.batch)
    if ptr is None:
        return _reference_forward("cogdl.models.nn.gin", "GIN")(self, batch)
    reps = [h]
    for layer, norm in zip(self.gin_layers, self.batch_norm):
        h = F.relu(norm(layer(batch, h)))
        reps.append(h)
    score = 0
    for rep, predict in zip(reps, self.linear_prediction):
        score = score + self.dropout(predict(segment_pool(rep, ptr, "sum")))
    return score


def sortpool_forward(self, batch):
    """SortPool.forward: the convolutions, each node's channels sorted ascending, then per graph the k nodes with the
    largest last channel in descending order (zero rows where the graph is smaller), as [B, channels, k] into the 1-D
    convolution and the two linear layers."""
    h = batch.x
    ptr = _segments(h, batch.batch)
    if ptr is None:
        return _reference_forward("cogdl.models.nn.sortpool", "SortPool")(self, batch)
    for conv in self.gnn_convs:
        h = F.relu(conv(batch, h))
    h, _ = h.sort(dim=-1)
    pooled, _ = sort_pool(h, ptr, self.k)
    h = F.relu(self.conv1d(pooled.permute(0, 2, 1))).view(pooled.shape[0], -1)
    h = F.relu(self.fc1(h))
    h = F.dropout(h, p=self.dropout, training=self.training)
    return self.fc2(h)
