"""Inputs shared by test_readout_host.py and test_readout_gpu.py: the grids of the readout operators and plain references."""
import numpy as np
import torch

LENGTHS = [0, 1, 2, 63, 64, 65, 129, 300, 0]
WIDTHS = (1, 7, 64, 65, 130)
SORT_SIZES = [1, 2, 29, 30, 31, 64, 65, 200]
SORT_K = (1, 5, 30, 65)
SORT_WIDTHS = (8, 33)


def ptr_of(lengths):
    return torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)


def grid(extra=None):
    """(lengths, ptr, x [N, 130]) of the pooling grid, optionally with one more segment of `extra` rows at the end."""
    lengths = LENGTHS + ([extra] if extra else [])
    x = torch.randn(sum(lengths), max(WIDTHS), generator=torch.Generator().manual_seed(7)) * 100
    return lengths, ptr_of(lengths), x


def cols(x, f):
    return x[:, :f].contiguous()


def sequential_sum(x, ptr):
    """float32 additions in row order from +0.0f, one graph after the other (numpy adds rows elementwise, no pairwise tree)."""
    x, ptr = x.numpy(), ptr.numpy()
    out = np.zeros((len(ptr) - 1, x.shape[1]), dtype=np.float32)
    for g in range(len(ptr) - 1):
        acc = np.zeros(x.shape[1], dtype=np.float32)
        for i in range(ptr[g], ptr[g + 1]):
            acc = acc + x[i]
        out[g] = acc
    return out


def torch_pool(x, ptr, mode):
    """The plain torch composition (any dtype), differentiable: the reference for the backward checks."""
    rows = []
    p = ptr.tolist()
    for g in range(len(p) - 1):
        seg = x[p[g]:p[g + 1]]
        if seg.shape[0] == 0:
            rows.append(x.new_zeros(x.shape[1]))
        elif mode == "sum":
            rows.append(seg.sum(0))
        elif mode == "mean":
            rows.append(seg.mean(0))
        else:
            rows.append(seg.max(0)[0])
    return torch.stack(rows)


def stable_topk(key, ptr, k):
    """idx [B, k] by np.argsort(-key, kind="stable") per graph, -1 on padding."""
    p = ptr.tolist()
    idx = np.full((len(p) - 1, k), -1, dtype=np.int32)
    for g in range(len(p) - 1):
        order = np.argsort(-key[p[g]:p[g + 1]], kind="stable")[:k] + p[g]
        idx[g, :len(order)] = order
    return idx


def gather_rows(x, idx):
    """out [B, k, F] of x rows at idx, zeros where idx is -1."""
    idx = torch.as_tensor(idx, dtype=torch.long, device=x.device)
    out = x[idx.clamp(min=0)]
    return torch.where((idx >= 0).unsqueeze(-1), out, torch.zeros_like(out))
