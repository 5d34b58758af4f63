"""`torch_sparse.spspmm` / `torch_sparse.spmm` for CogDL models on a box without torch_sparse.

The reference's srgcn (models/nn/srgcn.py, utils/srgcn_utils.py), graph_unet (models/nn/graph_unet.py) and gtn
(models/nn/gtn.py) import these two functions from `torch_sparse`, an optional compiled dependency; without it the
models cannot even be imported.  `cogdl_amd.install(torch_sparse=True)` registers THIS module under the name
`torch_sparse` when the real one cannot be imported:
  spspmm   CUDA float32 -> cogdl_amd.operators.spgemm (coalesce + the HIP product, gradients for both value vectors);
           CPU tensors and other dtypes -> torch.sparse.mm on coalesced COO (graph_unet moves its index to the CPU).
  spmm     CUDA float32 -> the fused COO message operator (cogdl_amd.operators.ops.src_op_e_aggr_coo, mul / sum);
           otherwise the scatter-add torch_sparse itself computes.
A GPU spspmm reads back to the host five times (each coalesce: its index bounds and its distinct count; the product: nnz(C),
and once more when a row has more than 4096 products): it is host-synchronous, like torch_sparse's own CUDA path, and
cannot run inside a stream capture.
Both follow torch_sparse's contract: COO index int64 [2, nnz] (row, col), the result of spspmm coalesced and sorted
row-major, its pattern structural (an entry whose products cancel is kept).
"""
import torch

__all__ = ["spspmm", "spmm"]


def _hip_route(*tensors):
    return all(t.is_cuda for t in tensors) and all(t.dtype == torch.float32 for t in tensors if t.is_floating_point())


def spspmm(indexA, valueA, indexB, valueB, m, k, n, coalesced=False):
    """C = A . B, A [m, k] and B [k, n] as COO (index [2, nnz], value [nnz]) -> (index int64 [2, nnz(C)], value).
    The inputs are canonicalised whatever `coalesced` says: callers pass coalesced=True on indices whose appended self
    loops are not sorted (cogdl/utils/graph_utils.py: add_remaining_self_loops)."""
    del coalesced
    m, k, n = int(m), int(k), int(n)
    if _hip_route(indexA, valueA, indexB, valueB):
        from .operators.spgemm import _spgemm_trusted, coalesce

        rA, cA, vA = coalesce(indexA[0], indexA[1], valueA, m, k)
        rB, cB, vB = coalesce(indexB[0], indexB[1], valueB, k, n)
        rC, cC, vC = _spgemm_trusted(rA, cA, vA, rB, cB, vB, m, k, n)
        rows = torch.repeat_interleave(torch.arange(m, device=rC.device), (rC[1:] - rC[:-1]).long(), output_size=cC.numel())
        return torch.stack([rows, cC.long()]), vC
    A = torch.sparse_coo_tensor(indexA, valueA, (m, k)).coalesce()
    B = torch.sparse_coo_tensor(indexB, valueB, (k, n)).coalesce()
    C = torch.sparse.mm(A, B).coalesce()
    return C.indices(), C.values()


def spmm(index, value, m, n, matrix):
    """out [m, F] = A . matrix with A [m, n] as COO (index [2, nnz], value [nnz]), matrix [n, F]; differentiable in
    value and matrix."""
    m, n = int(m), int(n)
    row, col = index[0], index[1]
    vec = matrix.dim() == 1
    x = matrix.view(-1, 1) if vec else matrix
    if _hip_route(index, value, x) and row.numel() > 0 and x.shape[1] > 0:
        from .operators.ops import src_op_e_aggr_coo

        if m > x.shape[0]:  # (the operator's output has one row per row of its node features)
            x = torch.cat([x, x.new_zeros(m - x.shape[0], x.shape[1])])
        out = src_op_e_aggr_coo("mul", "sum", x, value.view(-1, 1), row, col)[:m]
    else:
        out = torch.zeros(m, x.shape[1], dtype=torch.promote_types(value.dtype, x.dtype), device=x.device)
        out = out.index_add(0, row, value.view(-1, 1) * x.index_select(0, col))
    return out.view(-1) if vec else out
