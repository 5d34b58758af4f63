"""Sweep layout of a stable transpose: the host side of `cogdl_hip_csr_spmm_sweep` (include/cogdl_hip.h, csrc/rowsweep.h).

The backward pass of csr_spmm runs over A^T, which comes from this library's own stable `csr2csc`: inside every row of A^T the
gathered rows (`rowind`) ascend.  So the edges of MANY rows may be visited merged in ascending order of the gathered row while
every row still sees its own edges in exactly its own order -- bit-identical sums -- and a wave that owns a group of rows then
walks the table `grad_out` top to bottom.  With every wave of the chip doing so at about the same pace, the gathers of an XCD
fall into a window of the table that its 4 MiB L2 holds.  The forward cannot do this: the rows of the
caller's CSR are not column-sorted, and their summation order is their CSR order.

Layout, for groups of `r` consecutive rows of A^T (group g = rows [g r, min((g + 1) r, n_rows))):
  goff [n_groups + 1]  edge offsets of the groups (the groups' edges are the contiguous CSC ranges colptr[g r] .. colptr[(g + 1) r])
  src  [nnz]           per edge, stably sorted by gathered row inside a group: gathered row | local row << 24
  eid  [nnz]           the edge's position in the CALLER's CSR edge order (the transpose's perm composed with the sort)
Built with torch ops on whatever device the plan's tensors live on (the tests build it on the CPU), lazily, kept on the plan.
"""
import torch

from . import _lib
from . import plan as _plan

LOCAL_SHIFT = 24            # tables of < 2^24 rows (as the XCD plans assume); local rows < 2^7
MAX_TABLE_ROWS = 1 << 23    # ... and 512-byte rows at 32-bit byte offsets (csrc/rowsweep.h)


class SweepPlan:
    __slots__ = ("goff", "src", "eid", "r", "n_rows", "n_src", "n_groups", "nnz", "_val_key", "_val_src", "_val_p")

    def __init__(self, goff, src, eid, r, n_rows, n_src):
        self.goff, self.src, self.eid = goff, src, eid
        self.r, self.n_rows, self.n_src = int(r), int(n_rows), int(n_src)
        self.n_groups, self.nnz = goff.numel() - 1, src.numel()
        self._val_key = self._val_src = self._val_p = None

    def nbytes(self):
        memo = self._val_p.numel() * self._val_p.element_size() if self._val_p is not None else 0
        return 4 * (self.goff.numel() + self.src.numel() + self.eid.numel()) + memo

    def permuted_values(self, w):
        """w in layout order (w[eid]); the rule of CscPlan.transposed_values: constant weights are gathered once (memo keyed on
        plan.tensor_key plus a held reference), weights that take part in autograd per call."""
        src = w.detach()
        if w.requires_grad:
            return _plan.gather_rows(self.eid, src)
        key = _plan.tensor_key(w)
        if key != self._val_key or self._val_src is None:
            self._val_p = _plan.gather_rows(self.eid, src)
            self._val_key, self._val_src = key, src
        return self._val_p


def build(colptr, rowind, perm, n_src, r):
    """-> SweepPlan of the column-sorted structure (colptr [n_rows + 1], rowind [nnz], perm [nnz]; int32) gathering from a
    table of n_src rows, in groups of r rows."""
    r, n_src = int(r), int(n_src)
    n_rows = colptr.numel() - 1
    if not (1 <= r < (1 << (31 - LOCAL_SHIFT))) or n_src >= (1 << LOCAL_SHIFT):
        raise _lib.BackendError("sweep layout: %d rows per group / a table of %d rows do not fit the packed edge word" % (r, n_src))
    dev = colptr.device
    cp = colptr.long()
    row = torch.repeat_interleave(torch.arange(n_rows, device=dev), cp[1:] - cp[:-1])
    group = torch.div(row, r, rounding_mode="floor")
    col = rowind.long()
    # one stable sort does every group at once; equal gathered rows (several rows of a group share a source, duplicate edges of
    # one row) keep their CSC order
    order = torch.sort(group * max(n_src, 1) + col, stable=True).indices
    src = (col[order] | ((row - group * r)[order] << LOCAL_SHIFT)).int()
    eid = perm.long()[order].int()
    n_groups = (n_rows + r - 1) // r
    goff = cp[torch.clamp(torch.arange(n_groups + 1, device=dev) * r, max=n_rows)].int()
    return SweepPlan(goff.contiguous(), src.contiguous(), eid.contiguous(), r, n_rows, n_src)


def group_rows(n_rows, round_rows, max_group_rows):
    """Rows per group for a structure of n_rows rows when one round holds round_rows = waves * max_group_rows: as few as still
    give every row a resident wave (a small structure spreads over all waves instead of filling a few to the brim)."""
    waves = max(1, int(round_rows) // int(max_group_rows))
    return max(1, min(int(max_group_rows), -(-int(n_rows) // waves)))


def round_rows(k, dtype):
    """How many rows of k columns one round holds on the current device (0: a width the kernel declines)."""
    code = _lib.DTYPE_CODE.get(dtype)
    return 0 if code is None else int(_lib.hip().cogdl_hip_csr_spmm_sweep_round_rows(int(k), code))


def of(csc, k, dtype):
    """The sweep layout of a plan.CscPlan, built on first use and kept on it (counted in the plan cache's byte budget)."""
    sp = csc.sweep
    if sp is None:
        r = group_rows(csc.n_cols, round_rows(k, dtype), _lib.hip().cogdl_hip_csr_spmm_sweep_group_rows())
        sp = csc.sweep = build(csc.colptr, csc.rowind, csc.perm, csc.m, r)
        _plan.PLANS.grew(csc, sp.nbytes())
    return sp


def values(csc, w):
    """The edge weights `w` (caller's CSR order) in the order of csc's sweep layout; a new memo is counted in the plan cache."""
    sp = csc.sweep
    before = sp.nbytes()
    w_p = sp.permuted_values(w)
    _plan.PLANS.grew(csc, sp.nbytes() - before)
    return w_p
