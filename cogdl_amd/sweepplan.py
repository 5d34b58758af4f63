"""Sweep layouts: the host side of `cogdl_hip_csr_spmm_sweep` and `cogdl_hip_csr_spmm_sweep_guarded` (include/cogdl_hip.h,
csrc/rowsweep.h).

A wave that owns a group of rows may visit the edges of ALL of them merged in ascending order of the gathered row while every row
still sees its own edges in exactly its own order -- bit-identical sums -- provided the merge is a STABLE sort on a key that never
decreases inside a row.  The wave then walks the gathered table top to bottom, and with every wave of the chip doing so at about
the same pace, the gathers of an XCD fall into a window of the table that its 4 MiB L2 holds.

Backward (`build`): the launch runs over A^T, which comes from this library's own stable `csr2csc`: inside every row of A^T the
gathered rows (`rowind`) ascend, so the key is the gathered row itself.
Forward (`build_forward`): the rows of the caller's CSR need not be column-sorted, and their summation order is their CSR order.
The key is the RUNNING MAXIMUM of the column inside the row: it never decreases, so the row's order is kept whatever the row looks
like; an edge whose column lies behind its row's running maximum is merely gathered out of table order (a row that CogDL's
`add_remaining_self_loops` made -- an ascending run plus one appended self loop -- has one such edge).  The share of such edges
is recorded with the layout; the policy (xcdplan.spmm_forward_sweep) declines structures with many of them.

Layout, for groups of `r` consecutive rows (group g = rows [g r, min((g + 1) r, n_rows))):
  goff [n_groups + 1]  edge offsets of the groups (the groups' edges are contiguous ranges of the structure's own edge order)
  src  [nnz]           per edge, stably sorted by the key inside a group: gathered row | local row << 24
  eid  [nnz]           the edge's position in the CALLER's CSR edge order (backward: the transpose's perm composed with the sort)
Built with torch ops on whatever device the structure's tensors live on (the tests build it on the CPU).  The backward's layout is
built lazily and kept on the transpose's plan; the forward's lives in a cache of its own (`FORWARD`, keyed by the structure's
Fingerprint key, outside the plan cache's byte count).
"""
import collections
import os

import torch

from . import _lib
from . import plan as _plan

LOCAL_SHIFT = 24            # tables of < 2^24 rows (as the XCD plans assume); local rows < 2^7
MAX_TABLE_ROWS = 1 << 23    # ... and 512-byte rows at 32-bit byte offsets (csrc/rowsweep.h)


class SweepPlan:
    __slots__ = ("goff", "src", "eid", "r", "n_rows", "n_src", "n_groups", "nnz", "_val_key", "_val_src", "_val_p",
                 "out_of_order", "long_rows", "hash")

    def __init__(self, goff, src, eid, r, n_rows, n_src, out_of_order=0.0, long_rows=False):
        self.goff, self.src, self.eid = goff, src, eid
        self.r, self.n_rows, self.n_src = int(r), int(n_rows), int(n_src)
        self.n_groups, self.nnz = goff.numel() - 1, src.numel()
        self._val_key = self._val_src = self._val_p = None
        # forward layouts (build_forward): the share of edges gathered out of table order, whether a row exceeds the exact-row
        # bound (read once, at build time), and -- once registered -- the structure's 64-bit hash, which guards the launches
        self.out_of_order, self.long_rows, self.hash = float(out_of_order), bool(long_rows), None

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


def build_forward(rowptr, colind, n_src, r):
    """-> SweepPlan of the CSR structure ITSELF (rowptr [m + 1], colind [nnz]; int32; any column order inside a row) gathering
    from a table of n_src rows, in groups of r rows: edges inside a group stably sorted by group * n_src + the running maximum
    of the column inside the row (one global cummax over col + row * n_src gives it: a row's first entry exceeds everything
    before it).  eid is the position in the caller's CSR order.  Two facts for the policy ride along, read back once here."""
    r, n_src = int(r), int(n_src)
    m = rowptr.numel() - 1
    if not (1 <= r < (1 << (31 - LOCAL_SHIFT))) or n_src >= (1 << LOCAL_SHIFT):
        raise _lib.BackendError("sweep layout: %d rows per group / a table of %d rows do not fit the packed edge word" % (r, n_src))
    dev = rowptr.device
    rp = rowptr.long()
    deg = rp[1:] - rp[:-1]
    row = torch.repeat_interleave(torch.arange(m, device=dev), deg)
    group = torch.div(row, r, rounding_mode="floor")
    col = colind.long()
    nnz = col.numel()
    stride = max(n_src, 1)
    base = row * stride
    run = (torch.cummax(col + base, 0).values - base) if nnz else col
    order = torch.sort(group * stride + run, stable=True).indices
    src = (col[order] | ((row - group * r)[order] << LOCAL_SHIFT)).int()
    n_groups = (m + r - 1) // r
    goff = rp[torch.clamp(torch.arange(n_groups + 1, device=dev) * r, max=m)].int()
    out_of_order = float((col < run).sum()) / nnz if nnz else 0.0
    long_rows = bool(m and nnz and int(deg.max()) > _lib.hip().cogdl_hip_exact_row_edges(nnz))
    return SweepPlan(goff.contiguous(), src.contiguous(), order.int().contiguous(), r, m, n_src, out_of_order, long_rows)


class ForwardCache:
    """The forward layouts, keyed by the structure's Fingerprint key; a byte budget of its own (COGDL_AMD_SWEEP_FWD_CACHE_MB),
    evicted from the cold end.  Not part of plan.PLANS' count: a CscPlan's nbytes() is its transpose and the backward's layout."""

    def __init__(self, budget_bytes=None):
        if budget_bytes is None:
            budget_bytes = int(os.environ.get("COGDL_AMD_SWEEP_FWD_CACHE_MB", "1024")) << 20
        self.budget, self.bytes = budget_bytes, 0
        self.lru = collections.OrderedDict()

    def get(self, key):
        sp = self.lru.get(key)
        if sp is not None:
            self.lru.move_to_end(key)
        return sp

    def put(self, key, sp):
        old = self.lru.pop(key, None)
        if old is not None:
            self.bytes -= old.nbytes()
        self.lru[key] = sp
        self.bytes += sp.nbytes()
        self._evict()

    def grew(self, delta):
        self.bytes += delta
        self._evict()

    def _evict(self):
        while self.bytes > self.budget and len(self.lru) > 1:
            key, old = self.lru.popitem(last=False)
            self.bytes -= old.nbytes()
            if _plan.CANDIDATES.get(key[:4]) == key:
                del _plan.CANDIDATES[key[:4]]

    def clear(self):
        self.lru.clear()
        self.bytes = 0


FORWARD = ForwardCache()
_plan._forward_layouts = FORWARD


def candidate(meta):
    """The forward layout registered for what a call knows of its structure before its hash lands, or None."""
    key = _plan.CANDIDATES.get(meta)
    return FORWARD.get(key) if key is not None else None


def register_forward(fp, rowptr, colind, k, dtype):
    """Backward pass, from the structure's second sighting on (the key is on the host: PLANS.get has waited for it): build the
    forward layout of the structure unless it is cached, and make the structure THE candidate of its (device, m, nnz, n_src)."""
    key = fp.key()
    meta = key[:4]
    sp = FORWARD.get(key)
    if sp is None:
        m = rowptr.numel() - 1
        r = group_rows(m, round_rows(k, dtype), _lib.hip().cogdl_hip_csr_spmm_sweep_group_rows())
        sp = build_forward(rowptr, colind, meta[3], r)
        sp.hash = key[4] & 0xFFFFFFFFFFFFFFFF
        if not takeable(sp):  # the facts are kept (no second build), the 8 bytes per edge are not
            sp.goff = sp.src = sp.eid = sp.goff.new_empty(0)
        FORWARD.put(key, sp)
    if takeable(sp) and _plan.CANDIDATES.get(meta) != key:
        _plan.CANDIDATES[meta] = key
    return sp


def takeable(sp):
    """Do the facts recorded with a forward layout let the policy take it (xcdplan.spmm_forward_sweep)?"""
    from . import xcdplan

    return not sp.long_rows and sp.out_of_order <= xcdplan.SWEEP_FORWARD_MAX_OUT_OF_ORDER


def forward_values(sp, w):
    """The edge weights `w` (caller's CSR order) in the order of a cached forward layout; a new memo is counted in FORWARD."""
    before = sp.nbytes()
    w_p = sp.permuted_values(w)
    if sp.nbytes() != before and any(p is sp for p in FORWARD.lru.values()):
        FORWARD.grew(sp.nbytes() - before)
    return w_p


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
    """The (backward) sweep layout of a plan.CscPlan, built on first use and kept on it (counted in the plan cache's byte budget)."""
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
