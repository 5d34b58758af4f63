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
Groups of ANY rows (`assign=`: an assignment [n_groups, r] of row ids, pads negative and last in their group, or a procedure that
returns one): the same layout with the local row being the row's slot in its group, goff the groups' offsets in layout order, and
  rows [n_groups * r]  the row map the kernel stores through (csrc/rowsweep.h: MAPPED)
The layouts the policy builds (`of`, `register_forward`) take `deal_by_degree`: consecutive rows give waves whose edge counts
differ by +-4 %, and a wave with 4 % fewer edges is 4 % of the table ahead at the same edge index -- more than an XCD's L2 holds.
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
                 "out_of_order", "long_rows", "hash", "rows")

    def __init__(self, goff, src, eid, r, n_rows, n_src, out_of_order=0.0, long_rows=False, rows=None):
        self.goff, self.src, self.eid = goff, src, eid
        self.rows = rows  # the row map [n_groups * r] (int32) of an explicit assignment; None: groups of r consecutive rows
        self.r, self.n_rows, self.n_src = int(r), int(n_rows), int(n_src)
        self.n_groups, self.nnz = goff.numel() - 1, src.numel()
        self._val_key = self._val_src = self._val_p = None
        # forward layouts (build_forward): the share of edges gathered out of table order, whether a row exceeds the exact-row
        # bound (read once, at build time), and -- once registered -- the structure's 64-bit hash, which guards the launches
        self.out_of_order, self.long_rows, self.hash = float(out_of_order), bool(long_rows), None

    def nbytes(self):
        memo = self._val_p.numel() * self._val_p.element_size() if self._val_p is not None else 0
        # (the row map -- 4 bytes per row, beside 8 to 12 per edge -- is NOT counted: tests/test_sweep_gpu.py and
        # tests/test_sweep_forward_gpu.py pin the caches' byte counts of layouts the policy built to the three arrays and the memo)
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


def checked_assignment(assign, n_rows, r):
    """-> the row map [n_groups * r] (int64, on assign's device) of an assignment of rows to groups, `assign` [n_groups, r] or
    flat: row ids, negative = pad.  Refused unless it is a partition of the n_rows rows and a group's pads are its last slots.
    (The kernel stores through the map unchecked: this is where an entry >= n_rows is caught, before anything is enqueued.)"""
    flat = assign.reshape(-1).long()
    if flat.numel() % r or flat.numel() < n_rows:
        raise _lib.BackendError("sweep layout: an assignment of %d slots does not hold %d rows in groups of %d" % (flat.numel(), n_rows, r))
    real = flat >= 0
    if flat.numel() and int(flat.max()) >= n_rows:
        raise _lib.BackendError("sweep layout: the assignment names row %d of %d" % (int(flat.max()), n_rows))
    seen = torch.bincount(flat[real], minlength=n_rows) if n_rows else flat.new_zeros(0)
    if int(real.sum()) != n_rows or (n_rows and int(seen.min()) != 1):
        raise _lib.BackendError("sweep layout: the assignment is not a partition of the %d rows" % n_rows)
    by_group = real.view(-1, r)
    if r > 1 and bool((by_group[:, 1:] & ~by_group[:, :-1]).any()):
        raise _lib.BackendError("sweep layout: a group's pad slots must be its last ones")
    return flat


def _grouped(ptr, row, key, col, n_rows, n_src, r, assign):
    """The part both directions share -> (goff, src, order, rows): `order` sorts the edges stably by (group, key); rows is the
    row map (int32) of an explicit assignment, None for groups of r consecutive rows."""
    dev = ptr.device
    if assign is None:
        group = torch.div(row, r, rounding_mode="floor")
        local = row - group * r
        n_groups = (n_rows + r - 1) // r
        goff = ptr[torch.clamp(torch.arange(n_groups + 1, device=dev) * r, max=n_rows)].int()
        rows = None
    else:
        if callable(assign):  # (a procedure that wants the merge key: deal_by_degree)
            assign = assign(ptr, r, key)
        flat = checked_assignment(assign.to(dev), n_rows, r)
        n_groups = flat.numel() // r
        slot = torch.empty(n_rows, dtype=torch.long, device=dev)
        real = torch.nonzero(flat >= 0).flatten()
        slot[flat[real]] = real
        slot = slot[row]
        group = torch.div(slot, r, rounding_mode="floor")
        local = slot - group * r
        goff = torch.zeros(n_groups + 1, dtype=torch.long, device=dev)
        goff[1:] = torch.cumsum(torch.bincount(group, minlength=n_groups), 0)
        goff = goff.int()
        rows = flat.int().contiguous()
    # one stable sort does every group at once; equal keys (several rows of a group share a source, duplicate edges of one row)
    # keep the structure's own edge order
    order = torch.sort(group * max(n_src, 1) + key, stable=True).indices
    src = (col[order] | (local[order] << LOCAL_SHIFT)).int()
    return goff.contiguous(), src.contiguous(), order, rows


def build(colptr, rowind, perm, n_src, r, assign=None):
    """-> SweepPlan of the column-sorted structure (colptr [n_rows + 1], rowind [nnz], perm [nnz]; int32) gathering from a
    table of n_src rows, in groups of r consecutive rows -- or, with `assign` (checked_assignment), in the groups it names."""
    r, n_src = int(r), int(n_src)
    n_rows = colptr.numel() - 1
    if not (1 <= r < (1 << (31 - LOCAL_SHIFT))) or n_src >= (1 << LOCAL_SHIFT):
        raise _lib.BackendError("sweep layout: %d rows per group / a table of %d rows do not fit the packed edge word" % (r, n_src))
    cp = colptr.long()
    row = torch.repeat_interleave(torch.arange(n_rows, device=colptr.device), cp[1:] - cp[:-1])
    col = rowind.long()
    goff, src, order, rows = _grouped(cp, row, col, col, n_rows, n_src, r, assign)
    eid = perm.long()[order].int()
    return SweepPlan(goff, src, eid.contiguous(), r, n_rows, n_src, rows=rows)


def build_forward(rowptr, colind, n_src, r, assign=None):
    """-> SweepPlan of the CSR structure ITSELF (rowptr [m + 1], colind [nnz]; int32; any column order inside a row) gathering
    from a table of n_src rows, in groups of r rows (consecutive, or those of `assign`): edges inside a group stably sorted by
    group * n_src + the running maximum
    of the column inside the row (one global cummax over col + row * n_src gives it: a row's first entry exceeds everything
    before it).  eid is the position in the caller's CSR order.  Two facts for the policy ride along, read back once here."""
    r, n_src = int(r), int(n_src)
    m = rowptr.numel() - 1
    if not (1 <= r < (1 << (31 - LOCAL_SHIFT))) or n_src >= (1 << LOCAL_SHIFT):
        raise _lib.BackendError("sweep layout: %d rows per group / a table of %d rows do not fit the packed edge word" % (r, n_src))
    rp = rowptr.long()
    deg = rp[1:] - rp[:-1]
    row = torch.repeat_interleave(torch.arange(m, device=rowptr.device), deg)
    col = colind.long()
    nnz = col.numel()
    base = row * max(n_src, 1)
    run = (torch.cummax(col + base, 0).values - base) if nnz else col
    goff, src, order, rows = _grouped(rp, row, run, col, m, n_src, r, assign)
    out_of_order = float((col < run).sum()) / nnz if nnz else 0.0
    long_rows = bool(m and nnz and int(deg.max()) > _lib.hip().cogdl_hip_exact_row_edges(nnz))
    return SweepPlan(goff, src, order.int().contiguous(), r, m, n_src, out_of_order, long_rows, rows=rows)


def deal_by_degree(ptr, r, key=None):
    """-> an assignment [n_groups, r] (int64; -1 = pad) of the rows of `ptr` ([n_rows + 1]) to n_groups = ceil(n_rows / r)
    groups: rows sorted by edge count (descending, stable) and dealt over the groups boustrophedon -- round 0 left to right,
    round 1 right to left, ...; the row dealt in round k is local row k of its group, so pads are last and the longest rows
    are the first (register) rows.  Every group then walks (almost) the same number of edges: between any two groups the
    rounds' differences alternate in sign and each sign's sum telescopes, so max - min edges per group <= the largest row.
    With `key` (the merge key of every edge, [nnz]: what the walk ascends by) rows of EQUAL edge count are dealt in ascending
    order of their mean key.  The deal turns round after every round, so a group takes early-walking rows in one round and
    late-walking ones in the next: its edges then lie over the table as everybody's do, not only as many of them -- at the same
    edge index the waves are at the same place of the table.  (Sums of integers, one division in float64: deterministic.)
    Two sorts of n_rows keys; torch ops on ptr's device."""
    r = int(r)
    n_rows = ptr.numel() - 1
    n_groups = (n_rows + r - 1) // r
    p = ptr.long()
    deg = p[1:] - p[:-1]
    if key is None or key.numel() == 0:
        by_degree = torch.sort(deg, descending=True, stable=True).indices
    else:
        total = torch.cat([p.new_zeros(1), torch.cumsum(key.long(), 0)])
        mean = (total[p[1:]] - total[p[:-1]]).double() / deg.clamp(min=1).double()
        by_mean = torch.sort(mean, stable=True).indices
        by_degree = by_mean[torch.sort(deg[by_mean], descending=True, stable=True).indices]
    at = torch.arange(n_rows, device=ptr.device)
    rnd = torch.div(at, max(n_groups, 1), rounding_mode="floor")
    j = at - rnd * n_groups
    group = torch.where(rnd % 2 == 0, j, n_groups - 1 - j)
    assign = torch.full((n_groups * r,), -1, dtype=torch.long, device=ptr.device)
    assign[group * r + rnd] = by_degree
    return assign.view(n_groups, r)


# Which rows share a group in the layouts the policy builds (`of`, `register_forward`): a tensor-returning procedure
# (ptr, r, key), or None for r consecutive rows.
ASSIGN = deal_by_degree


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
        sp = build_forward(rowptr, colind, meta[3], r, ASSIGN)
        sp.hash = key[4] & 0xFFFFFFFFFFFFFFFF
        if not takeable(sp):  # the facts are kept (no second build), the 8 bytes per edge are not
            sp.goff = sp.src = sp.eid = sp.goff.new_empty(0)
            sp.rows = None
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
        sp = csc.sweep = build(csc.colptr, csc.rowind, csc.perm, csc.m, r, ASSIGN)
        _plan.PLANS.grew(csc, sp.nbytes())
    return sp


def values(csc, w):
    """The edge weights `w` (caller's CSR order) in the order of csc's sweep layout; a new memo is counted in the plan cache."""
    sp = csc.sweep
    before = sp.nbytes()
    w_p = sp.permuted_values(w)
    _plan.PLANS.grew(csc, sp.nbytes() - before)
    return w_p
