"""XCD-partitioned column plans (round 6): the host side of `cogdl_hip_vrows` (include/cogdl_hip.h, csrc/rowreduce.h).

Every XCD of the MI355X has a private 4 MiB L2.  The gathered table of BASELINE configs[2] (233 k rows of 128-256 bytes)
fits none of them but fits the eight together -- if XCD x only ever gathers the columns it OWNS.  A plan gives every column
an owner (a multiplicative hash of its id: R-MAT / citation ids correlate with degree, `col % 8` leaves the XCDs 1.5x out of
balance), cuts every row of more than `split` edges into the sub-rows of its edges by owner (CSR order inside a sub-row,
pieces of at most `piece` edges) and lays these virtual rows out in units of 64 slots dealt round-robin to the XCDs -- the
order in which the hardware hands workgroups to them.  Shorter rows stay whole.  The reference has nothing like it (its
GE-SpMM kernels, cogdl/operators/spmm/spmm_kernel.cu:192-512, know one L2).

The plan is a property of the STRUCTURE: built once (a handful of sorts over the edge list, torch on the device: ~0.2 s at
1.1e8 edges), cached under the structure's content fingerprint next to the transpose (cogdl_amd/plan.py).  WHEN a launch runs
over one, and cut at which row length, is decided by the policy at the end of this file, for every operator that can take a plan.
fp32 csr_spmm is cut at the exact-row bound of its ordinary launch: rows up to it stay whole and bit-identical, only the longer
rows -- which the ordinary launch re-associates too -- are cut by owner.  `MODE` (COGDL_AMD_XCD) overrides the rules for A/B runs.
"""
import collections
import ctypes
import os

import torch

from . import _lib
from . import plan as _plan

UNIT = 64          # slots per unit (csrc/rowreduce.h: kVUnit)
XCDS = 8
SPLIT = 256        # rows of more than this many edges are cut by owner XCD (Reddit-shaped graph, fused GAT bf16 H8xF8 with dropout,
                   # fwd+bwd by split / piece: 64/256 6.21 ms, 128/256 6.02, 256/256 5.82, 256/512 6.15, 512/512 6.11: profiles/r06_gat_split.txt)
PIECE = 512        # edges per virtual row at most (with the virtual rows in order of length, same probe: 256/256 5.20 ms, 256/512 5.02,
                   # 512/512 5.24, 128/256 5.19, 256/128 5.47: profiles/r06_gat_split2.txt)
BIG_PARTS = 32     # (csrc/rowreduce.h: kVBigParts)
SORT_BY_LENGTH = os.environ.get("COGDL_AMD_XCD_SORT", "1") != "0"  # (A/B switch: the slot order inside an XCD's stream)
MODE = os.environ.get("COGDL_AMD_XCD", "auto")  # "auto" | "off" | "force" (every structure, every operator: tests)


class _VRowsStruct(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("vrowptr", "vcol", "vdesc", "eid", "mrow", "mptr", "big")] + \
               [(n, ctypes.c_int64) for n in ("n_slots", "n_multi", "n_parts", "n_big", "nnz")]


class XcdPlan:
    __slots__ = ("vrowptr", "vcol", "vdesc", "eid", "mrow", "mptr", "big", "n_slots", "n_multi", "n_parts", "n_big", "nnz", "m",
                 "_struct", "_val_key", "_val_src", "_val_p")

    def __init__(self, vrowptr, vcol, vdesc, eid, mrow, mptr, n_parts, m):
        self.vrowptr, self.vcol, self.vdesc, self.eid, self.mrow, self.mptr = vrowptr, vcol, vdesc, eid, mrow, mptr
        self.n_slots, self.n_multi, self.n_parts = vdesc.shape[0], mrow.numel(), int(n_parts)
        # rows of more than BIG_PARTS parts (csrc/rowreduce.h: kVBigParts): merged by a whole workgroup each
        self.big = torch.nonzero((mptr[1:] - mptr[:-1]) > BIG_PARTS).flatten().int()
        self.n_big = self.big.numel()
        self.nnz, self.m = vcol.numel(), m
        self._val_key = self._val_src = self._val_p = None
        s = _VRowsStruct()
        for name in ("vrowptr", "vcol", "vdesc", "eid", "mrow", "mptr", "big"):
            t = getattr(self, name)
            setattr(s, name, t.data_ptr() if t is not None and t.numel() else None)
        s.n_slots, s.n_multi, s.n_parts, s.n_big, s.nnz = self.n_slots, self.n_multi, self.n_parts, self.n_big, self.nnz
        self._struct = s

    def ref(self):
        """const cogdl_hip_vrows * (the plan keeps the tensors -- and the struct -- alive)."""
        return ctypes.byref(self._struct)

    def nbytes(self):
        return 4 * sum(t.numel() for t in (self.vrowptr, self.vcol, self.vdesc, self.eid, self.mrow, self.mptr, self.big))

    def permuted_values(self, w):
        """w in plan order (w[eid]).  Constant edge weights are gathered once (memo keyed like CscPlan.transposed_values)."""
        src = w.detach()
        if w.requires_grad:
            return _plan.gather_rows(self.eid, src)
        key = _plan.tensor_key(w)
        if key != self._val_key or self._val_src is None:
            self._val_p = _plan.gather_rows(self.eid, src)
            self._val_key, self._val_src = key, src
        return self._val_p


def owner_of(col):
    """Owner XCD of a column id (int64 tensor): the top three bits of a 32-bit multiplicative hash."""
    return ((col * 2654435761) & 0xFFFFFFFF) >> 29


def build(rowptr, colind, eid_base=None, split=None, piece=None):
    """-> XcdPlan of the CSR structure (rowptr [m + 1], colind [nnz]; int32 device tensors).  eid_base: what position j of
    THIS structure means to a per-edge operand (a CSC view passes the transpose's perm); None: the position itself."""
    split = SPLIT if split is None else int(split)
    piece = PIECE if piece is None else int(piece)
    dev = rowptr.device
    m, nnz = rowptr.numel() - 1, colind.numel()
    rp = rowptr.long()
    deg = rp[1:] - rp[:-1]
    rows = torch.arange(m, device=dev)
    row = torch.repeat_interleave(rows, deg)
    col = colind.long()
    is_long = deg > split
    xcd_e = torch.where(is_long[row], owner_of(col), row % XCDS)
    key = xcd_e * max(m, 1) + row
    del xcd_e
    order = torch.argsort(key, stable=True)  # (XCD, row), CSR order inside
    gkey, cnt = torch.unique_consecutive(key[order], return_counts=True)
    del key
    empty = torch.nonzero(deg == 0).flatten()
    if empty.numel():  # rows without edges still own a (whole, empty) slot: their output has to be written
        gkey = torch.cat([gkey, (empty % XCDS) * max(m, 1) + empty])
        cnt = torch.cat([cnt, torch.zeros_like(empty)])
        gkey, o = torch.sort(gkey)  # (edge offsets below come from a cumulative sum: empty groups add nothing)
        cnt = cnt[o]
    # pieces of at most `piece` edges -- for the sub-rows of LONG rows only: a row of at most `split` edges stays ONE virtual
    # row whatever its length (sequential CSR order: fp32 csr_spmm's bit-exact rows, split = its exact-row bound > piece)
    n_p = torch.where(is_long[gkey % max(m, 1)], torch.clamp((cnt + piece - 1) // piece, min=1), torch.ones_like(cnt))
    n_groups = gkey.numel()
    vg = torch.repeat_interleave(torch.arange(n_groups, device=dev), n_p)
    n_v = vg.numel()
    first_v = torch.cumsum(n_p, 0) - n_p
    idx = torch.arange(n_v, device=dev) - first_v[vg]
    vlen = torch.where(n_p[vg] == 1, cnt[vg], torch.where(idx < n_p[vg] - 1, torch.full_like(idx, piece), cnt[vg] - piece * (n_p[vg] - 1)))
    vx, vr = (gkey // max(m, 1))[vg], (gkey % max(m, 1))[vg]
    # records: the virtual rows of a row with several parts, in (row, XCD, piece) order
    parts_of_row = torch.bincount(vr, minlength=m)
    multi = parts_of_row > 1
    ord2 = torch.argsort(vr, stable=True)  # (the list is (XCD, row, piece)-ordered: stable by row keeps (XCD, piece))
    is_multi_sorted = multi[vr[ord2]]
    rec = torch.full((n_v,), -1, dtype=torch.long, device=dev)
    rec_sorted = torch.cumsum(is_multi_sorted.long(), 0) - 1
    rec[ord2[is_multi_sorted]] = rec_sorted[is_multi_sorted]
    n_parts = int(is_multi_sorted.sum())
    mrow = torch.nonzero(multi).flatten()
    mptr = torch.zeros(mrow.numel() + 1, dtype=torch.long, device=dev)
    torch.cumsum(parts_of_row[mrow], 0, out=mptr[1:])
    # slots: XCD x's k-th virtual row -> unit (k // 64) * 8 + x
    counts = torch.bincount(vx, minlength=XCDS)
    per = int((int(counts.max()) + UNIT - 1) // UNIT * UNIT) if n_v else 0
    n_slots = XCDS * per
    start = torch.cumsum(counts, 0) - counts
    if SORT_BY_LENGTH and n_v:
        # An XCD's virtual rows in order of DECREASING length: the lane groups of a wave (and the waves of a workgroup) then
        # walk rows of the same length -- a wave lasts as long as its longest row, and in (row, piece) order neighbours
        # differ by an order of magnitude on a skewed graph (Reddit-shaped graph, fused GAT forward: 5.2 vector instructions per
        # edge executed where the loop body has 3.5: a third of all lane-slots masked off, profiles/r06_mem_pipeline.txt).
        # Longest first is also the better schedule for the launch's tail.  Which slot walks a virtual row changes nothing
        # in what it computes, and the records are merged by (row, XCD, piece) as before: results are bit-identical.
        by_len = torch.argsort(vx * (int(vlen.max()) + 1) + (int(vlen.max()) - vlen), stable=True)
        k = torch.empty(n_v, dtype=torch.long, device=dev)
        k[by_len] = torch.arange(n_v, device=dev) - start[vx[by_len]]
        del by_len
    else:
        k = torch.arange(n_v, device=dev) - start[vx]
    slot = ((k // UNIT) * XCDS + vx) * UNIT + k % UNIT
    vdesc = torch.full((n_slots, 2), -1, dtype=torch.int32, device=dev)
    vdesc[slot, 0] = vr.int()
    vdesc[slot, 1] = rec.int()
    lens = torch.zeros(n_slots, dtype=torch.long, device=dev)
    lens[slot] = vlen
    vrowptr = torch.zeros(n_slots + 1, dtype=torch.long, device=dev)
    torch.cumsum(lens, 0, out=vrowptr[1:])
    v_of_edge = torch.repeat_interleave(torch.arange(n_v, device=dev), vlen)
    eorder = torch.argsort(slot[v_of_edge], stable=True)
    final = order[eorder]
    vcol = colind[final].contiguous()
    eid = (final if eid_base is None else eid_base.long()[final]).int().contiguous()
    if nnz >= 2 ** 31 or n_slots >= 2 ** 31:
        raise _lib.BackendError("XCD plan: the structure exceeds int32 positions")
    return XcdPlan(vrowptr.int(), vcol, vdesc.contiguous(), eid, mrow.int(), mptr.int(), n_parts, m)


def wanted(m, nnz, n_src, row_bytes):
    """Should a launch over this structure, gathering rows of `row_bytes` from an [n_src, .] table, take a plan?  Hub-heavy
    launches (>= 64 edges per row on average, >= 8 M edges) over tables between one L2 and a few times the eight of them, rows
    of at least 128 bytes.  Measured on the Reddit-shaped graph (493 edges per row, profiles/r06_xcd_quick.txt), fused GAT
    forward + backward: H = 8 x F = 8 bf16 (128-byte rows, 30 MB) 7.31 -> 5.66 ms, fp32 (60 MB) 11.83 -> 7.73 ms; H = 1 x
    F = 48 bf16 (96-byte rows, 22 MB: one head per lane group, bound by instruction issue, not by the gathers) 6.07 -> 5.97 ms
    without and 6.56 -> 6.93 ms with dropout -- not taken (the operator pads such rows to 128 bytes: fused_gat._padded_width).
    Which operators ask: the policy at the end of this file."""
    if MODE == "off" or _plan.transient():
        return False
    if n_src >= (1 << 24) or n_src * row_bytes >= (1 << 32):  # (the plan kernels address the table with 24 x 24 -> 32-bit offsets)
        return False
    if MODE == "force":
        return nnz > 0
    table = n_src * row_bytes
    return nnz >= (1 << 23) and nnz >= 64 * m and row_bytes >= 128 and (2 << 20) <= table <= (512 << 20)


ORDERED_MIN_EDGES = 1 << 18   # below: the launch is a few microseconds, nothing to balance
ORDERED_MAX_FILL = 0.5        # "skewed": eight consecutive rows fill less than this share of the lane-slots of their longest
_SKEW = {}


def ordered_wanted(fp, rowptr, m, nnz, n_src, row_bytes):
    """The second way into a plan (round 6): a SKEWED structure of any size whose fingerprint is ALREADY KNOWN on the host (who
    waits for it, and when a key counts as known: the policy at the end of this file).  What a
    plan buys there is its slot order: an XCD's virtual rows by decreasing length, so that the lane groups of a wave walk rows
    of one length, and hub rows as pieces merged by rowreduce_vcombine_kernel.  Measured on the arxiv-sized R-MAT graph (max
    degree 10^4; tools/exp/small_plan_ab.py, profiles/r06_small_plan_ab.txt), ordinary launch -> plan cut at the exact-row
    bound: fp32 F = 128 183 -> 144 us, F = 64 100 -> 63 us, F = 40 103 -> 60 us; bf16 134 -> 68, 96 -> 44, 95 -> 47 us; on
    the uniform graph of the same size +-3 % -- hence the skew test (one pass over the degrees per structure, cached): the
    share of lane-slots that eight consecutive rows fill, 0.73 on the uniform graph, 0.32 on the R-MAT one.
    A forward call whose hash is still in flight keeps the ordinary launch: waiting would drain the stream."""
    if MODE == "off" or _plan.transient() or fp is None or getattr(fp, "_key", None) is None:
        return False
    if nnz < ORDERED_MIN_EDGES or n_src >= (1 << 24) or n_src * row_bytes >= (1 << 32) or row_bytes >= (1 << 22):
        return False
    key = fp.key()
    hit = _SKEW.get(key)
    if hit is None:
        if len(_SKEW) > 256:
            _SKEW.clear()
        hit = _SKEW[key] = skewed(rowptr)
    return hit


def skewed(rowptr):
    """The skew test of ordered_wanted (one pass over the degrees + one host read): do eight consecutive rows fill less than
    ORDERED_MAX_FILL of the lane-slots of their longest?"""
    deg = (rowptr[1:] - rowptr[:-1]).float()
    pad = (-deg.numel()) % 8
    if pad:
        deg = torch.cat([deg, deg.new_zeros(pad)])
    fill = float(deg.sum() / (deg.view(-1, 8).max(1).values.sum() * 8).clamp(min=1.0))
    return fill < ORDERED_MAX_FILL


class _Cache:
    def __init__(self):
        self.budget = int(os.environ.get("COGDL_AMD_XCD_CACHE_MB", "8192")) << 20
        self.bytes = 0
        self.lru = collections.OrderedDict()

    def get(self, key, make):
        p = self.lru.get(key)
        if p is not None:
            self.lru.move_to_end(key)
            return p
        p = make()
        self.lru[key] = p
        self.bytes += p.nbytes()
        while self.bytes > self.budget and len(self.lru) > 1:
            _, old = self.lru.popitem(last=False)
            self.bytes -= old.nbytes()
        return p

    def clear(self):
        self.lru.clear()
        self.bytes = 0


XPLANS = _Cache()


def csr_plan(fp, rowptr, colind, split=None):
    """The plan of the structure itself, under its fingerprint (waits for the hash: one host synchronisation per call --
    `wanted()` only says yes to launches of hundreds of microseconds; with install(structure_memo=True) the key is memoised).
    split: rows of more than this many edges are cut by owner (default SPLIT; fp32 csr_spmm passes its exact-row bound)."""
    split = SPLIT if split is None else int(split)
    return XPLANS.get(("csr", split, PIECE) + fp.key(), lambda: build(rowptr, colind, split=split))


def csc_plan(fp, csc, split=None):
    """The plan of the transpose (a CscPlan): per-edge operands are indexed through its perm."""
    split = SPLIT if split is None else int(split)
    return XPLANS.get(("csc", split, PIECE) + fp.key(), lambda: build(csc.colptr, csc.rowind, eid_base=csc.perm, split=split))


# ------------------------------------------------------------------------------------------------------------ the policy
# Does a launch run over a plan, and cut at which row length?  The operators pass facts and launch what comes back (the rules in
# prose: DESIGN.md).  H = wanted(): needs no key.  S = ordered_wanted(): a Fingerprint whose hash is in flight gets a no.  E =
# cogdl_hip_exact_row_edges(nnz).  Decisions go through plan.taped_choice: a capture replays what its recorded eager run decided.


def forced():
    return MODE == "force"


def aligned(t, nbytes):
    """Does the dense operand start on a multiple of `nbytes`?  A contiguous view into a larger allocation (a slice of a flat
    parameter buffer, a narrow of a packed batch, an upstream gradient that is one) need not.  The plan kernels take 16-byte
    operands and the sweep kernels 8-byte ones (csrc/spmm.hip), the ordinary launch narrows its lanes instead: such an operand
    is a reason for the ordinary launch, decided here and never found out from a status code."""
    return t.data_ptr() % nbytes == 0


def spmm_split(fp, rowptr, m, nnz, x):
    """csr_spmm, either direction: the row length to cut at, or None (the ordinary launch).  fp: the structure's Fingerprint if its
    key counts as known to this call, else None.
      fp32    H: cut at E -- rows up to E stay whole and bit-identical to the reference loop; only the rows the ordinary path
              already re-associates (its long-row pieces) are cut by owner XCD instead of into contiguous chunks.  Measured on the
              Reddit-shaped graph, F = 64: see profiles/r06_xcd_spmm_fp32.txt.
      16-bit  H: cut at SPLIT (no bit-exact contract to keep; one plan per structure with the fused GAT operator).  Measured on the
              Reddit-shaped graph (profiles/r06_xcd_spmm_split.txt): bf16 F = 64 1524 -> 1316 us, F = 128 3241 -> 2291 us; at
              split 64 / 1024: 1386 / 1345 us.  (Before the hub rows' part records were merged by whole workgroups -- rowreduce.h:
              rowreduce_vcombine_kernel -- the same plan LOST: 1512 -> 1638 us, profiles/r06_xcd_quick.txt.)
      else S  cut at E whatever the dtype (rows up to it stay whole and sequential, as in the ordinary launch).
    An x that is not 16-byte aligned: None in every mode, "force" included (see aligned)."""
    if x.dim() != 2 or x.dtype not in _lib.DTYPE_CODE or not aligned(x, 16):
        return None
    n_src, row_bytes = x.shape[0], x.shape[1] * x.element_size()
    hub = wanted(m, nnz, n_src, row_bytes)
    if MODE == "force":  # (kept as is: S is not consulted, and fp32 is cut at SPLIT too)
        return SPLIT if hub else None
    if hub and x.dtype != torch.float32:
        return SPLIT
    return int(_lib.hip().cogdl_hip_exact_row_edges(nnz)) if hub or ordered_wanted(fp, rowptr, m, nnz, n_src, row_bytes) else None


def spmm_forward(fp, rowptr, colind, x):
    """SPMMFunction.forward -> (split, plan) or (None, None).  fp: the call's Fingerprint; None where the call hashed nothing (no
    gradient wanted, no memo knows the tensors): a hub-heavy launch then hashes here, for its plan's key.  A memoised structure
    waits for its key (ONCE per structure), and so does the recorded eager run of cogdl_amd.graphs.capture (kept as is: under ANY
    tape, where gat_forward asks for a recording one); the identity memo has its key once a backward pass has asked."""
    if _plan.transient():
        return None, None

    def decide():
        if fp is not None and (_plan.taping() or _plan.memoised(rowptr)):
            fp.wait()
        split = spmm_split(fp, rowptr, rowptr.numel() - 1, colind.numel(), x)
        if split is None:
            return None, None
        return split, csr_plan(fp if fp is not None else _plan.fingerprint_of(rowptr, colind, x.shape[0]), rowptr, colind, split)

    return _plan.taped_choice("csr_spmm.forward", decide)


def spmm_backward(fp, csc, grad_out, took_plan):
    """SPMMFunction.backward over the transpose `csc` (a plan.CscPlan) -> (split, plan) or (None, None).  PLANS.get has waited for
    the hash, but the key counts only after a plan forward or from the structure's SECOND sighting on: no plan build for one-offs."""
    def decide():
        split = spmm_split(fp if (took_plan or csc.sightings > 1) else None, csc.colptr, csc.colptr.numel() - 1,
                           csc.rowind.numel(), grad_out)
        return split, (csc_plan(fp, csc, split) if split is not None else None)

    return _plan.taped_choice("csr_spmm.backward", decide)


SWEEP_ROW_BYTES = 512            # fp32 F = 128: the one width the sweep kernel takes (csrc/rowsweep.h)
SWEEP_MIN_TABLE_BYTES = 32 << 20  # below: the gathered table fits the eight L2s together, the ordinary launch already hits


def spmm_backward_sweep(csc, grad_out, round_rows=None):
    """SPMMFunction.backward, asked only when spmm_backward said "ordinary": does the launch over the transpose `csc` (a
    plan.CscPlan) walk its sweep layout (cogdl_amd/sweepplan.py: every wave walks the gathered table top to bottom, bit-identical
    results)?  fp32 2-D operands of 512-byte rows; a table beyond the eight L2s and of at most 2^23 rows; a transpose without
    hub rows (the sweep reduces every row sequentially); from the structure's SECOND sighting on (a one-off never pays the
    layout's sort); MODE auto only; never for transient structures or under a plan tape (captured steps keep the ordinary
    launch); and only while all rows fit ONE round of the grid -- with two rounds the second starts when the first wave
    finishes, not when the table's top comes round again, and the ideal hit rate drops from 0.54 to 0.35.
    round_rows: rows of one round for this width (default: asked of the library, which asks the device)."""
    if MODE != "auto" or _plan.transient() or _plan.taping():
        return False
    if grad_out.dim() != 2 or grad_out.dtype != torch.float32 or grad_out.shape[1] * grad_out.element_size() != SWEEP_ROW_BYTES:
        return False
    if not aligned(grad_out, 8):  # (the sweep kernel's float2 lanes; the ordinary launch narrows instead)
        return False
    from . import sweepplan

    n_src = grad_out.shape[0]
    if csc.sightings < 2 or csc.nnz == 0 or n_src > sweepplan.MAX_TABLE_ROWS or n_src * SWEEP_ROW_BYTES < SWEEP_MIN_TABLE_BYTES:
        return False
    if round_rows is None:
        round_rows = sweepplan.round_rows(grad_out.shape[1], grad_out.dtype)
    if csc.n_cols > round_rows:
        return False
    return not csc.has_hub_columns()


SWEEP_FORWARD_MAX_OUT_OF_ORDER = 1.0 / 8  # a condition, not a tuned number: rows that are an ascending run plus an appended self loop
                                          # sit at 1 / (degree + 1) (the benchmark's graph: 0.0628); rows in random column order near
                                          # 1 - H(d) / d (0.78 at 14.8 edges per row) -- their walk has no order to speak of


def spmm_forward_sweep_shape(m, nnz, n_src, k, dtype, round_rows=None):
    """The part of spmm_forward_sweep that needs no layout (the backward pass asks it before it builds one): MODE auto, no
    transient structure, no plan tape, plan.VERIFY_HITS off (the forward has no host-side hit to verify: it trusts the 64-bit
    hash on the device), fp32 rows of 512 bytes, a table beyond the eight L2s and of at most 2^23 rows, all rows in one round."""
    if MODE != "auto" or _plan.transient() or _plan.taping() or _plan.VERIFY_HITS:
        return False
    if dtype != torch.float32 or k * 4 != SWEEP_ROW_BYTES or nnz == 0:
        return False
    from . import sweepplan

    if n_src > sweepplan.MAX_TABLE_ROWS or n_src * SWEEP_ROW_BYTES < SWEEP_MIN_TABLE_BYTES:
        return False
    if round_rows is None:
        round_rows = sweepplan.round_rows(k, dtype)
    return m <= round_rows


def spmm_forward_sweep(fp, rowptr, colind, x, round_rows=None):
    """SPMMFunction.forward, asked only when spmm_forward said "ordinary": does the call SPECULATE on the forward sweep layout
    (cogdl_amd/sweepplan.py: build_forward) of a structure seen before?  -> that layout, or None.  The call's own hash is
    still in flight, so the host cannot know whether this IS that structure; the device can (the hash kernel runs on the same
    stream in front of the SpMM): the sweep is enqueued guarded "run if the hash is the layout's", the ordinary launch
    guarded "run if it is not" (operators/spmm.py: csr_spmm_sweep_forward_raw).  Yes only if: the conditions of
    spmm_forward_sweep_shape; the stream is not capturing; a candidate with a layout is registered for the call's (device, m,
    nnz, n_src) and the call hashed into device memory (Fingerprint.dev); the layout has no row above the exact-row bound (the
    sweep reduces every row sequentially) and at most SWEEP_FORWARD_MAX_OUT_OF_ORDER of its edges behind their row's
    running maximum.  Never waits, never reads back."""
    if fp is None or getattr(fp, "dev", None) is None or x.dim() != 2 or not aligned(x, 8):
        return None  # (an x off the float2 lanes of BOTH guarded launches: refused here, before either is enqueued)
    if not spmm_forward_sweep_shape(rowptr.numel() - 1, colind.numel(), x.shape[0], x.shape[1], x.dtype, round_rows):
        return None
    from . import sweepplan

    sp = sweepplan.candidate(fp.meta)
    if sp is None or sp.hash is None or not sweepplan.takeable(sp):
        return None
    if torch.cuda.is_current_stream_capturing():
        return None
    return sp


def gat_forward(fp, rowptr, colind, n_src, row_bytes):
    """FusedGATFunction.forward -> the structure's plan (cut at SPLIT) or None.  row_bytes: None for an operand the kernels refuse.
    H; else S -- a memoised structure and the recorded eager run of cogdl_amd.graphs.capture wait for the key."""
    def decide():
        if row_bytes is None:
            return None
        m, nnz = rowptr.numel() - 1, colind.numel()
        if not wanted(m, nnz, n_src, row_bytes):
            if _plan.memoised(rowptr) or _plan.recording():  # (kept as is: a RECORDING tape, where spmm_forward asks for any)
                fp.wait()
            if not ordered_wanted(fp, rowptr, m, nnz, n_src, row_bytes):
                return None
        return csr_plan(fp, rowptr, colind)

    return _plan.taped_choice("fused_gat.forward", decide)


def gat_backward(fp, csc, rowptr, colind, n_src, row_bytes, took_plan):
    """FusedGATFunction.backward -> (plan of the structure, plan of its transpose `csc`) or None: the forward ran the plan kernels,
    or S from the structure's second sighting on (see spmm_backward).  (kept as is: H is not asked again)"""
    def decide():
        if took_plan or (csc.sightings > 1 and ordered_wanted(fp, rowptr, rowptr.numel() - 1, colind.numel(), n_src, row_bytes)):
            return csr_plan(fp, rowptr, colind), csc_plan(fp, csc)
        return None

    return _plan.taped_choice("fused_gat.backward", decide)


EDGE_LIST_MIN_COLUMNS = 65  # (narrower rows: the plan's launch measured 8-15 % SLOWER than the ordinary one: EdgePlan.xcd)


def edge_list_wanted(edges, k):
    """gspmm of k columns over a memoised edge list (operators/ops.py: EdgePlan.xcd): skewed lists from their second use on."""
    nnz = edges.perm.numel()
    if MODE == "off" or nnz == 0:
        return False
    if MODE == "force":
        return True
    if edges.uses < 2 or nnz < ORDERED_MIN_EDGES or k < EDGE_LIST_MIN_COLUMNS:
        return False
    if edges.skewed is None:
        if torch.cuda.is_current_stream_capturing():  # (the skew test reads back: never inside a capture)
            return False
        edges.skewed = skewed(edges.rowptr)
    return edges.skewed
