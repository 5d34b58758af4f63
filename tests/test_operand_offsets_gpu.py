"""Every operator on dense operands that start mid-allocation (the contract paragraph of INTEGRATION.md; tests/_offset.py).

Almost every kernel picks its vector width at launch from the address of its operands, so a contiguous tensor whose
data_ptr() is only element-aligned -- a slice of a flat parameter buffer, a narrow of a packed batch, an upstream gradient that
is such a view -- runs ANOTHER instantiation than a fresh tensor of the same values.  One table (ROWS) names, per operator and
shape: how its inputs are built, which arguments are dense floating-point operands (the upstream gradient is the operand
"grad", handed to out.backward as the shifted view itself), and the reference and rule to judge by.  The parametrisation is
row x operand x offset (fp32: 1 and 2 elements = 4 and 8 bytes; 16-bit: 1, 2 and 4 elements = 2, 4 and 8 bytes), one operand
at a time, plus one case per row with every operand shifted by one element.  Judgement of every case:

  a. the call returns: no BackendError, and under warnings.simplefilter("error") no TorchRouteWarning;
  b. every result satisfies the rule the operator's own test applies to the aligned call, against the same reference (the
     rules are imported or quoted from those tests, row by row below);
  c. where that rule is bit equality the result is also byte-identical to the aligned call's; elsewhere the test prints
     whether it was;
  d. guards_intact for every shifted operand, written ones (out=, acc=) included, whose own contents are the result.

The control: width 7 (fp32) is vector width 1 at every alignment, so the instantiation cannot change and every result of a
control row has to be byte-identical to the aligned call's -- a failure there is a bug of this harness.  (The width-7 rows under
xcdplan.MODE = "force" are not controls: there an offset operand changes the LAUNCH, plan to ordinary, whatever the width.)

Byte-identical across alignments (asserted): both sweep paths of csrspmm, scatter_max (values and argmax at every row length,
the CSC backward on short sources), segment_pool and sort_pool (both directions), gather_rows_by_id, the gradient of gspmm's edge
feature, edge_softmax (the clone), every width-7 control; and ON THE ROWS UP TO THE EXACT-ROW BOUND -- where the operators' own
rule is bit equality -- fp32 csrspmm forward and grad_x, csr_spmm_raw(out=), the fused epilogue (output and grad_x), the int64
segmented csrspmm, gspmm (output, grad_x), mhspmm fp32 (output, grad_feat), rel_gspmm (output, grad_x) and filter_step (out and
acc).  A longer row is cut into pieces per lane group, and the number of lane groups follows the vector width, so its sum is
re-associated when the width changes (fp32 F = 64: the 1000-edge row of the graph; F = 8, 6, 128 and 7 keep their lane groups and
came out identical on every row): those rows are judged by the rule alone.

Printed, not asserted (the rule is a tolerance), as they came out on an MI355X.  The same bytes in every case: the head
projection (both outputs and the three gradients), linear_wgrad, disen_route and gen_aggregate's output and edge-term gradient
under an offset upstream gradient, the fused epilogue's grad_x and grad_bias, 16-bit csrspmm under xcdplan.MODE = "force"
(forward, grad_x, grad_w), 16-bit mhspmm's output and grad_att.  Different bytes in some cases, inside the rule: csr_sddmm and
every weight gradient that is one (grad_w of csrspmm and gspmm, fp32 grad_att of mhspmm: the dot products re-associate with the
lane width), fp32 csrspmm under "force" (an offset operand takes the ordinary launch, which cuts long rows elsewhere than the
plan), fused GAT in fp32 and bf16 (all four results, ordinary launch and forced plan), gen_aggregate's grad_x, rel_gspmm's grad_rel, 16-bit mhspmm's grad_feat,
and tall_skinny_matmul (an x off its 16-byte lanes takes torch's product).

edge_softmax clones an offset operand (operators/edge_softmax.py: _aligned), so its C-ABI row kernels for unaligned operands
stay unreachable from Python; the case proves that the clone's result and gradient land where autograd expects them.  The contrastive loss (operators/contrast.py) is a torch composition: no kernel
of this library sees its addresses.

A second, smaller parametrisation passes every dense operand as a NON-contiguous view (a column slice of a wider tensor) and
asserts the bytes of the call on t.contiguous() where the wrapper copies, BackendError where the docstring refuses (filter_step,
gather_rows_by_id); and EVERY differentiable row of the table runs once more with its upstream gradient(s) as the stride-0
expansion of a scalar one -- out.sum().backward(), for the head projection (h_l.sum() + h_r.sum()).backward()."""
import functools
import types
import warnings

import numpy as np
import pytest
import torch

import _disen_cases as DC
import _gat_halfprec as GH
import _gen_cases as G
import _halfprec as hp
import _offset as O
import _prone_cases as PC
import _readout_cases as RC
from cogdl_amd import _lib, bigcsr, fused, linear, pipeline, plan, sweepplan, synth, xcdplan
from cogdl_amd.operators import disen as disen_mod
from cogdl_amd.operators import fused_gat as gat_mod
from cogdl_amd.operators import genaggr as genaggr_mod
from cogdl_amd.operators import ops as ops_mod
from cogdl_amd.operators import readout as readout_mod
from cogdl_amd.operators import relational as rel_mod
from cogdl_amd.operators import spmm as spmm_mod
from cogdl_amd.operators.edge_softmax import csr_edge_softmax
from cogdl_amd.operators.mhspmm import csrmhspmm
from cogdl_amd.operators.scatter_max import scatter_max, scatter_max_fp
from cogdl_amd.operators.spectral import filter_step
from cogdl_amd.operators.spmm import csr_sddmm_raw, csr_spmm_raw, csrspmm, csrspmm_fused
from oracle import oracle
from test_spmm_gpu import assert_rows_match  # rows up to the exact-row bound: the oracle's bytes; longer rows: 1e-5 of the terms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = G.N
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
OFFSETS = {4: (1, 2), 2: (1, 2, 4)}  # element size -> offsets in elements
WIDTHS = (8, 6, 64, 128, 7)          # 7: the control


def _rand(*shape, seed=0, dtype=F32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------ the graph
@functools.lru_cache(None)
def _csr():
    """_gen_cases.graph() as CSR (destination rows, the caller's edge order inside a row) + weights + its transpose."""
    row, col = G.graph()
    order = torch.argsort(row, stable=True)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=N), 0)
    colind = col[order].int()
    val = torch.rand(colind.numel(), generator=torch.Generator().manual_seed(11)) + 0.5
    g = types.SimpleNamespace(rowptr=rowptr.int(), colind=colind, val=val, nnz=colind.numel(), order=order)
    g.deg = np.diff(g.rowptr.numpy())
    g.row = np.repeat(np.arange(N), g.deg)
    g.col = colind.numpy().astype(np.int64)
    colptr, rowind, w_t, perm = oracle.csr2csc(g.rowptr, g.colind, g.val, n_cols=N)
    g.colptr, g.rowind, g.w_t, g.perm = np.asarray(colptr), np.asarray(rowind), np.asarray(w_t), np.asarray(perm)
    g.col_deg = np.diff(g.colptr)
    g.thresh = int(_lib.hip().cogdl_hip_exact_row_edges(g.nnz))
    assert g.thresh == 128 and g.deg.max() == 1000 and g.col_deg.max() >= 400
    return g


@functools.lru_cache(None)
def _csr_dev():
    """The same index tensors for every case: the plans are built once."""
    g = _csr()
    return g.rowptr.to(DEV), g.colind.to(DEV)


@functools.lru_cache(None)
def _coo_dev():
    return tuple(t.to(DEV) for t in G.graph())


def _edge_sum(terms, index, n):
    """float64 sum over the edges, and the sum of the absolute terms."""
    want, scale = np.zeros((n,) + terms.shape[1:]), np.zeros((n,) + terms.shape[1:])
    np.add.at(want, index, terms)
    np.add.at(scale, index, np.abs(terms))
    return want, scale


def _within(got, want, scale, rel=1e-5, floor=1e-6, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, bound = np.abs(got - want), rel * np.asarray(scale, dtype=np.float64) + floor
    assert np.isfinite(got).all() and np.all(err <= bound), "%s: err %.3e beyond the bound" % (what, float((err - bound).max()))


def _short_exact(got, want, short, scale, what):
    """Rows of at most the exact-row bound: the reference's bytes; every row: 1e-5 of the summands (re-association only)."""
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got[short].tobytes() == want[short].astype(np.float32).tobytes(), what
    _within(got, want, scale, floor=1e-6, what=what)


# ----------------------------------------------------------------------------------------------------------- the cases
class Case:
    """operands: name -> CPU tensor (every dense floating-point operand; "grad" is the upstream gradient).  run(ops) -> results
    (name -> tensor) from device operands; judge(results on the CPU) asserts rule (b); exact: the result names rule (c) binds
    (a name -> row mask restricts it to those rows); control: every result is bound; setup(monkeypatch): switches of the path;
    cleanup(): undoes what setup left outside monkeypatch's reach, run after every call whatever happened in it, asserts
    nothing; verify(shift): asserts which path the call took (shift None: the aligned call), only after a call that returned."""

    def __init__(self, operands, run, judge, exact=(), written=(), control=False, setup=None, cleanup=None, verify=None):
        self.operands, self.run, self.judge, self.written = operands, run, judge, tuple(written)
        self.exact = dict((k, None) for k in exact) if not isinstance(exact, dict) else exact
        self.control, self.setup, self.cleanup, self.verify = control, setup, cleanup, verify
        self._aligned = None

    def device_operands(self, shift):
        """shift: name -> offset in elements.  -> (ops, guards)"""
        ops, guards = {}, {}
        for name, t in self.operands.items():
            if name in shift:
                ops[name], guards[name] = O.shifted(t, shift[name], device=DEV)
            else:
                ops[name] = t.to(DEV).clone()
        return ops, guards

    def call(self, ops, monkeypatch, shift=None):
        try:
            if self.setup is not None:
                self.setup(monkeypatch)
            with warnings.catch_warnings():
                warnings.simplefilter("error")  # the kernel's route: no TorchRouteWarning
                res = self.run(ops)
            torch.cuda.synchronize()
            res = dict((k, v.detach().cpu()) for k, v in res.items())
        finally:
            if self.cleanup is not None:
                self.cleanup()
        if self.verify is not None:
            self.verify(shift)
        return res

    def aligned(self, monkeypatch):
        if self._aligned is None:
            res = self.call(self.device_operands({})[0], monkeypatch)
            self.judge(res)
            self._aligned = res
        return self._aligned


def _autograd(fn, diff, extra=None):
    """run(): out = fn(ops) with the operands `diff` as leaves, out.backward(ops["grad"]) -> out, g_<name>."""
    def run(o):
        for n in diff:
            o[n].requires_grad_()
        out = fn(o)
        out.backward(o["grad"])
        res = {"out": out}
        res.update(("g_" + n, o[n].grad) for n in diff)
        if extra is not None:
            res.update(extra(o, out))
        return res

    return run


# ---- csrspmm: the ordinary launch, forward and backward (tests/test_spmm_gpu.py: bit equality with the oracle up to the
#      exact-row bound, 1e-5 of the terms beyond; grad_w = csr_sddmm: 1e-5 of the terms, tests/test_ops_gpu.py::test_sddmm)
def _spmm_reference(k, weighted, x, gr):
    g = _csr()
    val = g.val if weighted else None
    ref = types.SimpleNamespace()
    ref.out = oracle.csr_spmm(g.rowptr, g.colind, val, x)
    ref.out_abs = oracle.csr_spmm_abs(g.rowptr, g.colind, val, x)
    w_t = g.w_t if weighted else None
    ref.gx = oracle.csr_spmm(g.colptr, g.rowind, w_t, gr)
    ref.gx_abs = oracle.csr_spmm_abs(g.colptr, g.rowind, w_t, gr)
    ref.gw = oracle.csr_sddmm(g.rowptr, g.colind, gr, x)
    ref.gw_abs = (gr.abs().numpy()[g.row] * x.abs().numpy()[g.col]).sum(1)
    return ref


def _judge_spmm(ref, weighted):
    g = _csr()

    def judge(res):
        assert_rows_match(res["out"].numpy(), ref.out, g.rowptr.numpy(), g.nnz, ref.out_abs)
        assert_rows_match(res["g_x"].numpy(), ref.gx, g.colptr, g.nnz, ref.gx_abs)
        if weighted:
            _within(res["g_w"].numpy(), ref.gw, ref.gw_abs, floor=1e-7, what="grad_w")

    return judge


def _short_rows():
    """Rule (c) for csr_spmm's family: the rows up to the exact-row bound (destinations for `out`, sources for `g_x`).  A longer row
    is cut into pieces per lane group, and the number of lane groups follows the vector width: fp32 F = 64 is 16 lanes of 4
    floats on 16-byte operands and a whole wave of single floats 4 bytes in, so its 1000-edge row is re-associated -- inside the
    rule, not the same bytes (measured: F = 8, 6, 128 and 7 keep their lane groups and their bytes)."""
    g = _csr()
    return {"out": g.deg <= g.thresh, "g_x": g.col_deg <= g.thresh}


@functools.lru_cache(None)
def spmm_case(k, weighted):
    g = _csr()
    x, gr = _rand(N, k, seed=k), _rand(N, k, seed=1000 + k)
    operands = {"x": x, "grad": gr}
    if weighted:
        operands["w"] = g.val
    rp, ci = _csr_dev()
    run = _autograd(lambda o: csrspmm(rp, ci, o["x"], o.get("w"), False), ("x", "w") if weighted else ("x",))

    def setup(monkeypatch):
        monkeypatch.setattr(xcdplan, "MODE", "off")

    return Case(operands, run, _judge_spmm(_spmm_reference(k, weighted, x, gr), weighted), exact=_short_rows(),
                control=(k == 7), setup=setup)


# ---- csrspmm with xcdplan.MODE = "force" (tests/test_xcd_gpu.py: tol * sum |terms| with its TOL / ATOL for fp32; every 16-bit
#      result: _halfprec.assert_close with the row degree as terms)
XCD_TOL = {F32: 2e-5}
_XCD_CALLS = []
_REAL_GAT_XCD = _lib.hip().cogdl_hip_gat_fwd_xcd
_REAL = dict((n, getattr(spmm_mod, n)) for n in ("csr_spmm_xcd_raw", "csr_spmm_sweep_forward_raw", "csr_spmm_sweep_raw"))


@functools.lru_cache(None)
def xcd_case(k, dtype):
    g = _csr()
    x, gr, w = _rand(N, k, seed=k, dtype=dtype), _rand(N, k, seed=1000 + k, dtype=dtype), g.val.to(dtype)
    rp, ci = _csr_dev()
    run = _autograd(lambda o: csrspmm(rp, ci, o["x"], o["w"], False), ("x", "w"))
    w64, x64, g64 = _np64(w), _np64(x), _np64(gr)
    out, out_abs = _edge_sum(w64[:, None] * x64[g.col], g.row, N)
    gx, gx_abs = _edge_sum(w64[:, None] * g64[g.row], g.col, N)
    dots = g64[g.row] * x64[g.col]

    def judge(res):
        if dtype == F32:
            _within(res["out"], out, out_abs, rel=XCD_TOL[F32], floor=1e-30, what="forward")
            _within(res["g_x"], gx, gx_abs, rel=XCD_TOL[F32], floor=1e-30, what="grad_x")
            _within(res["g_w"], dots.sum(1), np.abs(dots).sum(1), floor=1e-7, what="grad_w")
        else:
            assert all(res[n].dtype == dtype for n in ("out", "g_x", "g_w"))
            hp.assert_close(res["out"], out, out_abs, g.deg[:, None], dtype, "forward")
            hp.assert_close(res["g_x"], gx, gx_abs, g.col_deg[:, None], dtype, "grad_x")
            hp.assert_close(res["g_w"], dots.sum(1), np.abs(dots).sum(1), k, dtype, "grad_w")

    def setup(monkeypatch):
        monkeypatch.setattr(xcdplan, "MODE", "force")
        real = _REAL["csr_spmm_xcd_raw"]
        del _XCD_CALLS[:]
        xcdplan.XPLANS.clear()
        monkeypatch.setattr(spmm_mod, "csr_spmm_xcd_raw", lambda *a, **kw: (_XCD_CALLS.append(1), real(*a, **kw))[1])

    def verify(shift):
        if shift is None:
            assert len(_XCD_CALLS) == 2, "the aligned call did not run over the plan in both directions"
        else:  # an x off its 16-byte lanes keeps the forward off the plan, an upstream gradient the backward
            assert len(_XCD_CALLS) == 2 - ("x" in shift) - ("grad" in shift), (shift, len(_XCD_CALLS))

    return Case({"x": x, "grad": gr, "w": w}, run, judge, setup=setup, cleanup=xcdplan.XPLANS.clear, verify=verify)


# ---- csrspmm on the sweep-backward and the speculative sweep-forward path (tests/test_sweep_gpu.py, test_sweep_forward_gpu.py:
#      the oracle's bytes; the structure has no row beyond the exact-row bound in either direction)
_SWEEP_CALLS = {"pair": 0, "sweep": 0}


@functools.lru_cache(None)
def sweep_case():
    sg = synth.scaled(300, 8, seed=4)
    k = 128
    x, gr = _rand(sg.n_cols, k, seed=3), _rand(sg.num_nodes, k, seed=4)
    gd = sg.to(DEV)
    colptr, rowind, w_t, _ = oracle.csr2csc(sg.rowptr, sg.colind, sg.weight)
    want_out = oracle.csr_spmm(sg.rowptr, sg.colind, sg.weight, x).tobytes()
    want_gx = oracle.csr_spmm(colptr, rowind, w_t, gr).tobytes()
    assert int(sg.degrees().max()) <= 128 and int(np.diff(np.asarray(colptr)).max()) <= 128

    def run(o):
        o["x"].requires_grad_()
        for _ in range(4):  # sightings 1 .. 4: the backward sweeps from the second on, the forward speculates from the third
            o["x"].grad = None
            # fresh int32 copies of the structure every call, as CogDL's dispatcher makes them
            out = csrspmm(gd.rowptr.long().int(), gd.colind.long().int(), o["x"], o["w"], True)
            out.backward(o["grad"])
        return {"out": out, "g_x": o["x"].grad}

    def judge(res):
        assert _bytes(res["out"]) == want_out and _bytes(res["g_x"]) == want_gx

    def setup(monkeypatch):
        monkeypatch.setattr(xcdplan, "MODE", "auto")
        monkeypatch.setattr(xcdplan, "SWEEP_MIN_TABLE_BYTES", 0)  # (the table-size threshold, not a 70,000-row graph)
        monkeypatch.setattr(plan, "VERIFY_HITS", False)
        plan.PLANS.clear()
        plan.clear_identity_memo()
        _SWEEP_CALLS.update(pair=0, sweep=0)
        real_pair, real_sweep = _REAL["csr_spmm_sweep_forward_raw"], _REAL["csr_spmm_sweep_raw"]

        def pair(*a, **kw):
            _SWEEP_CALLS["pair"] += 1
            return real_pair(*a, **kw)

        def sweep(*a, **kw):
            _SWEEP_CALLS["sweep"] += 1
            return real_sweep(*a, **kw)

        monkeypatch.setattr(spmm_mod, "csr_spmm_sweep_forward_raw", pair)
        monkeypatch.setattr(spmm_mod, "csr_spmm_sweep_raw", sweep)

    def cleanup():
        plan.PLANS.clear()
        plan.clear_identity_memo()

    def verify(shift):
        x_ok = shift is None or shift.get("x", 0) % 2 == 0      # 8-byte lanes: an offset of two floats still sweeps
        g_ok = shift is None or shift.get("grad", 0) % 2 == 0
        assert _SWEEP_CALLS == {"pair": 2 if x_ok else 0, "sweep": 3 if g_ok else 0}, (shift, dict(_SWEEP_CALLS))

    return Case({"x": x, "grad": gr, "w": sg.weight}, run, judge, exact=("out", "g_x"), setup=setup, cleanup=cleanup,
                verify=verify)


# ---- csr_spmm_raw(out=): out += A x (tests/test_spmm_gpu.py::test_accumulate_mode: continuing the sequential sum from out)
@functools.lru_cache(None)
def acc_case(k):
    g = _csr()
    x, base = _rand(N, k, seed=k), _rand(N, k, seed=2000 + k)
    rp, ci = _csr_dev()
    # the oracle: every row starts with one more edge of weight 1 to a row of its own that holds `base`
    deg1 = g.deg + 1
    rowptr = np.concatenate([[0], np.cumsum(deg1)]).astype(np.int32)
    colind, val = np.empty(rowptr[-1], dtype=np.int32), np.empty(rowptr[-1], dtype=np.float32)
    first = rowptr[:-1]
    colind[first], val[first] = N + np.arange(N), 1.0
    rest = np.ones(rowptr[-1], dtype=bool)
    rest[first] = False
    colind[rest], val[rest] = g.colind.numpy(), g.val.numpy()
    both = torch.cat([x, base])
    want = oracle.csr_spmm(rowptr, colind, val, both)
    scale = oracle.csr_spmm_abs(rowptr, colind, val, both)
    short = g.deg <= g.thresh

    def run(o):
        res = csr_spmm_raw(rp, ci, o["w"], o["x"], out=o["out"])
        assert res is o["out"]
        return {"out": o["out"]}

    def setup(monkeypatch):
        monkeypatch.setattr(xcdplan, "MODE", "off")

    return Case({"x": x, "out": base, "w": g.val}, run, lambda res: _short_exact(res["out"], want, short, scale, "out += A x"),
                exact={"out": short}, written=("out",), control=(k == 7), setup=setup)


# ---- the fused epilogue (tests/test_fused_gpu.py: the bytes of relu(in_norm * (A (out_norm * x)) + bias) on short rows, 1e-5 of the
#      terms on all; grad_x 1e-5 of the terms + 1e-6 against the oracle's formula, grad_bias rtol 1e-5 / atol 1e-5)
@functools.lru_cache(None)
def epilogue_case(k):
    g = _csr()
    gen = torch.Generator().manual_seed(300 + k)
    x, gr = torch.randn(N, k, generator=gen), torch.randn(N, k, generator=gen)
    s_out, s_in, b = torch.rand(N, 1, generator=gen) + 0.2, torch.rand(N, 1, generator=gen) + 0.2, torch.randn(k, generator=gen)
    rp, ci = _csr_dev()
    run = _autograd(lambda o: csrspmm_fused(rp, ci, o["x"], o["w"], o["out_norm"], o["in_norm"], o["bias"], True), ("x", "bias"))
    pre = s_in.numpy() * oracle.csr_spmm(g.rowptr, g.colind, g.val, s_out * x) + b.numpy()
    want = np.maximum(pre, 0).astype(np.float32)
    scale = s_in.numpy() * oracle.csr_spmm_abs(g.rowptr, g.colind, g.val, s_out * x) + np.abs(b.numpy())
    short = g.deg <= g.thresh

    def judge(res):
        _short_exact(res["out"], want, short, scale, "epilogue")
        gm = (gr * (res["out"] > 0)) * s_in
        _within(res["g_x"], s_out.numpy() * oracle.csr_spmm(g.colptr, g.rowind, g.w_t, gm),
                s_out.numpy() * oracle.csr_spmm_abs(g.colptr, g.rowind, g.w_t, gm), floor=1e-6, what="grad_x")
        np.testing.assert_allclose(res["g_bias"].numpy(), (gr * (res["out"] > 0)).double().sum(0).numpy(), rtol=1e-5, atol=1e-5)

    return Case({"x": x, "w": g.val, "out_norm": s_out, "in_norm": s_in, "bias": b, "grad": gr}, run, judge,
                exact=_short_rows(), control=(k == 7))


# ---- the int64 segmented csrspmm with two segments (tests/test_bigcsr_gpu.py: the rule of the 32-bit operator)
@functools.lru_cache(None)
def big_case(k):
    g = _csr()
    x, gr = _rand(N, k, seed=k), _rand(N, k, seed=1000 + k)
    rp64, ci = _csr_dev()[0].long(), _csr_dev()[1]
    ref = _spmm_reference(k, True, x, gr)

    def fn(o):
        out = csrspmm(rp64, ci, o["x"], o["w"], False)
        assert bigcsr.plan_of(rp64, ci, N).n_segments == 2
        return out

    def setup(monkeypatch):
        _lib.hip().cogdl_hip_set_tuning(15, 2000)  # edges per segment: the graph's 3,700 edges in two segments
        bigcsr.clear_plans()

    def cleanup():
        _lib.hip().cogdl_hip_set_tuning(15, 0)
        bigcsr.clear_plans()

    return Case({"x": x, "grad": gr, "w": g.val}, _autograd(fn, ("x", "w")), _judge_spmm(ref, True), exact=_short_rows(),
                control=(k == 7), setup=setup, cleanup=cleanup)


# ---- gspmm with a per-edge vector feature (tests/test_message_ops_gpu.py: the oracle's bytes while a destination has at most the
#      exact-row bound of edges, 1e-5 of the summands for hub destinations; grad_x: CPU autograd's bytes while a source has at most
#      that many out-edges; grad of the edge feature: its bytes; grad of the edge weight -- a sum over the columns --: 1e-5)
@functools.lru_cache(None)
def gspmm_case(op, k):
    row, col = G.graph()
    e = row.numel()
    gen = torch.Generator().manual_seed(40 + k)
    x, ef, w, gr = torch.randn(N, k, generator=gen), torch.randn(e, k, generator=gen), torch.rand(e, generator=gen) + 0.5, \
        torch.randn(N, k, generator=gen)
    rd, cd = _coo_dev()
    run = _autograd(lambda o: ops_mod.src_op_e_aggr_coo(op, "sum", o["x"], o["ef"], rd, cd, data=o["w"]), ("x", "ef", "w"))
    want = oracle.src_op_e_aggr(op, "sum", x, ef, row, col, N, w=w)
    msg_abs = oracle.src_op_e_aggr("mul" if op == "mul" else "add", "sum", x.abs(), ef.abs(), row, col, N, w=w)  # scale of the summands
    xa, ea, wa = (t.clone().requires_grad_() for t in (x, ef, w))
    with G.edge_order():
        msg = ops_mod._BINARY[op](xa[col], ea) * wa.view(-1, 1)
        torch.zeros(N, k).index_add_(0, row, msg).backward(gr)
    dst_short = (torch.bincount(row, minlength=N) <= 128).numpy()
    src_short = (torch.bincount(col, minlength=N) <= 128).numpy()
    gx_abs = torch.zeros(N, k).index_add_(0, col, (gr[row] * w.view(-1, 1) * (ef if op == "mul" else 1.0)).abs()).numpy()
    gw_terms = (gr[row] * ops_mod._BINARY[op](x[col], ef)).double()

    def judge(res):
        _short_exact(res["out"], want, dst_short, np.maximum(msg_abs, 1e-30), "gspmm %s" % op)
        _short_exact(res["g_x"], xa.grad.numpy(), src_short, gx_abs, "grad_x %s" % op)
        assert _bytes(res["g_ef"]) == _bytes(ea.grad), "grad of the edge feature"
        _within(res["g_w"], gw_terms.sum(1).numpy(), gw_terms.abs().sum(1).numpy(), floor=1e-7, what="grad of the edge weight")

    return Case({"x": x, "ef": ef, "w": w, "grad": gr}, run, judge,
                exact={"out": dst_short, "g_x": src_short, "g_ef": None}, control=(k == 7))


# ---- mhspmm forward and backward, which runs mhsddmm (tests/test_ops_gpu.py: fp32 forward and grad_feat the oracle's bytes on
#      short rows, rtol 1e-4 / atol 1e-3 on re-associated long rows, grad_att rtol 1e-5 / atol 1e-5; tests/test_halfprec_rows_gpu.py:
#      16-bit results within half an ulp with the row degree as terms, grad_att within (2 F + 2) 2^-24 of its terms)
HEADS = ((8, 8), (2, 16), (4, 32))


@functools.lru_cache(None)
def mhspmm_case(h, f, dtype):
    g = _csr()
    gen = torch.Generator().manual_seed(100 * h + f)
    att = torch.rand(g.nnz, h, generator=gen)
    feat, gr = torch.randn(N, h, f, generator=gen).to(dtype), torch.randn(N, h, f, generator=gen).to(dtype)
    rp, ci = _csr_dev()
    run = _autograd(lambda o: csrmhspmm(rp, ci, o["feat"], o["att"]), ("feat", "att"))
    a64, f64, g64 = _np64(att), _np64(feat), _np64(gr)
    out, out_abs = _edge_sum(a64[:, :, None] * f64[g.col], g.row, N)
    gf, gf_abs = _edge_sum(a64[:, :, None] * g64[g.row], g.col, N)
    dots = g64[g.row] * f64[g.col]
    short, src_short = g.deg <= g.thresh, g.col_deg <= g.thresh
    if dtype == F32:
        want = oracle.mhspmm(g.rowptr, g.colind, att, feat)
        want_gf = oracle.mhspmm(g.colptr, g.rowind, oracle.mhtranspose(g.perm, att), gr)
        want_ga = oracle.mhsddmm(g.rowptr, g.colind, gr, feat)

    def judge(res):
        if dtype == F32:
            assert res["out"].numpy()[short].tobytes() == want[short].tobytes()
            np.testing.assert_allclose(res["out"].numpy(), want, rtol=1e-4, atol=1e-3)
            assert res["g_feat"].numpy()[src_short].tobytes() == want_gf[src_short].tobytes()
            np.testing.assert_allclose(res["g_feat"].numpy(), want_gf, rtol=1e-4, atol=1e-3)
            np.testing.assert_allclose(res["g_att"].numpy(), want_ga, rtol=1e-5, atol=1e-5)
        else:
            assert res["out"].dtype == dtype and res["g_feat"].dtype == dtype and res["g_att"].dtype == F32
            hp.assert_close(res["out"], out, out_abs, g.deg[:, None, None], dtype, "mhspmm")
            hp.assert_close(res["g_feat"], gf, gf_abs, g.col_deg[:, None, None], dtype, "grad_feat")
            hp.assert_within(res["g_att"].numpy(), dots.sum(-1), (2 * f + 2) * 2.0 ** -24 * np.abs(dots).sum(-1), "grad_att")

    exact = {"out": short, "g_feat": src_short} if dtype == F32 else {}
    return Case({"feat": feat, "att": att, "grad": gr}, run, judge, exact=exact, control=(f == 7))


# ---- csr_sddmm_raw (tests/test_ops_gpu.py::test_sddmm: 1e-5 of the terms + 1e-7)
@functools.lru_cache(None)
def sddmm_case(k):
    g = _csr()
    d1, d2 = _rand(N, k, seed=1), _rand(N, k, seed=2)
    rp, ci = _csr_dev()
    want = oracle.csr_sddmm(g.rowptr, g.colind, d1, d2)
    scale = (d1.abs().numpy()[g.row] * d2.abs().numpy()[g.col]).sum(1)
    return Case({"d1": d1, "d2": d2}, lambda o: {"out": csr_sddmm_raw(rp, ci, o["d1"], o["d2"])},
                lambda res: _within(res["out"], want, scale, floor=1e-7, what="sddmm"), control=(k == 7))


# ---- scatter_max forward, and backward through the CSC gather (tests/test_ops_gpu.py: values and argmax the oracle's bytes at
#      every row length; the gather's gradient its bytes while a source has at most the exact-row bound of out-edges, 1e-5 beyond)
@functools.lru_cache(None)
def scatter_max_case(k):
    g = _csr()
    x, gr = _rand(N, k, seed=k), _rand(N, k, seed=1000 + k)
    x[5] = x[6]  # ties: the first maximum in CSR order wins
    rp, ci = _csr_dev()
    want, want_id = oracle.scatter_max_fwd(g.rowptr, g.colind, x, quirk=False)
    want_g = oracle.scatter_max_bwd(gr, want_id, N)
    scale_g = oracle.scatter_max_bwd(gr.abs(), want_id, N)
    src_short = g.col_deg <= g.thresh

    def extra(o, out):
        return {"argmax": scatter_max_fp(rp, ci, o["x"].detach())[1]}

    def judge(res):
        assert res["out"].numpy().tobytes() == want.tobytes() and np.array_equal(res["argmax"].numpy(), want_id)
        assert res["g_x"].numpy()[src_short].tobytes() == want_g[src_short].tobytes()
        _within(res["g_x"], want_g, scale_g, floor=1e-12, what="scatter_max backward")

    return Case({"x": x, "grad": gr}, _autograd(lambda o: scatter_max(rp, ci, o["x"]), ("x",), extra), judge,
                exact={"out": None, "argmax": None, "g_x": src_short}, control=(k == 7))


# ---- fused GAT forward and backward (fp32, ordinary launch: tests/test_ops_gpu.py::test_hub_rows_mhspmm_mhsddmm_gat, forward rtol
#      2e-5 / atol 2e-6 against the oracle, gradients rtol 5e-4 / atol 5e-5 against float64; fp32 over a forced XCD plan:
#      tests/test_xcd_gpu.py, 2e-5 of the terms; 16-bit, either launch: tests/_gat_halfprec.py, out and grad_feat within
#      0.5 ulp(|want| + s) + s with s = 4e-5 of the terms, the two attention gradients within 4 * 2^-7 of theirs)
@functools.lru_cache(None)
def gat_case(h, f, dtype, pad, mode="off"):
    g = _csr()
    gen = torch.Generator().manual_seed(7 * h + f)
    ar, ac = torch.randn(N, h, generator=gen), torch.randn(N, h, generator=gen)
    feat, gr = torch.randn(N, h, f, generator=gen).to(dtype), torch.randn(N, h, f, generator=gen).to(dtype)
    rp, ci = _csr_dev()
    run = _autograd(lambda o: gat_mod.fused_gat_func(o["attn_row"], o["attn_col"], rp, ci, rp, ci, 0.2, o["feat"]),
                    ("attn_row", "attn_col", "feat"))
    fh, gh = feat.float().numpy(), gr.float().numpy()
    want = oracle.gat_fwd(g.rowptr, g.colind, ar, ac, fh, 0.2)
    want_abs = oracle.gat_fwd(g.rowptr, g.colind, ar, ac, np.abs(fh), 0.2)
    gf, gl, grr, sf, sl, sr = oracle.gat_bwd(g.rowptr, g.colind, ar, ac, fh, 0.2, gh, scales=True)

    def judge(res):
        if dtype != F32:  # tests/_gat_halfprec.py: check, with the S_REL of a graph with hub rows
            assert res["out"].dtype == dtype and res["g_feat"].dtype == dtype
            for name, ref, scale in (("out", want, want_abs), ("g_feat", gf, sf)):
                slack = GH.S_REL["hubs"] * np.asarray(scale, dtype=np.float64)
                hp.assert_within(_np64(res[name]), ref, 0.5 * hp.ulp(np.abs(ref) + slack, dtype) + slack, name)
            for name, ref, scale in (("g_attn_row", gl, sl), ("g_attn_col", grr, sr)):
                hp.assert_within(_np64(res[name]), ref, 4 * GH.ATTN_TOL[dtype] * np.asarray(scale, dtype=np.float64) + 1e-30, name)
        elif mode == "force":  # tests/test_xcd_gpu.py: _close with TOL[float32]
            for name, ref, scale in (("out", want, want_abs), ("g_feat", gf, sf), ("g_attn_row", gl, sl), ("g_attn_col", grr, sr)):
                _within(_np64(res[name]), ref, scale, rel=XCD_TOL[F32], floor=1e-30, what=name)
        else:
            np.testing.assert_allclose(res["out"].numpy(), want, rtol=2e-5, atol=2e-6)
            for got, ref, name in ((res["g_attn_row"], gl, "attn_row"), (res["g_attn_col"], grr, "attn_col"), (res["g_feat"], gf, "feat")):
                np.testing.assert_allclose(got.numpy(), ref, rtol=5e-4, atol=5e-5, err_msg=name)

    on_plan = []

    def setup(monkeypatch):
        monkeypatch.setattr(gat_mod, "PAD_FEATURES", pad)
        monkeypatch.setattr(xcdplan, "MODE", mode)
        xcdplan.XPLANS.clear()
        del on_plan[:]
        lib = _lib.hip()
        real = _REAL_GAT_XCD

        def fwd_xcd(*a):
            rc = real(*a)
            on_plan.append(rc)
            return rc

        monkeypatch.setattr(lib, "cogdl_hip_gat_fwd_xcd", fwd_xcd)

    def verify(shift):
        if mode == "force" and shift is None:
            assert on_plan == [0], "the aligned call did not run the plan's forward kernels"
        if mode == "off":
            assert not on_plan

    return Case({"attn_row": ar, "attn_col": ac, "feat": feat, "grad": gr}, run, judge, setup=setup, cleanup=xcdplan.XPLANS.clear,
                verify=verify, control=(f == 7 and not pad))


# ---- the head projection of cogdl_amd/fused.py (its forward arithmetic is the layer's (a * h).sum(-1): float64 of the rounded
#      inputs, within the fp32 summation of F products -- the bound of _halfprec.slack --; grad_feat one fp32 expression rounded once)
@functools.lru_cache(None)
def head_proj_case(h, f, dtype):
    gen = torch.Generator().manual_seed(3 * h + f)
    a_l, a_r = torch.randn(1, h, f, generator=gen), torch.randn(1, h, f, generator=gen)
    feat = torch.randn(N, h, f, generator=gen).to(dtype)
    g_l, g_r = torch.randn(N, h, generator=gen), torch.randn(N, h, generator=gen)
    f64 = _np64(feat)

    def run(o):
        for n in ("a_l", "a_r", "feat"):
            o[n].requires_grad_()
        h_l, h_r = fused._HeadProjections.apply(o["a_l"], o["a_r"], o["feat"])
        torch.autograd.backward([h_l, h_r], [o["grad_l"], o["grad_r"]])
        return {"h_l": h_l, "h_r": h_r, "g_feat": o["feat"].grad, "g_a_l": o["a_l"].grad, "g_a_r": o["a_r"].grad}

    def judge(res):
        for name, a in (("h_l", a_l), ("h_r", a_r)):
            terms = _np64(a) * f64
            hp.assert_within(res[name].numpy(), terms.sum(-1), hp.slack(np.abs(terms).sum(-1), f), name)
        gfeat = _np64(g_l)[:, :, None] * _np64(a_l) + _np64(g_r)[:, :, None] * _np64(a_r)
        gabs = np.abs(_np64(g_l))[:, :, None] * np.abs(_np64(a_l)) + np.abs(_np64(g_r))[:, :, None] * np.abs(_np64(a_r))
        if dtype == F32:
            hp.assert_within(res["g_feat"].numpy(), gfeat, hp.slack(gabs, 2), "grad_feat")
        else:
            hp.assert_close(res["g_feat"], gfeat, gabs, 2, dtype, "grad_feat")
        for name, gg in (("g_a_l", g_l), ("g_a_r", g_r)):
            terms = _np64(gg)[:, :, None] * f64
            hp.assert_within(res[name].numpy(), terms.sum(0)[None], hp.slack(np.abs(terms).sum(0)[None], N), name)

    return Case({"a_l": a_l, "a_r": a_r, "feat": feat, "grad_l": g_l, "grad_r": g_r}, run, judge, control=(f == 7))


# ---- edge_softmax: the wrapper clones an offset operand (tests/test_ops_gpu.py: forward rtol 1e-5 / atol 1e-9, backward 1e-5 of
#      the terms; 16-bit: tests/test_halfprec_softmax_gpu.py's terms)
@functools.lru_cache(None)
def softmax_case(h, dtype):
    g = _csr()
    v, gr = (_rand(g.nnz, h, seed=3) * 3.0).to(dtype), _rand(g.nnz, h, seed=4).to(dtype)
    rp = _csr_dev()[0]
    want, spread = hp.row_softmax(g.rowptr.numpy(), _np64(v))
    fwd_terms, bwd_terms = hp.softmax_terms(g.rowptr.numpy(), spread)

    def judge(res):
        assert res["out"].dtype == dtype and res["g_v"].dtype == dtype and res["g_v"].shape == v.shape
        _, _, want_g, scale_g = hp.row_softmax(g.rowptr.numpy(), None, _np64(gr), _np64(res["out"]))
        if dtype == F32:
            np.testing.assert_allclose(res["out"].numpy(), want, rtol=1e-5, atol=1e-9)
            _within(res["g_v"], want_g, scale_g, floor=1e-12, what="edge_softmax backward")
        else:
            hp.assert_close(res["out"], want, want, fwd_terms, dtype, "edge_softmax")
            hp.assert_close(res["g_v"], want_g, scale_g, bwd_terms, dtype, "edge_softmax backward")

    return Case({"v": v, "grad": gr}, _autograd(lambda o: csr_edge_softmax(rp, o["v"]), ("v",)), judge, exact=("out", "g_v"))


# ---- segment_pool and sort_pool (tests/test_readout_gpu.py: the host twin's bytes, forward and backward)
READOUT_LENGTHS = [0, 1, 63, 64, 65]


@functools.lru_cache(None)
def pool_case(mode, f):
    ptr = RC.ptr_of(READOUT_LENGTHS)
    x = _rand(sum(READOUT_LENGTHS), f, seed=f) * 100
    gr = _rand(len(READOUT_LENGTHS), f, seed=1)
    ptr_d = ptr.to(DEV)
    xc = x.clone().requires_grad_()
    want = readout_mod.segment_pool(xc, ptr, mode)
    want.backward(gr)

    def judge(res):
        assert _bytes(res["out"]) == _bytes(want) and _bytes(res["g_x"]) == _bytes(xc.grad)

    return Case({"x": x, "grad": gr}, _autograd(lambda o: readout_mod.segment_pool(o["x"], ptr_d, mode), ("x",)), judge,
                exact=("out", "g_x"), control=(f == 7))


@functools.lru_cache(None)
def sort_pool_case(f):
    ptr = RC.ptr_of(READOUT_LENGTHS)
    k = 30
    x = _rand(sum(READOUT_LENGTHS), f, seed=f) * 100
    x[:, 0] = torch.randint(0, 9, (x.shape[0],), generator=torch.Generator().manual_seed(2)).float()  # a key column full of ties
    gr = _rand(len(READOUT_LENGTHS), k, f, seed=4)
    ptr_d = ptr.to(DEV)
    xc = x.clone().requires_grad_()
    want, want_idx = readout_mod.sort_pool(xc, ptr, k, 0)
    want.backward(gr)
    idx = {}

    def fn(o):
        out, idx["idx"] = readout_mod.sort_pool(o["x"], ptr_d, k, 0)
        return out

    def judge(res):
        assert _bytes(res["out"]) == _bytes(want) and _bytes(res["idx"]) == _bytes(want_idx) and _bytes(res["g_x"]) == _bytes(xc.grad)

    return Case({"x": x, "grad": gr}, _autograd(fn, ("x",), lambda o, out: {"idx": idx["idx"]}), judge, exact=("out", "idx", "g_x"))


# ---- rel_gspmm: the rel table, the weights and the upstream gradient (tests/test_relational_gpu.py covers x; _gen_cases.check)
@functools.lru_cache(None)
def rel_case(op, k):
    row, col = G.graph()
    e, n_rel = row.numel(), 7
    gen = torch.Generator().manual_seed(60 + k)
    x, rel, w, gr = torch.randn(N, k, generator=gen), torch.randn(n_rel, k, generator=gen), torch.rand(e, generator=gen) + 0.5, \
        torch.randn(N, k, generator=gen)
    etype = torch.randint(0, n_rel, (e,), generator=gen)
    rd, cd = _coo_dev()
    td = etype.to(DEV)
    run = _autograd(lambda o: rel_mod.rel_gspmm(o["x"], o["rel"], rd, cd, td, o["w"], op, num_nodes=N), ("x", "rel"))

    def composition(dt):
        xa, ra = x.detach().clone().to(dt).requires_grad_(), rel.detach().clone().to(dt).requires_grad_()
        msg = ops_mod._BINARY[op](xa[col], ra[etype]) * w.to(dt).unsqueeze(-1)
        out = torch.zeros(N, k, dtype=dt).index_add_(0, row, msg)
        out.backward(gr.to(dt))
        return {"out": out.detach(), "g_x": xa.grad, "g_rel": ra.grad}

    with G.edge_order():
        oracle64, ref32 = composition(torch.float64), composition(F32)
    dst_short = (torch.bincount(row, minlength=N) <= 128).numpy()
    src_short = (torch.bincount(col, minlength=N) <= 128).numpy()

    def judge(res):
        G.check("rel_gspmm %s F=%d" % (op, k), res, oracle64, ref32)
        assert _bytes(res["out"][dst_short]) == _bytes(ref32["out"][dst_short])  # (test_relational_gpu.py: short rows, the same bytes)
        assert _bytes(res["g_x"][src_short]) == _bytes(ref32["g_x"][src_short])

    return Case({"rel": rel, "w": w, "grad": gr, "x": x}, run, judge, exact={"out": dst_short, "g_x": src_short}, control=(k == 7))


# ---- gen_aggregate and disen_route: the upstream gradient only, the tables are covered (their own cases, _gen_cases.check)
@functools.lru_cache(None)
def gen_case(aggr, k):
    x, eterm, gr = G.inputs(k, True)
    ref = G.reference(k, True, aggr, 0.75 if aggr == "softmax" else None, False)
    rd, cd = _coo_dev()
    beta = 0.75 if aggr == "softmax" else None
    run = _autograd(lambda o: genaggr_mod.gen_aggregate(o["x"], rd, cd, o["eterm"], aggr, beta, G.EPS, num_nodes=N), ("x", "eterm"))

    def judge(res):
        G.check("gen_aggregate %s F=%d" % (aggr, k), res, *ref)

    return Case({"x": x, "eterm": eterm, "grad": gr}, run, judge, control=(k == 7))


@functools.lru_cache(None)
def disen_case(K, d, tau):
    c, z, gr = DC.inputs(K, d)
    ref = DC.reference(K, d, tau)
    rd, cd = _coo_dev()
    run = _autograd(lambda o: disen_mod.disen_route(o["c"], o["z"], rd, cd, K, tau), ("c", "z"))
    return Case({"c": c, "z": z, "grad": gr}, run, lambda res: G.check("disen_route K=%d d=%d" % (K, d), res, *ref))


# ---- filter_step (tests/test_prone_gpu.py: the host twin's bytes wherever a row has at most the long-row threshold of edges; the
#      longer rows within the bound of the float64 oracle)
@functools.lru_cache(None)
def filter_case(k, alias=False):
    rowptr, colind = PC.ragged()
    ops = PC.step_operands(rowptr, colind, k, seed=9)
    t = dict((n, torch.from_numpy(ops[n].copy())) for n in ("x", "z1", "z2", "acc", "val", "dst_scale"))
    rp, ci = torch.from_numpy(rowptr.copy()), torch.from_numpy(colind.copy())
    kw = dict(a=ops["a"], b=ops["b"], c1=ops["c1"], c2=ops["c2"], d=ops["d"])
    acc_cpu = t["acc"].clone()
    want = filter_step(rp, ci, t["val"], t["x"], z1=t["z1"], z2=t["z2"], dst_scale=t["dst_scale"], acc=acc_cpu, **kw)
    out64, acc64 = PC.step_literal(rowptr, colind, ops["val"], ops["x"], ops["a"], ops["b"], ops["z1"], ops["c1"], ops["z2"],
                                   ops["c2"], ops["dst_scale"], ops["acc"], ops["d"], dtype=np.float64)
    short = np.diff(rowptr) <= PC.LONG
    assert (~short).sum() >= 1
    rp_d, ci_d = rp.to(DEV), ci.to(DEV)
    operands = dict((n, t[n]) for n in ("x", "z1", "z2", "acc"))
    if not alias:
        operands["out"] = torch.zeros_like(t["x"])
    val_d, ds_d = t["val"].to(DEV), t["dst_scale"].to(DEV)

    def run(o):
        dst = o["z1"] if alias else o["out"]
        out = filter_step(rp_d, ci_d, val_d, o["x"], z1=o["z1"], z2=o["z2"], dst_scale=ds_d, acc=o["acc"], out=dst, **kw)
        assert out is dst
        return {"out": dst, "acc": o["acc"]}

    def judge(res):
        assert _bytes(res["out"][short]) == _bytes(want[short]) and _bytes(res["acc"][short]) == _bytes(acc_cpu[short])
        # long rows: what the sequential float32 loop loses against float64, four times over, plus eight roundings
        for got, w32, w64 in ((res["out"], want, out64), (res["acc"], acc_cpu, acc64)):
            lost = np.abs(w32.numpy()[~short].astype(np.float64) - w64[~short]).max()
            err = np.abs(got.numpy()[~short].astype(np.float64) - w64[~short]).max()
            assert err <= 4 * lost + 8 * PC.EPS * np.abs(w64[~short]).max()

    written = ("z1", "acc") if alias else ("out", "acc")
    return Case(operands, run, judge, exact={"out": short, "acc": short}, written=written, control=(k == 7))


# ---- tall_skinny_matmul and linear_wgrad (tests/test_linear_gpu.py: fp32 1e-5 of (the terms + 1); bf16 one ulp of the result +
#      2e-6 of the terms + 1e-7 against float64 on the rounded operands; the weight gradient 1e-5 of the terms + 1e-6).  An x off
#      its 16-byte lanes takes torch's product, as the callers in cogdl_amd/linear.py do when the wrapper answers None.
LIN_ROWS, LIN_K, LIN_N = 4099, 64, 16


@functools.lru_cache(None)
def linear_case(dtype):
    x = _rand(LIN_ROWS, LIN_K, seed=1, dtype=dtype)
    w, b = _rand(LIN_N, LIN_K, seed=2), _rand(LIN_N, seed=3)
    if dtype != F32:
        b = b.to(dtype).float()  # (LinearBf16Function hands the kernel the bias rounded like autocast's cast)
    x64, w64 = _np64(x), _np64(w if dtype == F32 else w.to(dtype))
    want = x64 @ w64.T + _np64(b)
    scale = np.abs(x64) @ np.abs(w64.T) + np.abs(_np64(b))

    def run(o):
        x_dev = o["x"].contiguous()  # (what the wrapper hands the kernel: a strided x is copied, an offset one is not)
        if dtype == F32:
            out = linear.tall_skinny_matmul(x_dev, o["w"], o["bias"], True)
        else:
            out = linear.tall_skinny_matmul_16(x_dev, o["w"], o["bias"], True, dtype)
        # the kernel serves every call whose x is on its 16-byte lanes, whatever the offset of w and bias (tests/test_linear_gpu.py
        # asserts the same of the aligned call), and declines -- None, never an error -- every other
        assert (out is not None) == (x_dev.data_ptr() % 16 == 0), "x %d bytes past a 16-byte boundary" % (x_dev.data_ptr() % 16)
        if out is None and dtype == F32:
            out = torch.nn.functional.linear(o["x"], o["w"], o["bias"])
        elif out is None:
            out = torch.nn.functional.linear(o["x"], o["w"].to(dtype), o["bias"].to(dtype))
        return {"out": out}

    def judge(res):
        if dtype == F32:
            _within(res["out"], want, scale + 1.0, floor=0.0, what="linear forward")
        else:
            assert res["out"].dtype == dtype
            err = np.abs(_np64(res["out"]) - want)
            assert np.all(err <= np.abs(want) * 2.0 ** -8 + 2e-6 * scale + 1e-7), "linear forward (bf16)"

    return Case({"x": x, "w": w, "bias": b}, run, judge)


@functools.lru_cache(None)
def wgrad_case():
    x, gr = _rand(LIN_ROWS, LIN_K, seed=1), _rand(LIN_ROWS, LIN_N, seed=5)
    x64, g64 = _np64(x), _np64(gr)

    def run(o):
        gw, gb = linear.linear_wgrad(o["x"], o["grad"], want_bias=True)
        return {"g_w": gw, "g_b": gb}

    def judge(res):
        _within(res["g_w"], g64.T @ x64, np.abs(g64.T) @ np.abs(x64), floor=1e-6, what="grad_weight")
        _within(res["g_b"], g64.sum(0), np.abs(g64).sum(0), floor=1e-6, what="grad_bias")

    return Case({"x": x, "grad": gr}, run, judge)


# ---- gather_rows_by_id (tests/test_pipeline_gpu.py: the selected rows, bit for bit)
@functools.lru_cache(None)
def gather_case(f, dtype):
    src = _rand(500, f, seed=f, dtype=dtype)
    ids = torch.randint(0, 500, (300,), generator=torch.Generator().manual_seed(1))
    ids_d = ids.to(DEV)
    want = src[ids]

    def run(o):
        res = pipeline.gather_rows_by_id(o["src"], ids_d, out=o["out"])
        pipeline.check_gather(res)
        assert res is o["out"]
        return {"out": o["out"]}

    def judge(res):
        assert _bytes(res["out"]) == _bytes(want), "gather_rows_by_id: not the selected rows"

    return Case({"src": src, "out": torch.zeros(300, f, dtype=dtype)}, run, judge, exact=("out",), written=("out",), control=(f == 7))


# -------------------------------------------------------------------------------------------------------------- the table
class Row:
    def __init__(self, name, factory, operands, half=(), only=None):
        """operands: the dense floating-point operands of the case; half: those that are 16-bit; only: offsets to keep
        (gather_rows_by_id's closed exception: 16-bit rows need 4-byte alignment)."""
        self.name, self.factory, self.operands, self.half, self.only = name, factory, tuple(operands), tuple(half), only


ROWS = []
for _k in WIDTHS:
    ROWS.append(Row("csrspmm-weighted-F%d" % _k, functools.partial(spmm_case, _k, True), ("x", "w", "grad")))
    ROWS.append(Row("csrspmm-unweighted-F%d" % _k, functools.partial(spmm_case, _k, False), ("x", "grad")))
    ROWS.append(Row("csr_spmm_raw-out-F%d" % _k, functools.partial(acc_case, _k), ("x", "w", "out")))
    ROWS.append(Row("epilogue-F%d" % _k, functools.partial(epilogue_case, _k), ("x", "w", "out_norm", "in_norm", "bias", "grad")))
    ROWS.append(Row("csrspmm-int64-F%d" % _k, functools.partial(big_case, _k), ("x", "w", "grad")))
    ROWS.append(Row("csr_sddmm-F%d" % _k, functools.partial(sddmm_case, _k), ("d1", "d2")))
    ROWS.append(Row("scatter_max-F%d" % _k, functools.partial(scatter_max_case, _k), ("x", "grad")))
    ROWS.append(Row("filter_step-F%d" % _k, functools.partial(filter_case, _k), ("x", "z1", "z2", "acc", "out")))
    ROWS.append(Row("filter_step-out-is-z1-F%d" % _k, functools.partial(filter_case, _k, True), ("z1",)))
    ROWS.append(Row("gather_rows-f32-F%d" % _k, functools.partial(gather_case, _k, F32), ("src", "out")))
    for _op in ("mul", "add", "sub"):
        ROWS.append(Row("gspmm-%s-F%d" % (_op, _k), functools.partial(gspmm_case, _op, _k), ("x", "ef", "w", "grad")))
    ROWS.append(Row("rel_gspmm-sub-F%d" % _k, functools.partial(rel_case, "sub", _k), ("rel", "w", "grad")))
for _k in (64, 7):
    ROWS.append(Row("rel_gspmm-mul-F%d" % _k, functools.partial(rel_case, "mul", _k), ("rel", "w", "grad")))
    for _aggr in ("softmax", "sum"):
        ROWS.append(Row("gen_aggregate-%s-F%d" % (_aggr, _k), functools.partial(gen_case, _aggr, _k), ("grad",)))
for _K, _d, _tau in ((16, 4, 1.0), (8, 8, 0.5)):
    ROWS.append(Row("disen_route-K%d-d%d" % (_K, _d), functools.partial(disen_case, _K, _d, _tau), ("grad",)))
for _k in (8, 64, 7):
    ROWS.append(Row("csrspmm-force-f32-F%d" % _k, functools.partial(xcd_case, _k, F32), ("x", "w", "grad")))
    for _dt, _nm in ((BF16, "bf16"), (F16, "f16")):
        ROWS.append(Row("csrspmm-force-%s-F%d" % (_nm, _k), functools.partial(xcd_case, _k, _dt), ("x", "w", "grad"),
                        half=("x", "w", "grad")))
ROWS.append(Row("csrspmm-sweeps-F128", sweep_case, ("x", "w", "grad")))
for _h, _f in HEADS:
    ROWS.append(Row("mhspmm-f32-H%dxF%d" % (_h, _f), functools.partial(mhspmm_case, _h, _f, F32), ("feat", "att", "grad")))
    ROWS.append(Row("mhspmm-bf16-H%dxF%d" % (_h, _f), functools.partial(mhspmm_case, _h, _f, BF16), ("feat", "att", "grad"),
                    half=("feat", "grad")))
    for _pad in (True, False):
        _p = "pad" if _pad else "raw"
        ROWS.append(Row("gat-f32-%s-H%dxF%d" % (_p, _h, _f), functools.partial(gat_case, _h, _f, F32, _pad),
                        ("attn_row", "attn_col", "feat", "grad")))
        ROWS.append(Row("gat-bf16-%s-H%dxF%d" % (_p, _h, _f), functools.partial(gat_case, _h, _f, BF16, _pad),
                        ("attn_row", "attn_col", "feat", "grad"), half=("feat", "grad")))
    ROWS.append(Row("head_proj-f32-H%dxF%d" % (_h, _f), functools.partial(head_proj_case, _h, _f, F32),
                    ("a_l", "a_r", "feat", "grad_l", "grad_r")))
    ROWS.append(Row("head_proj-bf16-H%dxF%d" % (_h, _f), functools.partial(head_proj_case, _h, _f, BF16),
                    ("a_l", "a_r", "feat", "grad_l", "grad_r"), half=("feat",)))
# fused GAT over a forced XCD plan: the plan entries' workspace queries and kernels with an offset feat / upstream gradient
for _dt, _nm, _half in ((F32, "f32", ()), (BF16, "bf16", ("feat", "grad"))):
    ROWS.append(Row("gat-force-%s-H8xF8" % _nm, functools.partial(gat_case, 8, 8, _dt, True, "force"),
                    ("attn_row", "attn_col", "feat", "grad"), half=_half))
# the control of the head operators: one head of 7 columns at the caller's own width is vector width 1 at every alignment
ROWS.append(Row("mhspmm-f32-H1xF7", functools.partial(mhspmm_case, 1, 7, F32), ("feat", "att", "grad")))
ROWS.append(Row("gat-f32-raw-H1xF7", functools.partial(gat_case, 1, 7, F32, False), ("attn_row", "attn_col", "feat", "grad")))
ROWS.append(Row("head_proj-f32-H1xF7", functools.partial(head_proj_case, 1, 7, F32), ("a_l", "a_r", "feat", "grad_l", "grad_r")))
for _h in (8, 3):
    ROWS.append(Row("edge_softmax-f32-H%d" % _h, functools.partial(softmax_case, _h, F32), ("v", "grad")))
    ROWS.append(Row("edge_softmax-bf16-H%d" % _h, functools.partial(softmax_case, _h, BF16), ("v", "grad"), half=("v", "grad")))
for _f in (8, 64, 7):
    for _mode in ("sum", "mean", "max"):
        ROWS.append(Row("segment_pool-%s-F%d" % (_mode, _f), functools.partial(pool_case, _mode, _f), ("x", "grad")))
    ROWS.append(Row("sort_pool-F%d" % _f, functools.partial(sort_pool_case, _f), ("x", "grad")))
ROWS.append(Row("tall_skinny_matmul-f32", functools.partial(linear_case, F32), ("x", "w", "bias")))
ROWS.append(Row("tall_skinny_matmul-bf16", functools.partial(linear_case, BF16), ("x", "w", "bias"), half=("x",)))
ROWS.append(Row("linear_wgrad", wgrad_case, ("x", "grad")))
for _f in (8, 6, 64):
    ROWS.append(Row("gather_rows-bf16-F%d" % _f, functools.partial(gather_case, _f, BF16), ("src", "out"), half=("src", "out"),
                    only=(2, 4)))


def _offset_params():
    params = []
    for row in ROWS:
        for name in row.operands:
            for off in OFFSETS[2 if name in row.half else 4]:
                if row.only is None or off in row.only:
                    params.append(pytest.param(row, {name: off}, id="%s-%s+%d" % (row.name, name, off)))
        every = 1 if row.only is None else row.only[0]
        if len(row.operands) > 1:
            params.append(pytest.param(row, dict((name, every) for name in row.operands), id="%s-all+%d" % (row.name, every)))
    return params


@pytest.mark.parametrize("row,shift", _offset_params())
def test_operand_at_an_offset(row, shift, monkeypatch):
    case = row.factory()
    assert set(row.operands) <= set(case.operands), "the table names an operand the case does not have"
    aligned = case.aligned(monkeypatch)
    ops, guards = case.device_operands(shift)
    for name, view in ops.items():
        if name in shift:
            assert view.data_ptr() % 16 == (shift[name] * view.element_size()) % 16
    res = case.call(ops, monkeypatch, shift)                           # (a)
    assert all(O.guards_intact(g) for g in guards.values()), "a write outside a shifted operand"   # (d)
    assert set(case.written) <= set(case.operands)
    case.judge(res)                                                    # (b)
    assert res.keys() == aligned.keys()
    for name in sorted(res):                                           # (c)
        if case.control or name in case.exact:
            rows = None if case.control else case.exact[name]
            a, b = (res[name], aligned[name]) if rows is None else (res[name][rows], aligned[name][rows])
            assert _bytes(a) == _bytes(b), "%s: not the aligned call's bytes" % name
        if not case.control:
            same = _bytes(res[name]) == _bytes(aligned[name])
            print("%s %s %s: %s the aligned call's bytes" % (row.name, shift, name, "is" if same else "is NOT"))


# ------------------------------------------------------------------------------------------- non-contiguous operands
STRIDED = [r for r in ROWS if r.name in (
    "csrspmm-weighted-F64", "csr_spmm_raw-out-F64", "epilogue-F64", "csrspmm-int64-F64", "csr_sddmm-F64", "scatter_max-F64",
    "gspmm-mul-F64", "rel_gspmm-sub-F64", "gen_aggregate-softmax-F64", "disen_route-K16-d4", "mhspmm-f32-H8xF8", "mhspmm-bf16-H8xF8",
    "gat-f32-pad-H8xF8", "gat-bf16-raw-H8xF8", "head_proj-f32-H8xF8", "edge_softmax-f32-H8", "segment_pool-max-F64", "sort_pool-F64",
    "tall_skinny_matmul-f32", "tall_skinny_matmul-bf16", "linear_wgrad", "csrspmm-force-bf16-F64")]
REFUSES = [r for r in ROWS if r.name in ("filter_step-F64", "gather_rows-f32-F64", "csr_spmm_raw-out-F64")]


@pytest.mark.parametrize("row", STRIDED, ids=[r.name for r in STRIDED])
def test_non_contiguous_operands_are_copied(row, monkeypatch):
    """Every dense operand (the upstream gradient included) as a column slice of a wider tensor: the wrappers call
    .contiguous(), so the results are the bytes of the call on fresh contiguous copies.  (A written operand has to be
    contiguous: it is left as it is here and refused below.)"""
    case = row.factory()
    aligned = case.aligned(monkeypatch)
    ops = dict((n, t.to(DEV).clone() if n in case.written else O.strided(t.to(DEV))) for n, t in case.operands.items())
    res = case.call(ops, monkeypatch)
    assert res.keys() == aligned.keys()
    for name in res:
        assert _bytes(res[name]) == _bytes(aligned[name]), name


def _upstream(row):
    return [n for n in row.operands if n.startswith("grad")]


DIFFERENTIABLE = [r for r in ROWS if _upstream(r)]  # every differentiable row: sweeps, controls and the head projection included


@pytest.mark.parametrize("row", DIFFERENTIABLE, ids=[r.name for r in DIFFERENTIABLE])
def test_expanded_upstream_gradient(row, monkeypatch):
    """out.sum().backward() -- for the head projection (h_l.sum() + h_r.sum()).backward() --: every upstream gradient is a
    stride-0 expansion of one scalar.  The gradients are the bytes of the call that gets dense tensors of ones."""
    case = row.factory()
    ones = dict(case.operands)
    for n in _upstream(row):
        ones[n] = torch.ones_like(case.operands[n])
    results = []
    for expand in (False, True):
        ops = dict((n, t.to(DEV).clone()) for n, t in ones.items())
        if expand:
            for n in _upstream(row):
                ops[n] = torch.ones((), dtype=ones[n].dtype, device=DEV).expand(ones[n].shape)
                assert not ops[n].is_contiguous() and set(ops[n].stride()) == {0}
        results.append(case.call(ops, monkeypatch))
    want, got = results
    assert got.keys() == want.keys()
    for name in got:
        assert _bytes(got[name]) == _bytes(want[name]), name


@pytest.mark.parametrize("row", REFUSES, ids=[r.name for r in REFUSES])
def test_non_contiguous_operands_are_refused_by_name(row, monkeypatch):
    case = row.factory()
    if case.setup is not None:
        case.setup(monkeypatch)
    names = case.written if row.name.startswith("csr_spmm_raw") else row.operands
    for name in names:
        ops = dict((n, O.strided(t.to(DEV)) if n == name else t.to(DEV).clone()) for n, t in case.operands.items())
        with pytest.raises(_lib.BackendError, match="contiguous"):
            case.run(ops)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- refusals, by name
def test_gather_rows_names_the_operand_that_is_not_four_byte_aligned():
    """The one closed exception of the contract: 16-bit rows at an odd element offset."""
    src = _rand(100, 8, seed=1, dtype=BF16)
    ids = torch.arange(50, device=DEV)
    odd_src = O.shifted(src, 1, device=DEV)[0]
    with pytest.raises(_lib.BackendError, match="src must be 4-byte aligned"):
        pipeline.gather_rows_by_id(odd_src, ids)
    odd_out, guard = O.shifted(torch.zeros(50, 8, dtype=BF16), 1, device=DEV)
    with pytest.raises(_lib.BackendError, match="out must be 4-byte aligned"):
        pipeline.gather_rows_by_id(src.to(DEV), ids, out=odd_out)
    torch.cuda.synchronize()
    assert O.guards_intact(guard) and not odd_out.any()


def test_raw_plan_and_sweep_entries_name_the_operand():
    """The raw entries over a plan or a sweep layout refuse an operand off their lanes by name, before any launch (the forward
    speculation enqueues neither of its two guarded launches); the policy never sends one there (test_operand_offsets_cpu.py)."""
    g = _csr()
    rp, ci = _csr_dev()
    xplan = xcdplan.build(rp, ci)
    x, guard_x = O.shifted(_rand(N, 64, seed=1), 1, device=DEV)
    with pytest.raises(_lib.BackendError, match="csr_spmm_xcd: x starts 4 bytes past a multiple of 16"):
        spmm_mod.csr_spmm_xcd_raw(xplan, g.val.to(DEV), x)
    out, guard = O.shifted(torch.zeros(N, 64), 2, device=DEV)
    with pytest.raises(_lib.BackendError, match="csr_spmm_xcd: out starts 8 bytes past a multiple of 16"):
        spmm_mod.csr_spmm_xcd_raw(xplan, g.val.to(DEV), x.clone(), out=out)
    sg = synth.scaled(300, 8, seed=4).to(DEV)
    sp = sweepplan.build_forward(sg.rowptr, sg.colind, sg.n_cols, int(_lib.hip().cogdl_hip_csr_spmm_sweep_group_rows()))
    fp = plan.Fingerprint(sg.rowptr, sg.colind, sg.n_cols, dev_parts=True)
    sp.hash = fp.key()[4] & ((1 << 64) - 1)
    x128 = O.shifted(_rand(300, 128, seed=2), 1, device=DEV)[0]
    with pytest.raises(_lib.BackendError, match="csr_spmm_sweep_forward: x starts 4 bytes past a multiple of 8"):
        spmm_mod.csr_spmm_sweep_forward_raw(sp, fp.dev, sg.rowptr, sg.colind, sg.weight, x128)
    csc = plan.csr2csc(sg.rowptr, sg.colind, sg.n_cols)
    with pytest.raises(_lib.BackendError, match="csr_spmm_sweep: x starts 4 bytes"):
        spmm_mod.csr_spmm_sweep_raw(csc, sg.weight, x128)
    torch.cuda.synchronize()
    assert O.guards_intact(guard) and O.guards_intact(guard_x) and not out.any()
