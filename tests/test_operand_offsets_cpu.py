"""Operands that start mid-allocation, without a GPU (the contract paragraph of INTEGRATION.md; tests/_offset.py):
  * the helper itself: the view's address modulo 16, the sentinel pads and what guards_intact sees of a write past either end,
    strided views, and the control property (a call that cannot see the address returns the same bytes at every offset);
  * filter_step on CPU tensors through the host twin (cogdl_host_csr_filter_step): each of x, z1, z2, acc, out alone at an offset
    of 1 and 2 floats, all of them together, and out is z1 with both shifted -- the bytes of the literal float32 loop
    (_prone_cases.step_literal) and of the aligned call, guards intact; a strided operand is refused by name;
  * the address decisions of cogdl_amd/xcdplan.py, asked with CPU tensors whose data_ptr() the test controls: spmm_split answers
    None for an x off its 16-byte lanes, in "force" mode too; spmm_backward_sweep and spmm_forward_sweep answer no for an
    operand off the sweep's 8-byte lanes and yes for the same values 8 or 16 bytes in.  None of them loads the GPU library."""
import types

import numpy as np
import pytest
import torch

import _offset as O
import _prone_cases as cases
from cogdl_amd import _lib, plan, sweepplan, xcdplan
from cogdl_amd.operators.spectral import filter_step

OFFSETS32 = (1, 2)        # float32: 4- and 8-byte boundaries
OFFSETS16 = (1, 2, 4)     # 16-bit: 2, 4 and 8 bytes


# ------------------------------------------------------------------------------------------------------------- the helper
@pytest.mark.parametrize("dtype,offsets", [(torch.float32, OFFSETS32 + (0, 3, 4)), (torch.bfloat16, OFFSETS16 + (0, 3, 8)),
                                           (torch.float16, OFFSETS16), (torch.float64, (0, 1))])
def test_shifted_places_the_view_and_fills_the_pads(dtype, offsets):
    t = torch.arange(3 * 7, dtype=torch.float32).view(3, 7).to(dtype)
    for elems in offsets:
        view, guard = O.shifted(t, elems)
        assert view.is_contiguous() and view.shape == t.shape and view.dtype == dtype and torch.equal(view, t)
        assert view.data_ptr() % 16 == (elems * t.element_size()) % 16
        assert view.data_ptr() != t.data_ptr() and view.untyped_storage().data_ptr() == guard.store.untyped_storage().data_ptr()
        assert guard.lo >= 8 and guard.store.numel() - guard.hi >= 8
        assert bool((guard.store[:guard.lo] == torch.tensor(O.SENTINEL).to(dtype)).all())
        assert bool((guard.store[guard.hi:] == torch.tensor(O.SENTINEL).to(dtype)).all())
        assert O.guards_intact(guard)
        view.fill_(1.0)  # the operand's own contents are not guarded
        assert O.guards_intact(guard)


def test_guards_see_one_element_written_past_either_end():
    t = torch.zeros(5, 6)
    for where in ("before", "behind", "sign of the sentinel"):
        view, guard = O.shifted(t, 1)
        flat = guard.store
        if where == "before":
            flat[guard.lo - 1] = 0.0
        elif where == "behind":
            flat[guard.hi] = 0.0
        else:  # bit for bit: a value that compares equal under == after a round trip is still a write
            flat[guard.hi + 3] = float(np.nextafter(np.float32(O.SENTINEL), np.float32(0)))
        assert not O.guards_intact(guard), where
    nan_view, nan_guard = O.shifted(t, 2)
    nan_guard.store[nan_guard.lo - 2] = float("nan")
    assert not O.guards_intact(nan_guard)


def test_strided_is_a_column_slice_with_the_same_values():
    for t in (torch.randn(9, 5), torch.randn(11), torch.randn(4, 3, 2).bfloat16()):
        s = O.strided(t)
        assert not s.is_contiguous() and s.shape == t.shape and torch.equal(s, t)
        assert torch.equal(s.contiguous(), t) and s.contiguous().is_contiguous()


def test_control_a_call_that_cannot_see_the_address_gives_the_same_bytes():
    """The harness's own control: torch's elementwise kernels on the CPU do not choose by address."""
    t = torch.randn(13, 7)
    want = (t * 3.0 + 1.0).numpy().tobytes()
    for elems in (0,) + OFFSETS32:
        view, guard = O.shifted(t, elems)
        assert (view * 3.0 + 1.0).numpy().tobytes() == want and O.guards_intact(guard)


# ---------------------------------------------------------------------------------------- filter_step through the host twin
FILTER_WIDTHS = (8, 6, 7, 64, 128)
FILTER_OPERANDS = ("x", "z1", "z2", "acc", "out")


def _filter_case(f):
    rowptr, colind = cases.ragged()
    ops = cases.step_operands(rowptr, colind, f, seed=9)
    t = dict((k, torch.from_numpy(ops[k].copy())) for k in ("x", "z1", "z2", "acc", "val", "dst_scale"))
    t["out"] = torch.zeros_like(t["x"])
    return torch.from_numpy(rowptr.copy()), torch.from_numpy(colind.copy()), ops, t


def _filter_call(rp, ci, ops, t):
    return filter_step(rp, ci, t["val"], t["x"], a=ops["a"], b=ops["b"], z1=t["z1"], c1=ops["c1"], z2=t["z2"], c2=ops["c2"],
                       dst_scale=t["dst_scale"], acc=t["acc"], d=ops["d"], out=t["out"])


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def filter_aligned():
    """width -> (out bytes, acc bytes) of the aligned call, checked once against the literal float32 loop."""
    res = {}
    for f in FILTER_WIDTHS:
        rp, ci, ops, t = _filter_case(f)
        out = _filter_call(rp, ci, ops, t)
        want_out, want_acc = cases.step_literal(rp.numpy(), ci.numpy(), ops["val"], ops["x"], ops["a"], ops["b"], ops["z1"],
                                                ops["c1"], ops["z2"], ops["c2"], ops["dst_scale"], ops["acc"], ops["d"])
        assert out is t["out"] and _bytes(out) == want_out.tobytes() and _bytes(t["acc"]) == want_acc.tobytes()
        res[f] = (_bytes(out), _bytes(t["acc"]))
    return res


@pytest.mark.parametrize("offset", OFFSETS32)
@pytest.mark.parametrize("which", FILTER_OPERANDS + ("all",))
@pytest.mark.parametrize("f", FILTER_WIDTHS)
def test_filter_step_host_twin_at_an_offset(filter_aligned, f, which, offset):
    rp, ci, ops, t = _filter_case(f)
    guards = {}
    for name in (FILTER_OPERANDS if which == "all" else (which,)):
        t[name], guards[name] = O.shifted(t[name], offset if which != "all" else 1)
    out = _filter_call(rp, ci, ops, t)
    assert out is t["out"]
    assert (_bytes(out), _bytes(t["acc"])) == filter_aligned[f]
    assert all(O.guards_intact(g) for g in guards.values())


@pytest.mark.parametrize("offset", OFFSETS32)
@pytest.mark.parametrize("f", FILTER_WIDTHS)
def test_filter_step_host_twin_out_is_z1_both_shifted(filter_aligned, f, offset):
    rp, ci, ops, t = _filter_case(f)
    t["z1"], guard = O.shifted(t["z1"], offset)
    t["out"] = t["z1"]
    out = _filter_call(rp, ci, ops, t)
    assert out is t["z1"] and (_bytes(out), _bytes(t["acc"])) == filter_aligned[f] and O.guards_intact(guard)


@pytest.mark.parametrize("which", FILTER_OPERANDS)
def test_filter_step_refuses_a_strided_operand_by_name(which):
    rp, ci, ops, t = _filter_case(8)
    t[which] = O.strided(t[which])
    with pytest.raises(_lib.BackendError, match="%s must be contiguous" % which):
        _filter_call(rp, ci, ops, t)


# ------------------------------------------------------------------------------------------- the address decisions of xcdplan
@pytest.fixture
def no_gpu_library(monkeypatch):
    """The decisions below are taken before anything asks the GPU library: loading it fails the test."""
    def boom():
        raise AssertionError("an address decision loaded the GPU library")

    monkeypatch.setattr(_lib, "hip", boom)


def _x(n, f, dtype, elems):
    return O.shifted(torch.zeros(n, f, dtype=dtype), elems)[0]


@pytest.mark.parametrize("dtype,offsets", [(torch.float32, OFFSETS32), (torch.bfloat16, OFFSETS16), (torch.float16, OFFSETS16)])
def test_spmm_split_sends_an_offset_operand_to_the_ordinary_launch(monkeypatch, no_gpu_library, dtype, offsets):
    monkeypatch.setattr(xcdplan, "MODE", "force")
    rowptr = torch.empty(301, dtype=torch.int32, device="meta")
    per16 = 16 // torch.zeros(0, dtype=dtype).element_size()
    for elems in (0, per16):
        assert xcdplan.spmm_split(None, rowptr, 300, 3500, _x(300, 64, dtype, elems)) == xcdplan.SPLIT
    for elems in offsets:
        x = _x(300, 64, dtype, elems)
        assert x.data_ptr() % 16 != 0
        assert xcdplan.spmm_split(None, rowptr, 300, 3500, x) is None
        csc = types.SimpleNamespace(colptr=rowptr, rowind=torch.empty(3500, dtype=torch.int32, device="meta"), sightings=2)
        assert xcdplan.spmm_backward(None, csc, x, True) == (None, None)      # the upstream gradient
        assert xcdplan.spmm_forward(None, rowptr, csc.rowind, x) == (None, None)
    monkeypatch.setattr(xcdplan, "MODE", "off")
    assert xcdplan.spmm_split(None, rowptr, 300, 3500, _x(300, 64, dtype, 0)) is None


ROUND = 4096


def _csc(n_rows=300, n_src=300):
    return types.SimpleNamespace(n_cols=n_rows, m=n_src, nnz=3500, sightings=2, has_hub_columns=lambda: False)


def test_backward_sweep_asks_for_eight_byte_operands(monkeypatch, no_gpu_library):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    monkeypatch.setattr(xcdplan, "SWEEP_MIN_TABLE_BYTES", 0)
    for elems, want in ((0, True), (2, True), (4, True), (1, False), (3, False)):
        g = _x(300, 128, torch.float32, elems)
        assert xcdplan.spmm_backward_sweep(_csc(), g, round_rows=ROUND) is want, elems


def test_forward_sweep_asks_for_eight_byte_operands(monkeypatch, no_gpu_library):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    monkeypatch.setattr(xcdplan, "SWEEP_MIN_TABLE_BYTES", 0)
    monkeypatch.setattr(plan, "VERIFY_HITS", False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    sp = types.SimpleNamespace(hash=1234, long_rows=False, out_of_order=0.0)
    monkeypatch.setattr(sweepplan, "candidate", lambda meta: sp)
    monkeypatch.setattr(sweepplan, "takeable", lambda s: True)

    def boom():
        raise AssertionError("the forward policy never waits for the hash")

    fp = types.SimpleNamespace(dev=object(), meta=("cpu", 300, 3500, 300), wait=boom, key=boom)
    rowptr = torch.empty(301, dtype=torch.int32, device="meta")
    colind = torch.empty(3500, dtype=torch.int32, device="meta")
    for elems, want in ((0, sp), (2, sp), (1, None), (3, None)):
        x = _x(300, 128, torch.float32, elems)
        assert xcdplan.spmm_forward_sweep(fp, rowptr, colind, x, round_rows=ROUND) is want, elems


def test_aligned_is_the_address_modulo_the_lane():
    t = torch.zeros(64)
    for elems in range(0, 9):
        v = O.shifted(t, elems)[0]
        assert xcdplan.aligned(v, 16) == (elems % 4 == 0) and xcdplan.aligned(v, 8) == (elems % 2 == 0) and xcdplan.aligned(v, 4)
