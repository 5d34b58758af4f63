"""The one policy of cogdl_amd/xcdplan.py -- does a launch run over an XCD-partitioned plan, and cut at which row length? -- as a
decision table, host logic only: stand-in fingerprints that count their waits, meta tensors for the hub-heavy sizes (H never looks
at the structure), stub plan look-ups.  Expected values are written out from the rule list in DESIGN.md ("XCD-partitioned column
plans"), not computed with the code under test.  That the operators launch what the policy says is pinned on the GPU by
tests/test_xcd_gpu.py."""
import types

import pytest
import torch

from cogdl_amd import _lib, plan, synth, xcdplan

HUB_N, HUB_NNZ = synth.REDDIT_NODES, 114_848_857  # (the sizes of test_xcd_gpu.py::test_wanted_rule)
SPLIT = 256


class _Fp:
    """A plan.Fingerprint stand-in.  key: already read; pending: what a wait would deliver (a hash in flight)."""

    def __init__(self, key=None, pending=None):
        self._key, self._pending, self.waits = key, pending, 0

    def key(self):
        if self._key is None:
            self.waits += 1
            self._key = self._pending
        return self._key

    def wait(self):
        if self._pending is not None:
            self.key()


def _meta(n, dtype=torch.int32):
    return torch.empty(n, dtype=dtype, device="meta")


def _x(n, f, dtype):
    return torch.empty(n, f, dtype=dtype, device="meta")


class _Case:
    """The three structures of the table and the exact-row bounds of their sizes."""

    def __init__(self):
        self.skewed = synth.hub_csr(3000, 2500, base_deg=4, seed=2)
        self.flat = synth.random_csr(3000, 2500, 8, seed=2, ragged=False)
        exact = _lib.hip().cogdl_hip_exact_row_edges
        self.e_hub, self.e_skewed, self.e_flat = exact(HUB_NNZ), exact(self.skewed.nnz), exact(self.flat.nnz)
        assert len({self.e_hub, self.e_skewed, SPLIT}) == 3  # the table can tell the three cuts apart

    def hub(self):
        return _meta(HUB_N + 1), _meta(HUB_NNZ)

    def small(self, which, memoised=False):
        g = self.skewed if which == "skewed" else self.flat
        rowptr = g.rowptr.clone()
        if memoised:
            rowptr._cogdl_amd_struct = object()  # (what structure_memo attaches: plan.memoised)
        return rowptr, g.colind


@pytest.fixture
def case(monkeypatch):
    monkeypatch.setattr(xcdplan, "MODE", "auto")
    monkeypatch.setattr(xcdplan, "ORDERED_MIN_EDGES", 1000)
    # the look-ups behind a decision: not the policy's business (the real ones wait for the key and build)
    monkeypatch.setattr(xcdplan, "csr_plan", lambda fp, rowptr, colind, split=None: ("csr", SPLIT if split is None else split, fp))
    monkeypatch.setattr(xcdplan, "csc_plan", lambda fp, csc, split=None: ("csc", SPLIT if split is None else split, fp))
    xcdplan._SKEW.clear()
    assert xcdplan.SPLIT == SPLIT and not plan.taping() and not plan.transient()
    yield _Case()
    plan.set_tape(None)
    xcdplan._SKEW.clear()


def _in_flight(name):
    return _Fp(pending=(name,))


def _known(name):
    return _Fp(key=(name,))


def _spmm_fwd(fp, structure, x):
    split, xplan = xcdplan.spmm_forward(fp, structure[0], structure[1], x)
    assert (xplan is None) == (split is None) and (xplan is None or xplan[:2] == ("csr", split))
    return split


# ------------------------------------------------------------------------------------------------- csr_spmm forward
def test_spmm_forward_hub_heavy_launches_need_no_key(case, monkeypatch):
    hashed = []
    monkeypatch.setattr(plan, "fingerprint_of", lambda rowptr, colind, n_cols: hashed.append(n_cols) or _in_flight("hub"))
    fp = _in_flight("hub")
    assert _spmm_fwd(fp, case.hub(), _x(HUB_N, 32, torch.float32)) == case.e_hub   # fp32: the exact-row bound
    assert _spmm_fwd(fp, case.hub(), _x(HUB_N, 64, torch.bfloat16)) == SPLIT       # 16-bit: SPLIT
    assert _spmm_fwd(fp, case.hub(), _x(HUB_N, 64, torch.float16)) == SPLIT
    assert fp.waits == 0 and hashed == []
    assert _spmm_fwd(fp, case.hub(), _x(HUB_N, 48, torch.bfloat16)) is None        # 96-byte rows: not H; hash in flight: not S
    assert fp.waits == 0
    # a call that hashed nothing (inference, no memo): the plan's key is hashed for here
    split, xplan = xcdplan.spmm_forward(None, *case.hub(), _x(HUB_N, 32, torch.float32))
    assert split == case.e_hub and hashed == [HUB_N] and xplan[2].key() == ("hub",)
    assert xcdplan.spmm_forward(None, *case.hub(), _x(HUB_N, 48, torch.bfloat16)) == (None, None) and hashed == [HUB_N]


def test_spmm_forward_takes_only_2d_float_operands(case):
    fp = _known("hub")
    assert _spmm_fwd(fp, case.hub(), torch.empty(HUB_N, 4, 8, device="meta")) is None
    assert _spmm_fwd(fp, case.hub(), _x(HUB_N, 32, torch.float64)) is None
    assert _spmm_fwd(fp, case.hub(), _x(HUB_N, 32, torch.int32)) is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_spmm_forward_small_structures_need_a_known_key(case, dtype):
    x = _x(2500, 64, dtype)
    assert _spmm_fwd(None, case.small("skewed"), x) is None                        # no fingerprint
    fp = _in_flight("s")
    assert _spmm_fwd(fp, case.small("skewed"), x) is None and fp.waits == 0        # hash in flight: the ordinary launch, NO wait
    assert _spmm_fwd(_known("s"), case.small("skewed"), x) == case.e_skewed        # key read already: S -> E whatever the dtype
    fp = _in_flight("s")
    assert _spmm_fwd(fp, case.small("skewed", memoised=True), x) == case.e_skewed and fp.waits == 1  # memoised: ONE wait
    assert _spmm_fwd(fp, case.small("skewed", memoised=True), x) == case.e_skewed and fp.waits == 1  # ... per structure
    assert _spmm_fwd(_known("f"), case.small("flat"), x) is None                   # not skewed
    fp = _in_flight("f")
    assert _spmm_fwd(fp, case.small("flat", memoised=True), x) is None and fp.waits == 1
    assert xcdplan._SKEW == {("s",): True, ("f",): False}


def test_spmm_forward_below_ordered_min_edges(case, monkeypatch):
    monkeypatch.setattr(xcdplan, "ORDERED_MIN_EDGES", case.skewed.nnz + 1)
    assert _spmm_fwd(_known("s"), case.small("skewed"), _x(2500, 64, torch.float32)) is None


def test_spmm_forward_recording_waits_and_tapes_its_decision(case):
    x = _x(2500, 64, torch.float32)
    tape = plan.PlanTape()
    plan.set_tape(tape)
    fp_s, fp_f, fp_h = _in_flight("s"), _in_flight("f"), _in_flight("hub")
    assert _spmm_fwd(fp_s, case.small("skewed"), x) == case.e_skewed and fp_s.waits == 1   # not memoised: the recording run waits
    assert _spmm_fwd(fp_f, case.small("flat"), x) is None and fp_f.waits == 1
    assert _spmm_fwd(fp_h, case.hub(), _x(HUB_N, 64, torch.bfloat16)) == SPLIT and fp_h.waits == 1
    assert tape.choices == [("csr_spmm.forward", (case.e_skewed, ("csr", case.e_skewed, fp_s))), ("csr_spmm.forward", (None, None)),
                            ("csr_spmm.forward", (SPLIT, ("csr", SPLIT, fp_h)))]
    # the capture replays them by position: nothing is decided, nothing waited for (its fingerprints have no hash behind them)
    tape.mode = "replay"
    blank = _Fp()
    assert _spmm_fwd(blank, case.small("flat"), x) == case.e_skewed
    assert _spmm_fwd(blank, case.small("skewed"), x) is None and blank.waits == 0
    with pytest.raises(_lib.BackendError):
        xcdplan.spmm_backward(blank, None, x, False)  # (another call site than the recorded one)


def test_transient_structures_never_take_a_plan(case):
    x = _x(2500, 64, torch.float32)
    tape = plan.PlanTape()
    csc = types.SimpleNamespace(colptr=case.skewed.rowptr, rowind=case.skewed.colind, sightings=5)
    with plan.transient_structures():
        assert xcdplan.spmm_forward(_known("s"), *case.small("skewed", memoised=True), x) == (None, None)
        assert xcdplan.spmm_forward(None, *case.hub(), _x(HUB_N, 32, torch.float32)) == (None, None)
        assert xcdplan.spmm_backward(_known("s"), csc, x, True) == (None, None)
        assert xcdplan.gat_forward(_known("s"), *case.small("skewed", memoised=True), 2500, 256) is None
        assert xcdplan.gat_forward(_known("hub"), *case.hub(), HUB_N, 128) is None
        plan.set_tape(tape)
        assert xcdplan.spmm_forward(None, *case.small("skewed"), x) == (None, None)
        assert tape.choices == []  # a transient forward call takes no place on the tape
        xcdplan.MODE = "force"
        assert xcdplan.spmm_forward(None, *case.small("skewed"), x) == (None, None)


def test_spmm_mode_off_and_force(case, monkeypatch):
    x32, x16 = _x(2500, 64, torch.float32), _x(2500, 64, torch.bfloat16)
    monkeypatch.setattr(xcdplan, "MODE", "off")
    assert _spmm_fwd(_known("hub"), case.hub(), _x(HUB_N, 32, torch.float32)) is None
    assert _spmm_fwd(_known("s"), case.small("skewed", memoised=True), x32) is None
    csc = types.SimpleNamespace(colptr=case.skewed.rowptr, rowind=case.skewed.colind, sightings=2)
    assert xcdplan.spmm_backward(_known("s"), csc, x32, True) == (None, None)
    monkeypatch.setattr(xcdplan, "MODE", "force")
    # force: every structure, cut at SPLIT whatever the dtype (kept as is: fp32 too), no key needed, no wait
    fp = _in_flight("x")
    assert _spmm_fwd(fp, case.hub(), _x(HUB_N, 32, torch.float32)) == SPLIT
    assert _spmm_fwd(fp, case.small("skewed"), x32) == SPLIT and _spmm_fwd(fp, case.small("flat"), x16) == SPLIT and fp.waits == 0
    csc.sightings = 1
    assert xcdplan.spmm_backward(_known("s"), csc, x32, False) == (SPLIT, ("csc", SPLIT, _ANY))
    # ... except what the plan kernels cannot address; S is NOT consulted under force (kept as is)
    assert _spmm_fwd(_known("s"), case.small("skewed"), _x(1 << 24, 64, torch.float32)) is None
    empty = (torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    assert _spmm_fwd(_known("e"), empty, _x(3, 64, torch.float32)) is None


class _Any:
    def __eq__(self, other):
        return True


_ANY = _Any()


# ------------------------------------------------------------------------------------------------ csr_spmm backward
def test_spmm_backward_counts_the_key_from_the_second_sighting_on(case):
    x32, x16 = _x(3000, 64, torch.float32), _x(3000, 64, torch.bfloat16)
    fp = _known("s")
    csc = types.SimpleNamespace(colptr=case.skewed.rowptr, rowind=case.skewed.colind, sightings=1)
    assert xcdplan.spmm_backward(fp, csc, x32, False) == (None, None)                                  # first sighting
    assert xcdplan.spmm_backward(fp, csc, x32, True) == (case.e_skewed, ("csc", case.e_skewed, fp))    # ... after a plan forward
    csc.sightings = 2
    assert xcdplan.spmm_backward(fp, csc, x32, False) == (case.e_skewed, ("csc", case.e_skewed, fp))   # second sighting
    assert xcdplan.spmm_backward(fp, csc, x16, False) == (case.e_skewed, ("csc", case.e_skewed, fp))   # S: E whatever the dtype
    flat = types.SimpleNamespace(colptr=case.flat.rowptr, rowind=case.flat.colind, sightings=9)
    assert xcdplan.spmm_backward(_known("f"), flat, x32, True) == (None, None)
    # H needs no key: first sighting or not
    hub = types.SimpleNamespace(colptr=_meta(HUB_N + 1), rowind=_meta(HUB_NNZ), sightings=1)
    assert xcdplan.spmm_backward(fp, hub, _x(HUB_N, 32, torch.float32), False)[0] == case.e_hub
    assert xcdplan.spmm_backward(fp, hub, _x(HUB_N, 64, torch.bfloat16), False)[0] == SPLIT
    assert xcdplan.spmm_backward(fp, hub, torch.empty(HUB_N, 4, 16, device="meta"), False) == (None, None)
    tape = plan.PlanTape()
    plan.set_tape(tape)
    xcdplan.spmm_backward(fp, csc, x32, False)
    assert tape.choices == [("csr_spmm.backward", (case.e_skewed, ("csc", case.e_skewed, fp)))]


# ---------------------------------------------------------------------------------------------------- fused GAT
def test_gat_forward(case):
    fp = _in_flight("hub")
    assert xcdplan.gat_forward(fp, *case.hub(), HUB_N, 128) == ("csr", SPLIT, fp) and fp.waits == 0   # H: no key needed
    assert xcdplan.gat_forward(fp, *case.hub(), HUB_N, 96) is None and fp.waits == 0                  # not H, hash in flight
    fp = _in_flight("s")
    assert xcdplan.gat_forward(fp, *case.small("skewed"), 2500, 256) is None and fp.waits == 0        # NO wait
    fp = _known("s")
    assert xcdplan.gat_forward(fp, *case.small("skewed"), 2500, 256) == ("csr", SPLIT, fp)            # the GAT cut is always SPLIT
    fp = _in_flight("s")
    assert xcdplan.gat_forward(fp, *case.small("skewed", memoised=True), 2500, 256) == ("csr", SPLIT, fp) and fp.waits == 1
    fp = _in_flight("f")
    assert xcdplan.gat_forward(fp, *case.small("flat", memoised=True), 2500, 256) is None and fp.waits == 1
    assert xcdplan.gat_forward(_known("f"), *case.small("flat"), 2500, 256) is None
    assert xcdplan.gat_forward(_known("s"), *case.small("skewed"), 2500, None) is None                # an operand the kernels refuse


def test_gat_forward_recording_and_modes(case, monkeypatch):
    tape = plan.PlanTape()
    plan.set_tape(tape)
    fp = _in_flight("s")
    assert xcdplan.gat_forward(fp, *case.small("skewed"), 2500, 256) == ("csr", SPLIT, fp) and fp.waits == 1  # recording: waits
    assert xcdplan.gat_forward(_known("s"), *case.small("skewed"), 2500, None) is None
    assert tape.choices == [("fused_gat.forward", ("csr", SPLIT, fp)), ("fused_gat.forward", None)]
    tape.mode = "replay"
    blank = _Fp()
    assert xcdplan.gat_forward(blank, *case.small("flat"), 2500, 256) == ("csr", SPLIT, fp) and blank.waits == 0
    plan.set_tape(None)
    monkeypatch.setattr(xcdplan, "MODE", "off")
    assert xcdplan.gat_forward(_known("hub"), *case.hub(), HUB_N, 128) is None
    assert xcdplan.gat_forward(_known("s"), *case.small("skewed"), 2500, 256) is None
    monkeypatch.setattr(xcdplan, "MODE", "force")
    fp = _in_flight("f")
    assert xcdplan.gat_forward(fp, *case.small("flat"), 2500, 256) == ("csr", SPLIT, fp) and fp.waits == 0
    assert xcdplan.gat_forward(fp, *case.small("flat"), 2500, None) is None


def test_gat_backward(case):
    fp = _known("s")
    rowptr, colind = case.small("skewed")
    csc = types.SimpleNamespace(sightings=1)
    both = (("csr", SPLIT, fp), ("csc", SPLIT, fp))
    assert xcdplan.gat_backward(fp, csc, rowptr, colind, 2500, 256, False) is None       # first sighting
    assert xcdplan.gat_backward(fp, csc, rowptr, colind, 2500, 256, True) == both        # the forward ran the plan kernels
    csc.sightings = 2
    assert xcdplan.gat_backward(fp, csc, rowptr, colind, 2500, 256, False) == both       # second sighting and S
    assert xcdplan.gat_backward(_known("f"), csc, *case.small("flat"), 2500, 256, False) is None
    # H is not asked again (kept as is): a hub-heavy launch whose forward fell back takes S's answer
    xcdplan._SKEW[("hub",)] = False
    assert xcdplan.gat_backward(_known("hub"), csc, *case.hub(), HUB_N, 128, False) is None
    xcdplan.MODE = "force"  # (kept as is: force reaches the backward only through a forward call that took the plan)
    assert xcdplan.gat_backward(_known("f"), csc, *case.small("flat"), 2500, 256, False) is None
    xcdplan.MODE = "auto"
    tape = plan.PlanTape()
    plan.set_tape(tape)
    xcdplan.gat_backward(fp, csc, rowptr, colind, 2500, 256, False)
    assert tape.choices == [("fused_gat.backward", both)]


# --------------------------------------------------------------------------------------------- memoised edge lists
def test_edge_list_wanted(case, monkeypatch):
    capturing = [False]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])

    def edges(g, uses):
        return types.SimpleNamespace(rowptr=g.rowptr, perm=g.colind, uses=uses, skewed=None)

    assert xcdplan.EDGE_LIST_MIN_COLUMNS == 65
    assert not xcdplan.edge_list_wanted(edges(case.skewed, 1), 128)      # first use
    assert not xcdplan.edge_list_wanted(edges(case.skewed, 2), 64)       # rows of more than 64 columns only
    e = edges(case.skewed, 2)
    capturing[0] = True
    assert not xcdplan.edge_list_wanted(e, 65) and e.skewed is None      # the skew test reads back: never inside a capture
    capturing[0] = False
    assert xcdplan.edge_list_wanted(e, 65) and e.skewed is True
    capturing[0] = True
    assert xcdplan.edge_list_wanted(e, 65)                               # ... once cached it needs no read-back
    capturing[0] = False
    e = edges(case.flat, 2)
    assert not xcdplan.edge_list_wanted(e, 128) and e.skewed is False
    monkeypatch.setattr(xcdplan, "ORDERED_MIN_EDGES", case.skewed.nnz + 1)
    assert not xcdplan.edge_list_wanted(edges(case.skewed, 2), 128)
    monkeypatch.setattr(xcdplan, "MODE", "force")
    assert xcdplan.forced() and xcdplan.edge_list_wanted(edges(case.flat, 0), 1)
    empty = types.SimpleNamespace(rowptr=torch.zeros(4, dtype=torch.int32), perm=torch.zeros(0, dtype=torch.int32), uses=5, skewed=None)
    assert not xcdplan.edge_list_wanted(empty, 128)
    monkeypatch.setattr(xcdplan, "MODE", "off")
    assert not xcdplan.forced() and not xcdplan.edge_list_wanted(edges(case.skewed, 5), 128)


# ----------------------------------------------------------------------------------------- the facts' public helpers
def test_the_predicates_the_policy_asks():
    t = torch.zeros(3, dtype=torch.int32)
    assert not plan.memoised(t)
    t._cogdl_amd_struct = object()
    assert plan.memoised(t)
    assert not plan.taping() and not plan.recording()
    tape = plan.PlanTape()
    plan.set_tape(tape)
    try:
        assert plan.taping() and plan.recording()
        tape.mode = "replay"
        assert plan.taping() and not plan.recording() and plan.replaying()
    finally:
        plan.set_tape(None)
    assert plan.CscPlan(t, t, t, 2, 2, 0).sightings == 1

    class Event:
        waits = 0

        def synchronize(self):
            self.waits += 1

    fp = plan.Fingerprint.__new__(plan.Fingerprint)  # (no device here: the fields a hash in flight would have)
    fp.meta, fp._key, fp.event, fp.host = (0, 2, 0, 2), None, Event(), torch.tensor([5, 6])
    fp.wait()
    assert fp.key() == (0, 2, 0, 2, 11) and fp.event.waits == 1
    fp.wait()
    assert fp.event.waits == 1
    fp._key, fp.event, fp.host = None, None, None  # made while a capture replays: nothing to wait for
    fp.wait()
    assert fp._key is None
