"""cogdl_amd/_rebind.py: the one journal behind install() / uninstall() and the per-feature uninstall entry points.  The
journal itself is checked on types.ModuleType fakes with a journal of the test's own; what touches sys.modules or installs
real features runs in a child interpreter."""
import json
import os
import subprocess
import sys
import types

import pytest

from cogdl_amd import _rebind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_LIB = os.path.exists(os.path.join(ROOT, "cogdl_amd", "csrc", "libcogdl_hip.so"))


@pytest.fixture
def journal(monkeypatch):
    monkeypatch.setattr(_rebind, "_journal", [])
    return _rebind._journal


def test_put_twice_records_once_and_undo_restores_by_identity(journal):
    mod, first, ours = types.ModuleType("fake"), object(), object()
    mod.thing = first
    _rebind.put("a", mod, "thing", ours)
    _rebind.put("a", mod, "thing", ours)
    assert mod.thing is ours and len(journal) == 1 and _rebind.original(mod, "thing") is first
    _rebind.undo("a")
    assert mod.thing is first and journal == [] and _rebind.original(mod, "thing") is None


def test_undo_deletes_what_was_not_there_before(journal):
    class Base:
        def forward(self):
            return "base"

    class Layer(Base):
        pass

    mod, table = types.ModuleType("fake"), {}  # (a dict owner is how sys.modules is journalled)
    _rebind.put("a", mod, "thing", 1)
    _rebind.put("a", Layer, "forward", lambda self: "ours")
    _rebind.put("a", table, "key", mod)
    assert mod.thing == 1 and Layer().forward() == "ours" and table["key"] is mod and len(journal) == 3
    _rebind.undo()
    assert not hasattr(mod, "thing") and "forward" not in vars(Layer) and Layer().forward() == "base" and table == {}


@pytest.mark.parametrize("feature,left", [(None, "first"), ("a", "first"), ("b", "a")])
def test_two_features_on_one_place_unwind_from_the_top(journal, feature, left):
    mod = types.ModuleType("fake")
    values = {"first": object(), "a": object(), "b": object()}
    mod.thing = values["first"]
    other = types.ModuleType("other")  # a place only A holds: undo("b") must leave it alone
    other.thing = values["first"]
    _rebind.put("a", mod, "thing", values["a"])
    _rebind.put("a", other, "thing", values["a"])
    _rebind.put("b", mod, "thing", values["b"])  # B wraps A
    _rebind.undo(feature)
    assert mod.thing is values[left]
    assert other.thing is values["first" if feature != "b" else "a"]
    assert _rebind.original(mod, "thing") is (values["first"] if feature == "b" else None)
    _rebind.undo("a")  # after undo("b") A is still undoable
    assert mod.thing is values["first"] and other.thing is values["first"] and journal == []


def test_a_place_someone_else_overwrote_is_left_alone_and_forgotten(journal):
    mod, foreign = types.ModuleType("fake"), object()
    mod.thing = "first"
    _rebind.put("a", mod, "thing", "ours")
    mod.thing = foreign
    _rebind.undo()
    assert mod.thing is foreign and journal == []


STACKED_FRONTS = r'''
import json, sys, types
sys.path.insert(0, sys.argv[1])
import cogdl_amd
from cogdl_amd import big_dispatch, fused

def dummy(graph, x, actnn=False, fast_spmm=None, fast_spmm_cpu=None):
    return x

holders = []
for name in ("cogdl", "cogdl.utils", "cogdl.utils.spmm_utils", "cogdl.layers.gcn_layer"):
    sys.modules[name] = mod = types.ModuleType(name)
    mod.spmm = dummy
    holders.append(mod)
back = lambda: all(m.spmm is dummy for m in holders)
result = {}
for case, steps in (("big_fused_uninstall", (big_dispatch.install, fused.install, cogdl_amd.uninstall)),
                    ("fused_big_uninstall", (fused.install, big_dispatch.install, cogdl_amd.uninstall)),
                    ("fused_big_fused_uninstall", (fused.install, big_dispatch.install, fused.uninstall))):
    assert back(), case
    for step in steps[:2]:
        assert step() is True, (case, step)
    stacked = [bool(getattr(m.spmm, "_cogdl_amd_fused", False) or getattr(m.spmm, "_cogdl_amd_big", False)) for m in holders]
    steps[2]()
    result[case] = {"stacked": all(stacked), "back": back()}
    for m in holders:  # (so that one failing case does not fail the next)
        m.spmm = dummy
    big_dispatch.uninstall(), fused.uninstall()
print(json.dumps(result))
'''


@pytest.fixture(scope="module")
def stacked_fronts():
    if not HAVE_LIB:
        pytest.skip("libcogdl_hip.so is not built (the spmm fronts import the operators)")
    out = subprocess.run([sys.executable, "-c", STACKED_FRONTS, ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case", ["big_fused_uninstall", "fused_big_uninstall", "fused_big_fused_uninstall"])
def test_stacked_spmm_fronts_are_undone_in_reverse_order(stacked_fronts, case):
    """install(big_graphs=True), install(fused_norm=True), uninstall() used to leave the 64-bit front bound for good: the
    fronts were undone in a fixed order, not in the reverse order of installation."""
    assert stacked_fronts[case] == {"stacked": True, "back": True}


INSTALL_UNINSTALL = r'''
import importlib.abc, sys, types
ROOT, HAVE_LIB = sys.argv[1], sys.argv[2] == "1"
sys.path.insert(0, ROOT)
ABSENT = ("metis", "torch_sparse", "gensim")

class Absent(importlib.abc.MetaPathFinder):  # the real packages, where installed, cannot be imported in this interpreter
    def find_spec(self, fullname, path=None, target=None):
        if fullname in ABSENT:
            raise ModuleNotFoundError("No module named %r (marked absent)" % fullname, name=fullname)

sys.meta_path.insert(0, Absent())
import torch
import cogdl_amd
from cogdl_amd import _rebind

# a sys.modules key that was absent: undo removes the key
probe = types.ModuleType("cogdl_amd_journal_probe")
_rebind.put("probe", sys.modules, probe.__name__, probe)
_rebind.put("probe", sys.modules, probe.__name__, probe)
assert sys.modules[probe.__name__] is probe and len(_rebind._journal) == 1
_rebind.undo("probe")
assert probe.__name__ not in sys.modules and not _rebind._journal

# install(metis=True) is undone
cogdl_amd.install()
assert "metis" not in sys.modules
cogdl_amd.install(metis=True)
import metis
assert metis.__name__ == "cogdl_amd.metis_compat"
cogdl_amd.uninstall()
assert "metis" not in sys.modules, "uninstall() left metis registered"

# nothing is planted in anybody's namespace, and everything registered is gone afterwards
def planted():
    found = []
    for modname, mod in list(sys.modules.items()):
        for name, value in list(getattr(mod, "__dict__", {}).items()):
            if name.startswith("_cogdl_amd_orig"):
                found.append(modname + "." + name)
            if isinstance(value, type):
                found += [modname + "." + name + "." + a for a in vars(value) if a.startswith("_cogdl_amd_orig")]
    return found

torch_linear = torch.nn.functional.linear
flags = dict(metis=True, torch_sparse=True, skipgram=True)
if HAVE_LIB:
    flags.update(linear=True, fused_norm=True, narrow_side=True)
before = set(sys.modules)
cogdl_amd.install(**flags)
cogdl_amd.install(**flags)
for name in ABSENT + ("gensim.models",):
    assert sys.modules[name].__name__.startswith("cogdl_amd."), name
assert not HAVE_LIB or torch.nn.functional.linear is not torch_linear
assert planted() == [], planted()
cogdl_amd.uninstall()
assert planted() == [], planted()
assert not _rebind._journal and torch.nn.functional.linear is torch_linear
left = [n for n in set(sys.modules) - before if not n.startswith("cogdl_amd")]
assert not [n for n in left if n.split(".")[0] in ABSENT], left
print("ok")
'''


def test_install_then_uninstall_leaves_no_registration_and_no_planted_attribute():
    """install(metis=True) was never undone; the originals used to be planted as _cogdl_amd_orig_* attributes."""
    out = subprocess.run([sys.executable, "-c", INSTALL_UNINSTALL, ROOT, "1" if HAVE_LIB else "0"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")
