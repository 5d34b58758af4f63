"""The one journal of what install() and the opt-in features replaced, and the only code that reverts a replacement.

An entry is (feature, owner, name, before, value): `value` was put under `name` of `owner` -- an attribute of a module or a
class, or, where `owner` is a dict (sys.modules), a key -- in place of `before` (_ABSENT: nothing was there).  Entries are
kept in the order of recording and reverted in the reverse order, so stacked replacements of one place (the two `spmm`
fronts, each a closure over what it found) unwind from the top whichever feature asks."""
import sys

_ABSENT = object()
_journal = []


def _read(owner, name):
    return (owner if isinstance(owner, dict) else vars(owner)).get(name, _ABSENT)  # (vars: a class's own raw descriptor)


def _write(owner, name, value):
    if isinstance(owner, dict):
        owner.pop(name, None) if value is _ABSENT else owner.__setitem__(name, value)
    elif value is _ABSENT:
        delattr(owner, name)
    else:
        setattr(owner, name, value)


def put(feature, owner, name, value):
    """Bind `value` under `name` of `owner` and record what it replaced.  Idempotent: a place that already holds `value`
    gets no second entry, so the first original is never overwritten by our own object."""
    before = _read(owner, name)
    if before is not value:
        _journal.append((feature, owner, name, before, value))
        _write(owner, name, value)


def put_where_held(feature, name, value, holds):
    """put() in every loaded cogdl / cogdl.* module whose attribute `name` satisfies holds(current): `from x import name`
    copies a function into the importing module, so each holder is rebound."""
    for modname, mod in list(sys.modules.items()):
        if mod is not None and (modname == "cogdl" or modname.startswith("cogdl.")):
            cur = getattr(mod, name, None)
            if cur is not None and holds(cur):
                put(feature, mod, name, value)


def original(owner, name):
    """What `name` of `owner` held before the first recorded replacement (None: no entry, or nothing was there)."""
    for _, o, n, before, _ in _journal:
        if o is owner and n == name:
            return None if before is _ABSENT else before
    return None


def undo(feature=None):
    """Revert, newest first, every entry (feature=None) or the entries of `feature` together with every later entry on the
    same places: those wrap what the feature put there, and a closure cannot be taken out of the middle.  A place that no
    longer holds what the entry put there was rebound by someone else: it is left alone, the entry is dropped all the same."""
    places, victims = set(), []
    for entry in _journal:
        place = (id(entry[1]), entry[2])
        if feature is None or entry[0] == feature or place in places:
            places.add(place)
            victims.append(entry)
    gone = set(map(id, victims))
    _journal[:] = [entry for entry in _journal if id(entry) not in gone]
    for _, owner, name, before, value in reversed(victims):
        if _read(owner, name) is value:
            _write(owner, name, before)
