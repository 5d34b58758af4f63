"""Knowledge-graph training batches on the CPU: the host twin of negative_batch follows csrc/kgsample_law.h -- the published
known answers, the numpy restatement on every case of tests/_kgsample_cases.py, membership and range against Python sets, the
uniformity condition; train_tables equals the reference's Python dictionaries (restated here, and as recorded from the reference
in tests/golden/kg_sample.npz) and refuses what it must; TrainBatches follows the reference iterator's order, epochs and batch
lengths, and the sid law makes a positive's negatives independent of the batch size."""
import inspect
import math

import numpy as np
import pytest
import torch

import _kgsample_cases as C
from cogdl_amd import _lib
from cogdl_amd.kgsample import TrainBatches, train_tables
from cogdl_amd.operators import kgsample as KS
from cogdl_amd.operators import negative_batch

_TABLES = {}


def tables_of(mode):
    if mode not in _TABLES:
        _TABLES[mode] = train_tables(torch.tensor(C.sweep_kg(mode)[0]), C.N)
    return _TABLES[mode]


def twin(name):
    c = C.make(name)
    return negative_batch(tables_of(c["mode"]), c["mode"], torch.from_numpy(c["order"]), c["K"], C.SEED, c["first_sid"],
                          index_dtype=c["index_dtype"])


def one_list_tables(a, n, mode):
    """Tables in which triple i's `mode` list is `a` (the other entity is 1)."""
    return train_tables(torch.tensor([(e, 0, 1) if mode == "head-batch" else (1, 0, e) for e in a]), n)


def test_known_answers():
    a = [0, 3, 4, 10]
    for mode, sid, want in (("tail-batch", 0, [1, 8, 5, 1, 2, 6, 2, 7]), ("head-batch", 2 ** 32 + 5, [9, 5, 8, 2, 8, 7, 7, 6])):
        assert C.law_row(a, 11, 0, mode, sid, 8).tolist() == want
        for dtype in (torch.int64, torch.int32):
            pos, neg, _ = negative_batch(one_list_tables(a, 11, mode), mode, torch.tensor([2], dtype=torch.int32), 8, 0, sid,
                                         index_dtype=dtype)
            assert neg.dtype == dtype and neg.tolist() == [want]
            assert pos.tolist() == [[4, 0, 1] if mode == "head-batch" else [1, 0, 4]]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_twin_equals_the_restatement(name):
    c = C.make(name)
    pos, neg, weight = twin(name)
    want_pos, want_neg, want_weight = C.restated(name)
    assert pos.dtype == torch.int64 and neg.dtype == c["index_dtype"] and weight.dtype == torch.float32
    assert tuple(neg.shape) == (len(c["order"]), c["K"])
    assert np.array_equal(pos.numpy(), want_pos)
    assert np.array_equal(neg.numpy().astype(np.int64), want_neg)
    assert weight.numpy().tobytes() == want_weight.tobytes()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_negatives_are_in_range_and_never_true(name):
    c = C.make(name)
    lists = C.true_lists(c["triples"], c["mode"])  # Python sets over the triples: nothing of the tables
    neg = twin(name)[1].numpy()
    assert neg.min() >= 0 and neg.max() < C.N
    for row, t in zip(neg, c["order"]):
        true = lists[C.list_key(c["triples"][t], c["mode"])]
        assert not true.intersection(row.tolist())
        if len(true) == C.N - 1:
            assert len(set(row.tolist())) == 1  # the one free entity


def python_tables(triples, mode):
    lists = C.true_lists(triples, mode)
    return {key: sorted(v) for key, v in lists.items()}


def tables_as_dict(tables, triples, mode):
    m = tables.modes[mode]
    ptr, idx, group = m.list_ptr.tolist(), m.list_idx.tolist(), m.group.tolist()
    assert ptr[0] == 0 and ptr[-1] == len(idx) and len(group) == len(triples)
    out = {}
    for t, g in zip(triples, group):
        got = idx[ptr[g]:ptr[g + 1]]
        assert out.setdefault(C.list_key(t, mode), got) == got
    assert len(out) == len(ptr) - 1  # one list per group, none per query
    return out


def test_tables_equal_the_reference_dictionaries():
    triples = C.small_kg()[0][:300]
    multiplicity = {}
    for t in triples:
        multiplicity[t] = multiplicity.get(t, 0) + 1
    assert {2, 3} <= set(multiplicity.values())
    tables = train_tables(torch.tensor(triples), 40)
    assert tables.triples.dtype == torch.int32 and tables.triples.tolist() == [list(t) for t in triples]
    for mode in C.MODES:
        m = tables.modes[mode]
        assert m.list_ptr.dtype == m.list_idx.dtype == m.group.dtype == torch.int32
        assert tables_as_dict(tables, triples, mode) == python_tables(triples, mode)
    assert max(len(v) for v in python_tables(triples, "head-batch").values()) >= 30  # the hub
    count = C.frequency(triples)
    want = torch.cat([C.reference_weight(count, t) for t in triples])
    assert tables.weight.dtype == torch.float32 and tables.weight.numpy().tobytes() == want.numpy().tobytes()
    # a list of tuples, as the reference keeps its triples, serves as well
    again = train_tables(triples, 40)
    assert torch.equal(again.weight, tables.weight) and torch.equal(again.modes["head-batch"].list_idx, tables.modes["head-batch"].list_idx)


def test_tables_equal_the_recorded_reference():
    g = np.load(C.GOLDEN)
    triples = [tuple(int(v) for v in row) for row in g["triples"]]
    assert triples == C.small_kg()[0]
    train = triples[int(g["train_start"]):int(g["valid_start"])]
    tables = train_tables(torch.tensor(train), int(g["num_entities"]))
    for mode in C.MODES:
        side = mode.split("-")[0]
        ptr, idx = g["list_ptr_" + side].tolist(), g["list_idx_" + side].tolist()
        recorded = {tuple(int(v) for v in key): idx[ptr[i]:ptr[i + 1]] for i, key in enumerate(g["keys_" + side])}
        assert tables_as_dict(tables, train, mode) == recorded
        assert tables.weight.numpy().tobytes() == g["weight_" + side].tobytes()


def test_tables_refusals():
    ok = [(0, 0, 1), (1, 0, 2)]
    for bad in ([(0, 0, 3)], [(3, 0, 0)], [(-1, 0, 0)], [(0, -1, 1)]):
        with pytest.raises(ValueError):
            train_tables(torch.tensor(ok + bad), 3)
    with pytest.raises(ValueError):
        train_tables(torch.tensor(ok), 2 ** 31 - 1)                     # N beyond int32
    with pytest.raises(ValueError):
        train_tables(torch.zeros((1, 3), dtype=torch.int8).expand(2 ** 31 - 1, 3), 3)  # T beyond int32 (a view: no memory)
    with pytest.raises(ValueError):
        train_tables(torch.tensor([(0, 0, 1), (1, 0, 1), (2, 0, 1)]), 3)  # every entity is a true head of (0, 1)
    with pytest.raises(ValueError):
        train_tables(torch.tensor([[0.0, 0.0, 1.0]]), 3)
    train_tables(torch.tensor([(0, 0, 1), (1, 0, 1)]), 3)               # one entity free: served


def test_entry_point_refuses_a_full_list_and_a_foreign_id():
    """M = 0 and an id of T at the C entry point: -1 rows, the status raised, the other rows untouched."""
    tables = one_list_tables([0, 1, 2], 4, "tail-batch")
    order = torch.tensor([0, 3, 1, -1], dtype=torch.int32)
    want = negative_batch(tables, "tail-batch", order[[0, 2]].contiguous(), 6, 5, 0, check=True)
    with pytest.raises(_lib.BackendError):
        negative_batch(tables, "tail-batch", order, 6, 5, 0)
    pos, neg, weight = negative_batch(tables, "tail-batch", order, 6, 5, 0, check=False)
    assert int(tables.status) == 1
    assert pos[[1, 3]].eq(-1).all() and neg[[1, 3]].eq(-1).all() and weight[[1, 3]].eq(0).all()
    assert torch.equal(pos[0], want[0][0]) and torch.equal(neg[0], want[1][0]) and neg[0].eq(3).all()
    # (row 2 is positive first_sid + 2: its own draws, still the one free entity)
    assert torch.equal(pos[2], want[0][1]) and neg[2].eq(3).all()
    full = one_list_tables([0, 1, 2], 4, "tail-batch")
    full.num_entities = 3  # past the refusal of train_tables: every entity is true
    pos, neg, weight = negative_batch(full, "tail-batch", order[:1], 6, 5, 0, check=False)
    assert int(full.status) == 2 and pos.eq(-1).all() and neg.eq(-1).all()
    with pytest.raises(_lib.BackendError):
        negative_batch(full, "tail-batch", order[:1], 6, 5, 0)


def test_empty_batches_launch_nothing(monkeypatch):
    tables = one_list_tables([0, 3], 5, "head-batch")

    def refuse(*a, **k):
        raise AssertionError("a launch for an empty batch")

    monkeypatch.setattr(_lib, "twin_call", refuse)
    pos, neg, weight = negative_batch(tables, "head-batch", torch.zeros(0, dtype=torch.int32), 7, 0, 0)
    assert tuple(pos.shape) == (0, 3) and tuple(neg.shape) == (0, 7) and tuple(weight.shape) == (0,)
    pos, neg, weight = negative_batch(tables, "head-batch", torch.tensor([1, 0], dtype=torch.int32), 0, 0, 0)
    assert pos.tolist() == [[3, 0, 1], [0, 0, 1]] and tuple(neg.shape) == (2, 0) and torch.equal(weight, tables.weight[[1, 0]])
    with pytest.raises(ValueError):
        negative_batch(tables, "single", torch.zeros(1, dtype=torch.int32), 1, 0, 0)


def test_uniformity():
    """65536 draws over the 7 free entities of N = 11, list [0, 3, 4, 10]: every count within 5 sigma of n / 7."""
    a, n_ent, k = [0, 3, 4, 10], 11, 128
    free = [e for e in range(n_ent) if e not in a]
    worst = 0.0
    for seed in (0, 1, 12345):
        for mode in C.MODES:
            tables = one_list_tables(a, n_ent, mode)
            order = torch.zeros(512, dtype=torch.int32)
            neg = negative_batch(tables, mode, order, k, seed, 0)[1].numpy()
            assert np.array_equal(neg[:3], np.stack([C.law_row(a, n_ent, seed, mode, sid, k) for sid in range(3)]))
            counts = np.bincount(neg.reshape(-1), minlength=n_ent)
            n = int(counts.sum())
            assert n == 65536 and all(counts[e] == 0 for e in a)
            sigma = math.sqrt(n * (1 / 7) * (6 / 7))
            dev = max(abs(int(counts[e]) - n / 7) for e in free) / sigma
            print("seed %d %s: largest deviation %.2f sigma" % (seed, mode, dev))
            worst = max(worst, dev)
            assert dev <= 5.0, (seed, mode, counts.tolist())
    print("largest deviation over all runs %.2f sigma" % worst)


def batches(it, count):
    return [next(it) for _ in range(count)]


def test_iterator_order_epochs_and_lengths():
    triples = C.small_kg()[0][:23]
    it = TrainBatches(triples, 40, 6, 5, seed=11)
    got = batches(it, 20)  # two epochs of five batches per mode
    assert [b[3] for b in got] == ["tail-batch", "head-batch"] * 10
    index = {}
    for i, t in enumerate(triples):
        index.setdefault(t, []).append(i)
    for mode in C.MODES:
        mine = [b for b in got if b[3] == mode]
        assert [b[0].shape[0] for b in mine] == [5, 5, 5, 5, 3] * 2
        for epoch in (mine[:5], mine[5:]):
            served = sorted(tuple(row) for b in epoch for row in b[0].tolist())
            assert served == sorted(triples)  # a permutation of 0 .. T-1 (equal triples are interchangeable)
        assert [tuple(r) for b in mine[:5] for r in b[0].tolist()] != [tuple(r) for b in mine[5:] for r in b[0].tolist()]
        for b in mine:
            assert b[0].dtype == torch.int64 and b[1].dtype == torch.int64 and b[2].dtype == torch.float32
            assert tuple(b[1].shape) == (b[0].shape[0], 6) and tuple(b[2].shape) == (b[0].shape[0],)
    # the ids themselves: a permutation per epoch
    it = TrainBatches(triples, 40, 2, 5, seed=11)
    seen = {mode: [] for mode in C.MODES}
    real = it._order

    def spy(mode):
        order = real(mode)
        seen[mode].append(order.tolist())
        return order

    it._order = spy
    batches(it, 20)
    for mode in C.MODES:
        flat = [i for o in seen[mode] for i in o]
        assert sorted(flat[:23]) == list(range(23)) and sorted(flat[23:]) == list(range(23)) and flat[:23] != flat[23:]
    # two iterators with one seed agree exactly; another seed does not
    a, b, c = (batches(TrainBatches(triples, 40, 6, 5, seed=s), 12) for s in (3, 3, 4))
    assert all(x[3] == y[3] and all(torch.equal(p, q) for p, q in zip(x[:3], y[:3])) for x, y in zip(a, b))
    assert any(not torch.equal(x[1], y[1]) for x, y in zip(a, c))


def test_sid_law_makes_negatives_independent_of_the_batch_size():
    triples = C.small_kg()[0][:23]
    per_size = []
    for size in (7, 3):
        it = TrainBatches(triples, 40, 9, size, seed=5, shuffle=False)
        rows = {mode: [] for mode in C.MODES}
        while min(len(v) for v in rows.values()) < 46:  # two epochs per mode
            pos, neg, weight, mode = next(it)
            rows[mode] += [(tuple(p), tuple(n), w) for p, n, w in zip(pos.tolist(), neg.tolist(), weight.tolist())]
        per_size.append({mode: v[:46] for mode, v in rows.items()})
    assert per_size[0] == per_size[1]
    for mode in C.MODES:
        assert [r[0] for r in per_size[0][mode]] == triples + triples  # ascending order, epoch after epoch
        assert per_size[0][mode][0][1] != per_size[0][mode][23][1]     # the second visit is another positive of the stream


def test_apply_to_device_is_a_noop_on_the_current_device():
    triples = C.small_kg()[0][:23]
    a, b = TrainBatches(triples, 40, 6, 5, seed=9), TrainBatches(triples, 40, 6, 5, seed=9)
    batches(a, 3), batches(b, 3)
    tables = b.tables
    assert b.apply_to_device(torch.device("cpu")) is b and b.apply_to_device("cpu") is b and b.tables is tables
    for x, y in zip(batches(a, 9), batches(b, 9)):
        assert x[3] == y[3] and all(torch.equal(p, q) for p, q in zip(x[:3], y[:3]))


def test_install_takes_the_flag():
    import cogdl_amd
    from cogdl_amd import kgsample_compat

    sig = inspect.signature(cogdl_amd.install)
    assert "kg_sample" in sig.parameters and sig.parameters["kg_sample"].default is False
    assert "kg_sample=True" in cogdl_amd.install.__doc__
    assert callable(kgsample_compat.train_wrapper)
    assert KS.LDS_LIST == 1024 and KS.TAGS == C.TAGS
