"""Knowledge-graph training batches on the GPU: the HIP kernel of negative_batch equals the host twin bit for bit -- positive,
negative and the bits of weight -- on every case of tests/_kgsample_cases.py (true lists of 1, 2, 63, 64, 65 ids, one below, at
and one above the LDS threshold, and all but one entity; K of 1 .. 257; B of 1, 5 and 1027; an ordinal that crosses 2^32; int32
and int64 negatives), with operands that start mid-allocation; an order id of T at the C entry point gives a -1 row and the
status, nothing else changes; empty batches launch nothing; TrainBatches on the GPU serves the CPU iterator's batches."""
import pytest
import torch

import _kgsample_cases as C
import _offset as O
from cogdl_amd import _lib
from cogdl_amd.kgsample import ModeTables, TrainBatches, TrainTables, train_tables
from cogdl_amd.operators import negative_batch

pytestmark = pytest.mark.gpu

DEV = "cuda"
_CPU, _GPU, _TWIN = {}, {}, {}


def tables_of(mode, dev):
    memo = _GPU if dev == DEV else _CPU
    if mode not in memo:
        cpu = _CPU.get(mode) or train_tables(torch.tensor(C.sweep_kg(mode)[0]), C.N)
        _CPU[mode] = cpu
        memo[mode] = cpu.to(dev)
    return memo[mode]


def twin(name):
    if name not in _TWIN:
        c = C.make(name)
        _TWIN[name] = negative_batch(tables_of(c["mode"], "cpu"), c["mode"], torch.from_numpy(c["order"]), c["K"], C.SEED,
                                     c["first_sid"], index_dtype=c["index_dtype"])
    return _TWIN[name]


def same(got, want):
    return all(g.is_cuda and g.dtype == w.dtype and g.shape == w.shape and g.cpu().numpy().tobytes() == w.numpy().tobytes()
               for g, w in zip(got, want))


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_kernel_equals_the_twin_bit_for_bit(name):
    c = C.make(name)
    got = negative_batch(tables_of(c["mode"], DEV), c["mode"], torch.from_numpy(c["order"]).to(DEV), c["K"], C.SEED,
                         c["first_sid"], index_dtype=c["index_dtype"])
    assert same(got, twin(name))


@pytest.mark.parametrize("name", ["k65_sid_hi", "b5_i32", "k128"])
def test_operands_that_start_mid_allocation(name):
    """Every table and the order 4 bytes past a 16-byte boundary: the same bits."""
    c = C.make(name)
    cpu = tables_of(c["mode"], "cpu")
    shifted = TrainTables(O.shifted(cpu.triples, 1, device=DEV)[0], O.shifted(cpu.weight, 1, device=DEV)[0],
                          {k: ModeTables(*(O.shifted(getattr(m, f), 1, device=DEV)[0] for f in ("list_ptr", "list_idx", "group")))
                           for k, m in cpu.modes.items()}, cpu.num_entities)
    order = O.shifted(torch.from_numpy(c["order"]), 1, device=DEV)[0]
    assert shifted.triples.data_ptr() % 16 == 4 and order.data_ptr() % 16 == 4
    assert shifted.modes[c["mode"]].list_idx.data_ptr() % 16 == 4
    got = negative_batch(shifted, c["mode"], order, c["K"], C.SEED, c["first_sid"], index_dtype=c["index_dtype"])
    assert same(got, twin(name))


def test_entry_point_refuses_an_order_id_of_T():
    """An input check, nothing is dereferenced with the id: the row is -1, the status is raised, every other row is the
    twin's; outputs that start mid-allocation keep their guards."""
    c = C.make("b5_sid_hi")
    mode, k = c["mode"], c["K"]
    tables = tables_of(mode, DEV)
    m = tables.modes[mode]
    order = torch.from_numpy(c["order"]).clone()
    order[2] = tables.num_triples
    order_d = order.to(DEV)
    pos, gp = O.shifted(torch.zeros((5, 3), dtype=torch.int64), 1, device=DEV)
    neg, gn = O.shifted(torch.zeros((5, k), dtype=torch.int64), 1, device=DEV)
    weight, gw = O.shifted(torch.zeros(5), 1, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    rc = _lib.hip().cogdl_hip_kg_train_batch(
        tables.triples.data_ptr(), tables.weight.data_ptr(), m.group.data_ptr(), m.list_ptr.data_ptr(), m.list_idx.data_ptr(),
        tables.num_triples, m.list_ptr.numel() - 1, m.list_idx.numel(), order_d.data_ptr(), 5, k, C.N, C.SEED, C.TAGS[mode],
        c["first_sid"], 1, pos.data_ptr(), neg.data_ptr(), weight.data_ptr(), status.data_ptr(), _lib.stream_of(pos))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status) == 1
    assert O.guards_intact(gp) and O.guards_intact(gn) and O.guards_intact(gw)
    want = twin("b5_sid_hi")
    keep = [0, 1, 3, 4]
    assert pos[2].eq(-1).all() and neg[2].eq(-1).all() and float(weight[2]) == 0.0
    assert torch.equal(pos.cpu()[keep], want[0][keep]) and torch.equal(neg.cpu()[keep], want[1][keep])
    assert weight.cpu()[keep].numpy().tobytes() == want[2][keep].numpy().tobytes()
    with pytest.raises(_lib.BackendError):
        negative_batch(tables, mode, order_d, k, C.SEED, c["first_sid"])
    got = negative_batch(tables, mode, order_d, k, C.SEED, c["first_sid"], check=False)
    assert torch.equal(got[1], neg) and int(tables.status) == 1
    negative_batch(tables, mode, torch.from_numpy(c["order"]).to(DEV), k, C.SEED, c["first_sid"])  # the status is zeroed per call


def test_empty_batches_launch_nothing(monkeypatch):
    tables = tables_of("head-batch", DEV)

    def refuse(*a, **k):
        raise AssertionError("a launch for an empty batch")

    monkeypatch.setattr(_lib, "twin_call", refuse)
    pos, neg, weight = negative_batch(tables, "head-batch", torch.zeros(0, dtype=torch.int32, device=DEV), 7, 0, 0)
    assert pos.is_cuda and tuple(pos.shape) == (0, 3) and tuple(neg.shape) == (0, 7) and tuple(weight.shape) == (0,)
    order = torch.tensor([4, 0], dtype=torch.int32, device=DEV)
    pos, neg, weight = negative_batch(tables, "head-batch", order, 0, 0, 0)
    assert tuple(neg.shape) == (2, 0) and torch.equal(pos, tables.triples[order.long()].long())
    assert torch.equal(weight, tables.weight[order.long()])


def test_train_batches_on_the_gpu_equal_the_cpu_iterator():
    triples = C.small_kg()[0][:300]
    cpu = TrainBatches(triples, 40, 33, 70, seed=21, shuffle=False)
    gpu = TrainBatches(triples, 40, 33, 70, seed=21, shuffle=False, device=DEV)
    moved = TrainBatches(triples, 40, 33, 70, seed=21, shuffle=False)
    assert moved.apply_to_device(torch.device(DEV)) is moved and moved.device.type == "cuda"
    tables = moved.tables
    moved.apply_to_device(torch.device("cuda", torch.cuda.current_device()))
    assert moved.tables is tables
    for _ in range(6):
        want = next(cpu)
        for it in (gpu, moved):
            got = next(it)
            assert got[3] == want[3] and same(got[:3], want[:3])
    # shuffled: a permutation per epoch, drawn on the device
    it = TrainBatches(triples[:23], 40, 4, 5, seed=21, device=DEV)
    rows = [next(it) for _ in range(10)]
    assert [r[0].shape[0] for r in rows if r[3] == "tail-batch"] == [5, 5, 5, 5, 3]
    assert sorted(tuple(p) for r in rows if r[3] == "head-batch" for p in r[0].tolist()) == sorted(triples[:23])
