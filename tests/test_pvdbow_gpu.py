"""The PV-DBOW kernel (csrc/pvdbow.hip) on the GPU: the serial mode equals the host twin bit for bit over the grid of
test_pvdbow_host.py, and twice alike; the throughput mode reaches the twin's quality on the two-family corpus; a launch that
ends on a remainder; error flags instead of faults."""
import pytest
import torch

from cogdl_amd import _lib
from cogdl_amd.operators import doc2vec_dbow
from cogdl_amd.operators import pvdbow as pv_mod
from cogdl_amd.operators import sgns as sgns_mod

from test_pvdbow_host import GRID, KW, LENGTHS, QUALITY, VOCAB, corpus, grid_id, purity, twin_purity, two_family_corpus

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_serial_mode_equals_the_host_twin_bit_for_bit(case):
    d, k_neg, sample = case
    doc_ptr, words = corpus()
    host = doc2vec_dbow(doc_ptr, words, VOCAB, dim=d, negative=k_neg, sample=sample, **KW)
    gpu = doc2vec_dbow(doc_ptr.to(DEV), words.to(DEV), VOCAB, dim=d, negative=k_neg, sample=sample, **KW)
    assert gpu[0].is_cuda and gpu[0].dtype == torch.float32 and tuple(gpu[0].shape) == (len(LENGTHS), d)
    assert tuple(gpu[1].shape) == (VOCAB, d)
    assert torch.equal(host[0], gpu[0].cpu()), "dv: max difference %g" % float((host[0] - gpu[0].cpu()).abs().max())
    assert torch.equal(host[1], gpu[1].cpu()), "syn1: max difference %g" % float((host[1] - gpu[1].cpu()).abs().max())


def test_serial_mode_with_the_store_row_update_equals_the_host_twin_bit_for_bit():
    """Tuning key 17 = 1: syn1 rows are updated by write-through stores of (loaded + delta), which in serial order is the
    law's sum."""
    doc_ptr, words = corpus()
    host = doc2vec_dbow(doc_ptr, words, VOCAB, dim=65, negative=5, sample=0.0, **KW)
    _lib.hip().cogdl_hip_set_tuning(17, 1)
    try:
        gpu = doc2vec_dbow(doc_ptr.to(DEV), words.to(DEV), VOCAB, dim=65, negative=5, sample=0.0, **KW)
    finally:
        _lib.hip().cogdl_hip_set_tuning(17, 0)
    assert torch.equal(host[0], gpu[0].cpu()), "dv: max difference %g" % float((host[0] - gpu[0].cpu()).abs().max())
    assert torch.equal(host[1], gpu[1].cpu()), "syn1: max difference %g" % float((host[1] - gpu[1].cpu()).abs().max())


def test_serial_mode_continues_from_the_callers_tables_and_runs_twice_alike():
    doc_ptr, words = corpus()
    kw = dict(dim=65, negative=5, epochs=1, seed=3, workers=1)
    first = doc2vec_dbow(doc_ptr, words, VOCAB, **kw)
    host = doc2vec_dbow(doc_ptr, words, VOCAB, init=first, **dict(kw, seed=4))
    init = (first[0].to(DEV), first[1].to(DEV))
    gpu = doc2vec_dbow(doc_ptr.to(DEV), words.to(DEV), VOCAB, init=init, **dict(kw, seed=4))
    again = doc2vec_dbow(doc_ptr.to(DEV), words.to(DEV), VOCAB, init=init, **dict(kw, seed=4))
    assert torch.equal(init[0].cpu(), first[0]) and torch.equal(init[1].cpu(), first[1])  # init is not modified
    assert torch.equal(host[0], gpu[0].cpu()) and torch.equal(host[1], gpu[1].cpu())
    assert torch.equal(gpu[0], again[0]) and torch.equal(gpu[1], again[1])
    assert torch.equal(gpu[0][0], init[0][0])  # the empty document


def test_throughput_mode_reaches_the_twins_quality_on_the_two_family_corpus():
    doc_ptr, words, v, family = two_family_corpus()
    host = twin_purity()
    init = pv_mod.init_tables(len(family), v, QUALITY["dim"], 2, DEV)
    dv, syn1 = doc2vec_dbow(doc_ptr.to(DEV), words.to(DEV), v, seed=2, init=init, **QUALITY)
    got = purity(dv, family)
    print("1-NN family purity: GPU throughput mode %.4f, sequential host twin %.4f" % (got, host))
    assert torch.isfinite(dv).all() and torch.isfinite(syn1).all()
    assert not torch.equal(dv, init[0]) and not torch.equal(syn1, init[1])
    assert host >= 0.9
    assert got >= host - 0.05


def test_throughput_mode_with_few_documents_in_flight(monkeypatch):
    """Launches of 8 documents with G = 61: the last launch is a remainder, and no multiple of the workgroup's 4."""
    g = torch.Generator().manual_seed(4)
    lengths = torch.randint(1, 90, (61,), generator=g)
    lengths[7], lengths[60] = 0, 33
    doc_ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(lengths, 0)])
    words = torch.randint(0, 500, (int(doc_ptr[-1]),), generator=g)
    monkeypatch.setattr(pv_mod, "DOCS_IN_FLIGHT", 8)
    init = pv_mod.init_tables(61, 500, 200, 5, DEV)
    dv, syn1 = doc2vec_dbow(doc_ptr.to(DEV), words.to(DEV), 500, dim=200, epochs=2, seed=5, init=init)
    assert torch.isfinite(dv).all() and torch.isfinite(syn1).all()
    empty = lengths == 0
    assert bool(empty.any()) and torch.equal(dv.cpu()[empty], init[0].cpu()[empty])
    # every document with a token was trained, the last one (alone in the remainder launch's second workgroup) included
    moved = (dv.cpu() != init[0].cpu()).any(1)
    assert torch.equal(moved, ~empty)
    seen = torch.zeros(500, dtype=torch.bool)
    seen[words] = True
    assert bool((syn1.cpu()[seen] != 0).any(1).all())


def test_flags_instead_of_faults():
    doc_ptr, words = corpus()
    dp, wd = doc_ptr.to(DEV), words.to(DEV)
    bad = words.clone()
    bad[10] = VOCAB
    with pytest.raises(_lib.BackendError, match="outside"):
        doc2vec_dbow(dp, bad.to(DEV), VOCAB, dim=16, seed=1)
    bad[10] = 2 ** 40
    with pytest.raises(_lib.BackendError, match="outside"):
        doc2vec_dbow(dp, bad.to(DEV), VOCAB, dim=16, seed=1, workers=1)
    back = doc_ptr.clone()
    back[2] = 5
    with pytest.raises(_lib.BackendError, match="doc_ptr"):
        doc2vec_dbow(back.to(DEV), wd, VOCAB, dim=16, seed=1)
    past = doc_ptr.clone()
    past[-1] += 1
    with pytest.raises(_lib.BackendError, match="doc_ptr"):
        doc2vec_dbow(past.to(DEV), wd, VOCAB, dim=16, seed=1)
    keep = torch.full((VOCAB,), 2 ** 32 - 1)
    cum = torch.linspace(1, 2 ** 31 - 1, VOCAB).long()
    cum[20] = cum[19] - 1
    with pytest.raises(_lib.BackendError, match="noise table"):
        doc2vec_dbow(dp, wd, VOCAB, dim=16, seed=1, tables=(keep, cum))
    # the tables are not touched when a flag is raised
    lib = _lib.hip()
    init = pv_mod.init_tables(5, VOCAB, 16, 1, DEV)
    dv, syn1 = init[0].clone(), init[1].clone()
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    k32, c32, table = sgns_mod._u32(keep, DEV), sgns_mod._u32(cum, DEV), sgns_mod.exp_table().to(DEV)
    rc = lib.cogdl_hip_pvdbow_train(_lib.ptr(dp), 5, _lib.ptr(wd), words.numel(), VOCAB, 16, 5, 1, 0.025, 1e-4, _lib.ptr(k32),
                                    _lib.ptr(c32), _lib.ptr(table), 1, 0, 0, _lib.ptr(dv), _lib.ptr(syn1), _lib.ptr(flags),
                                    _lib.stream_of(wd))
    assert rc == 0 and int(flags) == 2
    assert torch.equal(dv, init[0]) and torch.equal(syn1, init[1])
    torch.cuda.synchronize()
    good = doc2vec_dbow(dp, wd, VOCAB, dim=16, seed=1)  # the device is fine afterwards
    assert torch.isfinite(good[0]).all()
