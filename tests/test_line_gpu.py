"""The LINE kernel (csrc/line.hip) on the GPU: the serial mode equals the host twin bit for bit over the grid of
_line_cases.py; the chunking of the throughput mode alone, and a Hogwild run whose concurrent samples share no row, equal the
serial result bit for bit too; the throughput mode reaches the twin's and the reference's embedding quality on the
planted-partition graph; error flags instead of faults; stream use; the reference's unchanged LINE class."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cogdl_amd import _lib, embedding
from cogdl_amd.operators import line as line_mod
from cogdl_amd.operators import line_train
from cogdl_amd.operators import sgns as sgns_mod

from _line_cases import (GRID, QUALITY, SAMPLES_PER_NODE, graph, grid_id, grid_init, grid_run, quality_edges, reference_purity,
                         twin_purity)
from test_sgns_host import ROOT, neighbour_purity, planted_partition

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tables(out):
    return (out,) if torch.is_tensor(out) else tuple(out)


def _assert_same(host, gpu):
    host, gpu = _tables(host), _tables(gpu)
    assert len(host) == len(gpu)
    for name, h, g in zip(("emb", "ctx"), host, gpu):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == h.shape
        assert torch.equal(h, g.cpu()), "%s: max difference %g" % (name, float((h - g.cpu()).abs().max()))


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_serial_mode_equals_the_host_twin_bit_for_bit(case):
    _assert_same(grid_run(case), grid_run(case, DEV))


def test_serial_mode_continues_from_the_callers_tables_and_runs_twice_alike():
    case = ("weighted", 1000, 65, 5, 2)
    first = grid_run(case)
    host = grid_run(case, init=first, seed=4)
    init = (first[0].to(DEV), first[1].to(DEV))
    gpu = grid_run(case, DEV, init=init, seed=4)
    again = grid_run(case, DEV, init=init, seed=4)
    assert torch.equal(init[0].cpu(), first[0]) and torch.equal(init[1].cpu(), first[1])  # init is not modified
    _assert_same(host, gpu)
    assert torch.equal(gpu[0], again[0]) and torch.equal(gpu[1], again[1])


@pytest.mark.parametrize("order", [1, 2])
def test_one_sample_in_flight_equals_the_serial_result(monkeypatch, order):
    """Launches of one sample each: the chunking of the throughput mode alone."""
    case = ("weighted", 61, 65, 5, order)
    monkeypatch.setattr(line_mod, "SAMPLES_IN_FLIGHT", 1)
    _assert_same(grid_run(case), grid_run(case, DEV, workers=0))


def _big_random_graph():
    g = torch.Generator().manual_seed(3)
    return torch.randint(0, 2 ** 17, (2 ** 18, 2), generator=g), 2 ** 17


def _disjoint_seed(edges, v, samples, k, in_flight):
    """The first seed in 0..31 with which no two samples of one launch of `in_flight` consecutive samples touch a common row
    (input row or target row, of either table), read from the host trace; None if there is none."""
    for seed in range(32):
        rec = line_train(edges, v, 1, 2, samples, negative=k, seed=seed, workers=1, trace=samples * (k + 1))[-1].numpy()
        ok = True
        for first in range(0, samples, in_flight):
            seen = {}
            for s, u, t, _, _ in rec[(rec[:, 0] >= first) & (rec[:, 0] < first + in_flight)]:
                for row in (int(u), int(t)):
                    ok &= seen.setdefault(row, s) == s
        if ok:
            return seed
    return None


@pytest.mark.parametrize("order", [1, 2])
def test_hogwild_launches_whose_samples_share_no_row_equal_the_serial_twin(monkeypatch, order):
    """SAMPLES_IN_FLIGHT = 8, S = 61 (a partial last launch of 5 samples: three waves of its second workgroup have no sample),
    D = 65, on a graph of 2^17 nodes and 2^18 edges.  The seed is chosen on the CPU so that the samples of a launch are
    independent; the concurrent result is then a function of the inputs and must equal the serial twin's."""
    edges, v = _big_random_graph()
    samples, k, d = 61, 5, 65
    seed = _disjoint_seed(edges, v, samples, k, 8)
    assert seed is not None
    init = sgns_mod.init_tables(v, d, 7, "cpu")
    other = sgns_mod.init_tables(v, d, 8, "cpu")[0]
    init = init[0] if order == 1 else (init[0], other)
    kw = dict(negative=k, alpha=0.05, seed=seed)
    host = line_train(edges, v, d, order, samples, workers=1, init=init, **kw)
    monkeypatch.setattr(line_mod, "SAMPLES_IN_FLIGHT", 8)
    init_d = init.to(DEV) if order == 1 else (init[0].to(DEV), init[1].to(DEV))
    gpu = line_train(edges.to(DEV), v, d, order, samples, workers=0, init=init_d, **kw)
    _assert_same(host, gpu)
    assert not torch.equal(_tables(host)[0], _tables(init)[0])


@pytest.mark.parametrize("order", [1, 2])
def test_throughput_mode_reaches_the_twins_and_the_references_quality(order):
    edges, n, community = quality_edges()
    init = sgns_mod.init_tables(n, QUALITY["dim"], 2, DEV)
    out = line_train(edges.to(DEV), n, QUALITY["dim"], order, SAMPLES_PER_NODE * n, negative=QUALITY["negative"],
                     alpha=QUALITY["alpha"], seed=2, init=init[0] if order == 1 else init)
    got, host, ref = neighbour_purity(_tables(out)[0], community), twin_purity(order), reference_purity()[order]
    print("neighbour purity, order %d: GPU throughput mode %.4f, serial host twin %.4f, reference %.4f" % (order, got, host, ref))
    for t, t0 in zip(_tables(out), init):
        assert torch.isfinite(t).all() and not torch.equal(t, t0)
    assert got >= host - 0.05
    assert got >= ref - 0.05


def test_embedding_line_order_3_reaches_the_twins_and_the_references_quality():
    indptr, indices, n, community = planted_partition()
    emb = embedding.line((indptr.to(DEV), indices.to(DEV)), dim=64, walk_length=80, walk_num=20, negative=QUALITY["negative"],
                         alpha=QUALITY["alpha"], order=3, seed=2)
    assert emb.is_cuda and emb.dtype == torch.float32 and tuple(emb.shape) == (n, 64) and torch.isfinite(emb).all()
    assert torch.allclose(emb[:, :32].norm(dim=1), torch.ones(n, device=DEV), atol=1e-5)
    assert torch.allclose(emb[:, 32:].norm(dim=1), torch.ones(n, device=DEV), atol=1e-5)
    got, host, ref = neighbour_purity(emb, community), twin_purity(3), reference_purity()[3]
    print("neighbour purity, order 3: embedding.line on the GPU %.4f, serial host twin %.4f, reference %.4f" % (got, host, ref))
    assert got >= host - 0.05
    assert got >= ref - 0.05


def test_flags_instead_of_faults():
    edges, v, w = graph("weighted")
    m = edges.shape[0]
    bad = edges.clone()
    bad[5, 1] = v
    for workers in (0, 1):
        with pytest.raises(_lib.BackendError, match="outside"):
            line_train(bad.to(DEV), v, 16, 1, 500, seed=1, workers=workers)
    bad[5, 1] = 2 ** 40
    with pytest.raises(_lib.BackendError, match="outside"):
        line_train(bad.to(DEV), v, 16, 2, 500, seed=1, edge_weight=w)
    bad[5, 1] = -1
    with pytest.raises(_lib.BackendError, match="outside"):
        line_train(bad.to(DEV), v, 16, 2, 500, seed=1, workers=1)
    ncum = sgns_mod.build_tables(line_mod.weighted_degree(edges, v, w), 0, 0.75)[1]
    ecum = line_mod.edge_table(w)
    back = ncum.clone()
    back[100] = back[99] - 1
    ebad = ecum.clone()
    ebad[10] = ecum[9] - 1
    for workers in (0, 1):
        with pytest.raises(_lib.BackendError, match="noise table"):
            line_train(edges.to(DEV), v, 16, 1, 500, seed=1, workers=workers, tables=(ecum, back))
        with pytest.raises(_lib.BackendError, match="noise table"):
            line_train(edges.to(DEV), v, 16, 1, 500, seed=1, workers=workers, tables=(None, torch.zeros(v, dtype=torch.long)))
        with pytest.raises(_lib.BackendError, match="edge table"):
            line_train(edges.to(DEV), v, 16, 2, 500, seed=1, workers=workers, tables=(ebad, ncum))
        with pytest.raises(_lib.BackendError, match="edge table"):
            line_train(edges.to(DEV), v, 16, 2, 500, seed=1, workers=workers, tables=(torch.zeros(m, dtype=torch.long), ncum))
    # the tables are not touched when a flag is raised
    lib = _lib.hip()
    init = sgns_mod.init_tables(v, 16, 1, DEV)
    emb, ctx = init[0].clone(), (init[0] * 2).clone()
    ctx0 = ctx.clone()
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    ed = edges.to(DEV)
    eu, ev = ed[:, 0].contiguous(), ed[:, 1].contiguous()
    n32, table = sgns_mod._u32(back, DEV), sgns_mod.exp_table().to(DEV)
    e64 = ebad.to(DEV)
    for workers in (0, 1):
        rc = lib.cogdl_hip_line_train(_lib.ptr(eu), _lib.ptr(ev), _lib.ptr(e64), m, v, _lib.ptr(n32), _lib.ptr(table), 16, 5, 2, 500, 0.025,
                                      1, workers, 0, _lib.ptr(emb), _lib.ptr(ctx), _lib.ptr(flags), _lib.stream_of(ed))
        assert rc == 0 and int(flags) in (2, 4, 6)  # (flags are raised without atomics: of two different bits one may be lost)
        assert torch.equal(emb, init[0]) and torch.equal(ctx, ctx0)
    torch.cuda.synchronize()
    good = line_train(ed, v, 16, 2, 500, seed=1, edge_weight=w)  # the device is fine afterwards
    assert torch.isfinite(good[0]).all() and not torch.equal(good[0], init[0])


def test_line_train_on_a_side_stream_is_ordered_with_the_callers_work():
    case = ("random", 1000, 64, 5, 2)
    edges, v, _ = graph("random")
    want = grid_run(case, seed=8)
    init = grid_init(case, DEV)
    # priority -1, as in test_metapath_gpu.py: torch hands high-priority streams out of a pool of their own, and the runtime
    # gives that pool its own hardware queues.  A stream of the ordinary pool would shift by one which pool stream, and with it
    # which hardware queue, every later test's side stream gets: the overlap test of test_pipeline_gpu.py needs its side
    # stream on another queue than the stream that trains.
    side = torch.cuda.Stream(device=DEV, priority=-1)
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3  # work in front of the call on this stream
        ed = torch.zeros(tuple(edges.shape), dtype=torch.long, device=DEV)
        ed.copy_(edges.to(DEV), non_blocking=True)  # the kernel must see this copy
        emb, ctx = line_train(ed, v, 64, 2, 1000, negative=5, alpha=0.05, seed=8, workers=1, init=init)
        total = emb.sum() + ctx.sum()  # and this must see the kernel's result
    side.synchronize()
    assert torch.equal(emb.cpu(), want[0]) and torch.equal(ctx.cpu(), want[1])
    assert float(total) == pytest.approx(float(want[0].sum() + want[1].sum()), rel=1e-4, abs=1e-5)


# ------------------------------------------------------------------------------------------------------- end to end
REF_PKG = os.path.join(ROOT, "oracle", "_ref", "pkg")

REFERENCE_SCRIPT = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
from tools import refpkg
refpkg.setup(install=True)
from cogdl_amd.install import install, uninstall
from cogdl.models.emb.line import LINE
reference_forward = LINE.forward
install(line=True)
assert LINE.forward is not reference_forward and LINE.forward.__module__ == "cogdl_amd.line_compat"
from cogdl.data import Graph
from test_sgns_host import planted_partition, neighbour_purity
indptr, indices, n, community = planted_partition()
row = torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])
g = Graph(edge_index=torch.stack([row, indices]), num_nodes=n).to(sys.argv[2])
model = LINE(64, 80, 20, 5, 1000, 0.025, 3)
torch.manual_seed(1)
emb = model(g)
assert isinstance(emb, np.ndarray) and emb.dtype == np.float64 and emb.shape == (n, 64), (emb.dtype, emb.shape)
d = model.forward(g, return_dict=True)
assert isinstance(d, dict) and len(d) == n and d[5].shape == (64,)
assert model.dimension == 64
print("purity %.4f" % neighbour_purity(torch.from_numpy(emb), community))
uninstall()
assert LINE.forward is reference_forward
'''


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_PKG, "cogdl")), reason="the reference package is not staged under oracle/_ref/pkg")
def test_reference_line_class_runs_under_install_line():
    out = subprocess.run([sys.executable, "-c", REFERENCE_SCRIPT, ROOT, DEV], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    purity = float(out.stdout.strip().splitlines()[-1].split()[-1])
    print("reference LINE under install(line=True): neighbour purity %.4f" % purity)
    assert purity >= 0.95
