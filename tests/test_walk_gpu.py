"""The walk kernels (csrc/walk.hip) on the GPU: bit-for-bit equal to the host twin over graphs, walker counts, lengths and
parameters; every transition of an arxiv-sized run is an edge; error flags instead of faults; stream and hipGraph use."""
import numpy as np
import pytest
import torch

from cogdl_amd import _lib, synth
from cogdl_amd.operators import node2vec_walk, random_walk
from cogdl_amd.operators import walk as walk_mod
from cogdl_amd.random_walk_compat import RandomWalker

from test_walk_host import GRAPHS, csr_of, n2v_graph, unequal_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PQ = [(0.25, 4.0), (4.0, 0.25), (1.0, 1.0)]


def rmat_graph():
    """R-MAT with hub rows, symmetrised, rows sorted by column (synth.finalize coalesces), int64."""
    n = 1 << 14
    src, dst = synth.rmat_pairs(n, 200_000, seed=3)
    g = synth.finalize(src, dst, n, symmetrise=True, self_loops=False, norm="sym")
    assert int(g.degrees().max()) > 500
    return g.rowptr.long(), g.colind.long(), n


ALL_GRAPHS = dict(GRAPHS, rmat=rmat_graph, n2v=n2v_graph, unequal=unequal_graph)


def both(fn, indptr, indices, start, *args, **kw):
    host = fn(indptr, indices, start, *args, **kw)
    gpu = fn(indptr.to(DEV), indices.to(DEV), start.to(DEV), *args, **kw)
    assert gpu.is_cuda and gpu.dtype == torch.int64
    return host, gpu.cpu()


@pytest.mark.parametrize("name", sorted(ALL_GRAPHS))
def test_gpu_equals_host_on_every_graph(name, monkeypatch):
    indptr, indices, n = ALL_GRAPHS[name]()
    start = torch.randint(0, n, (3000,), generator=torch.Generator().manual_seed(1))
    start[:64] = start[0]  # repeated start ids
    for restart in (0.0, 0.3, 1.0):
        host, gpu = both(random_walk, indptr, indices, start, 33, restart_p=restart, seed=7)
        assert torch.equal(host, gpu), "random_walk restart %g" % restart
    for p, q in PQ:
        host, gpu = both(node2vec_walk, indptr, indices, start, 33, p=p, q=q, seed=8)
        assert torch.equal(host, gpu), "node2vec p=%g q=%g" % (p, q)
    monkeypatch.setattr(walk_mod, "NODE2VEC_TRIALS", 1)
    host, gpu = both(node2vec_walk, indptr, indices, start, 33, p=0.25, q=4.0, seed=9)
    assert torch.equal(host, gpu), "node2vec with the exact fallback forced"


@pytest.fixture(scope="module")
def rmat():
    indptr, indices, n = rmat_graph()
    return (indptr, indices), (indptr.to(DEV), indices.to(DEV)), n


def n2v_both(rmat, start, length, **kw):
    """node2vec_walk with its fallback counts on both sides -> the walks; asserts that walks and counts are equal."""
    host_g, gpu_g, _ = rmat
    hw, hf = node2vec_walk(*host_g, start, length, return_fallback=True, **kw)
    gw, gf = node2vec_walk(*gpu_g, start.to(DEV), length, return_fallback=True, **kw)
    assert gw.is_cuda and gw.dtype == torch.int64 and tuple(gw.shape) == (start.numel(), length)
    assert gf.is_cuda and gf.dtype == torch.int32 and tuple(gf.shape) == (start.numel(),)
    assert torch.equal(hw, gw.cpu()) and torch.equal(hf, gf.cpu())
    return hw


# 255 / 256 / 257: a workgroup short by a lane, exactly one, one lane into a second (parked lanes, the last workgroup)
@pytest.mark.parametrize("w", [0, 1, 63, 64, 65, 255, 256, 257, 100003])
def test_gpu_equals_host_over_walker_counts(rmat, w):
    host_g, gpu_g, n = rmat
    start = torch.randint(0, n, (w,), generator=torch.Generator().manual_seed(w))
    host = random_walk(*host_g, start, 17, restart_p=0.3, seed=70)
    gpu = random_walk(*gpu_g, start.to(DEV), 17, restart_p=0.3, seed=70)
    assert gpu.is_cuda and gpu.dtype == torch.int64 and tuple(gpu.shape) == (w, 17) and torch.equal(host, gpu.cpu())
    n2v_both(rmat, start, 17, p=0.25, q=4.0, seed=71)


# 7 / 8 / 9 / 16: one short of a tile of the kernel's staging, exactly one tile, one past it, two tiles
@pytest.mark.parametrize("length", [1, 2, 7, 8, 9, 16, 80, 257])
def test_gpu_equals_host_over_lengths(rmat, length, monkeypatch):
    host_g, gpu_g, n = rmat
    start = torch.randint(0, n, (1000,), generator=torch.Generator().manual_seed(length))
    for restart in (0.0, 0.3):
        host = random_walk(*host_g, start, length, restart_p=restart, seed=80)
        gpu = random_walk(*gpu_g, start.to(DEV), length, restart_p=restart, seed=80)
        assert gpu.is_cuda and gpu.dtype == torch.int64 and tuple(gpu.shape) == (1000, length) and torch.equal(host, gpu.cpu())
    n2v_both(rmat, start, length, p=4.0, q=0.25, seed=81)
    monkeypatch.setattr(walk_mod, "NODE2VEC_TRIALS", 2)  # (so that the counts are not all zero)
    n2v_both(rmat, start, length, p=0.25, q=4.0, seed=82)


def test_fallback_counts_equal_the_host(monkeypatch):
    indptr, indices, n = rmat_graph()
    start = torch.arange(0, n, 3)
    monkeypatch.setattr(walk_mod, "NODE2VEC_TRIALS", 2)
    hw, hf = node2vec_walk(indptr, indices, start, 20, p=0.25, q=4.0, seed=5, return_fallback=True)
    gw, gf = node2vec_walk(indptr.to(DEV), indices.to(DEV), start.to(DEV), 20, p=0.25, q=4.0, seed=5, return_fallback=True)
    assert torch.equal(hw, gw.cpu()) and torch.equal(hf, gf.cpu()) and int(hf.sum()) > 0


def test_same_seed_same_array_and_streams():
    indptr, indices, n = rmat_graph()
    ip, ix = indptr.to(DEV), indices.to(DEV)
    start = torch.arange(n, device=DEV)
    a = random_walk(ip, ix, start, 40, restart_p=0.2, seed=5)
    assert torch.equal(a, random_walk(ip, ix, start, 40, restart_p=0.2, seed=5))
    assert not torch.equal(a, random_walk(ip, ix, start, 40, restart_p=0.2, seed=6))
    b = node2vec_walk(ip, ix, start, 40, p=0.25, q=4.0, seed=5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a2 = random_walk(ip, ix, start, 40, restart_p=0.2, seed=5)
        b2 = node2vec_walk(ip, ix, start, 40, p=0.25, q=4.0, seed=5)
    side.synchronize()
    assert torch.equal(a, a2) and torch.equal(b, b2)


def test_arxiv_sized_run_walks_edges_only():
    g = synth.arxiv_like(seed=0)
    n = g.num_nodes
    ip, ix = g.rowptr.long().to(DEV), g.colind.long().to(DEV)
    walks = random_walk(ip, ix, torch.arange(n, device=DEV), 80, seed=1)  # raises if a flag was set
    assert tuple(walks.shape) == (n, 80) and bool((walks[:, 0] == torch.arange(n, device=DEV)).all())
    row = torch.repeat_interleave(torch.arange(n, device=DEV), ip[1:] - ip[:-1])
    keys = torch.unique(row * n + ix)  # sorted
    deg = ip[1:] - ip[:-1]
    a, b = walks[:, :-1].reshape(-1), walks[:, 1:].reshape(-1)
    assert a.numel() == n * 79
    want = a * n + b
    pos = torch.searchsorted(keys, want).clamp(max=keys.numel() - 1)
    ok = (keys[pos] == want) | ((a == b) & (deg[a] == 0))
    assert bool(ok.all()), "%d transitions are not edges" % int((~ok).sum())


def test_out_of_range_ids_raise_and_the_gpu_stays_healthy():
    indptr, indices, n = n2v_graph()
    ip, ix = indptr.to(DEV), indices.to(DEV)
    with pytest.raises(_lib.BackendError, match="start id"):
        random_walk(ip, ix, torch.tensor([0, 5, 1], device=DEV), 6, seed=0)
    with pytest.raises(_lib.BackendError, match="start id"):
        node2vec_walk(ip, ix, torch.tensor([-3], device=DEV), 6, seed=0)
    bad = torch.full_like(ix, 1 << 40)
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        random_walk(ip, bad, torch.tensor([0, 1], device=DEV), 6, seed=0)
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        node2vec_walk(ip, bad, torch.tensor([0, 1], device=DEV), 6, seed=0)
    with pytest.raises(_lib.BackendError, match="indptr"):
        random_walk(torch.tensor([0, 2, 1 << 40, 5, 6, 7], device=DEV), ix, torch.tensor([1], device=DEV), 6, seed=0)
    with pytest.raises(_lib.BackendError):
        random_walk(ip, indices, torch.tensor([0], device=DEV), 6)  # mixed devices: refused before any launch
    start = torch.tensor([0, 1, 2], device=DEV)
    assert torch.equal(random_walk(ip, ix, start, 6, seed=2).cpu(), random_walk(indptr, indices, start.cpu(), 6, seed=2))
    torch.cuda.synchronize()


def test_captured_random_walk_replays_to_the_same_array():
    indptr, indices, n = rmat_graph()
    ip, ix = indptr.to(DEV), indices.to(DEV)
    start = torch.arange(4096, device=DEV)
    want = random_walk(ip, ix, start, 24, restart_p=0.1, seed=12)
    out = torch.zeros(4096, 24, dtype=torch.long, device=DEV)
    flags = torch.ones(1, dtype=torch.int32, device=DEV)
    _lib.hip()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # warm-up outside the capture
        random_walk(ip, ix, start, 24, restart_p=0.1, seed=12, out=out, check=False, flags=flags)
    side.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        random_walk(ip, ix, start, 24, restart_p=0.1, seed=12, out=out, check=False, flags=flags)
    for _ in range(2):
        out.zero_()
        flags.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and int(flags.item()) == 0
    walk_mod.raise_for_flags("random_walk", flags, n)


def test_random_walker_keeps_a_cuda_graph_on_the_gpu():
    rng = np.random.default_rng(4)
    n = 5000
    ei = torch.from_numpy(np.stack([rng.integers(0, n, 60000), rng.integers(0, n, 60000)]))
    host = RandomWalker(ei, num_nodes=n)
    gpu = RandomWalker(ei.to(DEV), num_nodes=n)
    assert gpu.indptr.is_cuda and gpu.indices.is_cuda
    assert torch.equal(gpu.indptr.cpu(), host.indptr) and torch.equal(gpu.indices.cpu(), host.indices)
    start = list(range(0, n, 5))
    t = gpu.walk_tensor(start, 12, restart_p=0.25, seed=3)
    assert t.is_cuda and t.dtype == torch.int64
    got = gpu.walk(start, 12, restart_p=0.25, seed=3)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64
    assert np.array_equal(got, host.walk(start, 12, restart_p=0.25, seed=3)) and np.array_equal(got, t.cpu().numpy())
    n2v = gpu.node2vec_walk(torch.tensor(start), 12, p=0.5, q=2.0, seed=3)
    assert n2v.is_cuda and torch.equal(n2v.cpu(), host.node2vec_walk(start, 12, p=0.5, q=2.0, seed=3))
