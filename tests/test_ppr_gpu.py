"""Top-k personalised PageRank on the GPU (csrc/ppr.hip): the kernel returns the host twin's arrays bit for bit, on the
fixture graphs, on an R-MAT graph with hub rows, with the table in LDS and in the workspace; error flags instead of faults.
Every case launches once."""
import os

import numpy as np
import pytest
import torch

from cogdl_amd import _lib, synth
from cogdl_amd.operators import ppr as ppr_mod
from cogdl_amd.operators import topk_ppr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppr.npz"))
CONFIGS = [(float(a), float(e), int(k)) for a, e, k in GOLDEN["configs"]]


def fixture_graph(name):
    return torch.from_numpy(GOLDEN[name + "_indptr"]), torch.from_numpy(GOLDEN[name + "_indices"])


def rmat_graph():
    n = 1 << 14
    src, dst = synth.rmat_pairs(n, 200_000, seed=3)
    g = synth.finalize(src, dst, n, symmetrise=True, self_loops=False, norm="sym")
    assert int(g.degrees().max()) > 500
    return g.rowptr.long(), g.colind.long(), n


def both(indptr, indices, sources, alpha, eps, topk):
    host = topk_ppr(indptr, indices, sources, alpha, eps, topk)
    gpu = topk_ppr(indptr.to(DEV), indices.to(DEV), sources.to(DEV), alpha, eps, topk)
    assert all(t.is_cuda for t in gpu)
    return host, tuple(t.cpu() for t in gpu)


def assert_same(host, gpu, what):
    for h, g, name in zip(host, gpu, ("nbr", "val", "count")):
        assert h.dtype == g.dtype and h.shape == g.shape, (what, name)
        assert h.numpy().tobytes() == g.numpy().tobytes(), "%s: %s differs between GPU and host twin" % (what, name)


@pytest.mark.parametrize("name", ["sym", "iso", "directed"])
@pytest.mark.parametrize("config", range(3))
def test_gpu_equals_host_on_fixture_graphs(name, config):
    indptr, indices = fixture_graph(name)
    alpha, eps, topk = CONFIGS[config]
    sources = torch.from_numpy(GOLDEN["sources"])
    assert_same(*both(indptr, indices, sources, alpha, eps, topk), what="%s config %d" % (name, config))


# (alpha, eps): the first keeps the table in LDS on the R-MAT graph for sources of small degree, the second and third need
# the workspace (PPRGo's and MVGRL's parameters)
@pytest.mark.parametrize("alpha,eps,lds", [(0.5, 1e-2, True), (0.5, 1e-4, False), (0.4, 1e-4, False)])
@pytest.mark.parametrize("n_sources", [1, 63, 64, 65, 3000])
def test_gpu_equals_host_on_rmat(alpha, eps, lds, n_sources):
    indptr, indices, n = rmat_graph()
    deg = indptr[1:] - indptr[:-1]
    if lds:  # sources of degree <= 500: 1 + deg + 1 / (alpha eps) <= 1024 entries
        pool = torch.nonzero(deg <= 500).flatten()
    else:  # every node, the hubs first
        pool = torch.argsort(deg, descending=True, stable=True)
    sources = pool[torch.arange(n_sources) % pool.numel()].contiguous()
    if n_sources >= 64:
        sources[1] = sources[0]  # a repeated source
    plan = ppr_mod.plan(n, indices.numel(), int(deg[sources].max()), alpha, eps)
    assert plan["lds"] == lds
    host, gpu = both(indptr, indices, sources, alpha, eps, 32)
    assert_same(host, gpu, what="rmat S=%d" % n_sources)
    if n_sources >= 64:
        assert torch.equal(gpu[0][0], gpu[0][1]) and torch.equal(gpu[1][0], gpu[1][1])


def test_hub_sources_with_lds_sized_budget_use_the_workspace_and_agree():
    indptr, indices, n = rmat_graph()
    deg = indptr[1:] - indptr[:-1]
    sources = torch.argsort(deg, descending=True, stable=True)[:16].contiguous()
    assert not ppr_mod.plan(n, indices.numel(), int(deg.max()), 0.5, 1e-2)["lds"]
    assert_same(*both(indptr, indices, sources, 0.5, 1e-2, 64), what="hub sources")


def test_arxiv_shaped_graph_pprgo_defaults():
    g = synth.arxiv_like(seed=0)
    n = g.num_nodes
    indptr, indices = g.rowptr.long(), g.colind.long()
    sources = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:4096].contiguous()
    nbr, val, count = topk_ppr(indptr.to(DEV), indices.to(DEV), sources.to(DEV), 0.5, 1e-4, 32)  # raises if a flag was set
    nbr, val, count = nbr.cpu(), val.cpu(), count.cpu()
    used = torch.arange(32)[None, :] < count[:, None]
    assert bool((count >= 1).all())
    assert bool(((nbr >= 0) & (nbr < n))[used].all()) and bool((nbr[~used] == -1).all()) and bool((val[~used] == 0).all())
    assert bool((val[:, :-1] >= val[:, 1:]).all()) and bool((val[used] > 0).all())
    assert float(val.double().sum(1).max()) <= 1.0
    assert bool((nbr[:, 0] == sources).all())  # alpha = 0.5: the source keeps the largest score
    rows = torch.arange(0, 4096, 64)
    host = topk_ppr(indptr, indices, sources[rows].contiguous(), 0.5, 1e-4, 32)
    assert_same(host, (nbr[rows], val[rows], count[rows]), what="arxiv sample")


def test_bad_ids_raise_flags_not_faults():
    indptr, indices = fixture_graph("sym")
    n = indptr.numel() - 1
    ip, ix = indptr.to(DEV), indices.to(DEV)
    with pytest.raises(_lib.BackendError, match="source id"):
        topk_ppr(ip, ix, torch.tensor([0, n, 5], device=DEV), 0.5, 1e-4, 8)
    with pytest.raises(_lib.BackendError, match="source id"):
        topk_ppr(ip, ix, torch.tensor([-1], device=DEV), 0.5, 1e-4, 8)
    bad = indices.clone()
    bad[indptr[0]] = n + 7  # a neighbour of node 0
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        topk_ppr(ip, bad.to(DEV), torch.tensor([0], device=DEV), 0.5, 1e-4, 8)
    bad_ptr = indptr.clone()
    bad_ptr[11] = indices.numel() + 1000
    with pytest.raises(_lib.BackendError, match="indptr"):
        topk_ppr(bad_ptr.to(DEV), ix, torch.tensor([10], device=DEV), 0.5, 1e-4, 8)
    # check=False: the rows of the good sources are still right, the bad one is empty
    nbr, val, count = topk_ppr(ip, ix, torch.tensor([0, n, 5], device=DEV), 0.5, 1e-4, 8, check=False, max_source_degree=n)
    good = topk_ppr(indptr, indices, torch.tensor([0, 5]), 0.5, 1e-4, 8, max_source_degree=n)
    assert int(count[1]) == 0 and bool((nbr[1] == -1).all()) and bool((val[1] == 0).all())
    assert torch.equal(nbr[[0, 2]].cpu(), good[0]) and torch.equal(val[[0, 2]].cpu(), good[1])
    with pytest.raises(_lib.BackendError, match="table overflowed"):  # a degree bound that is too small, a tiny budget
        indptr_r, indices_r, _ = rmat_graph()
        hub = int(torch.argmax(indptr_r[1:] - indptr_r[:-1]))
        topk_ppr(indptr_r.to(DEV), indices_r.to(DEV), torch.tensor([hub], device=DEV), 0.5, 0.5, 8, max_source_degree=0)


def test_streams_and_repeated_calls():
    indptr, indices, n = rmat_graph()
    ip, ix = indptr.to(DEV), indices.to(DEV)
    sources = torch.arange(0, n, 16, device=DEV)
    a = topk_ppr(ip, ix, sources, 0.5, 1e-4, 32)
    b = topk_ppr(ip, ix, sources, 0.5, 1e-4, 32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = topk_ppr(ip, ix, sources, 0.5, 1e-4, 32)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    empty = topk_ppr(ip, ix, torch.empty(0, dtype=torch.long, device=DEV), 0.5, 1e-4, 32)
    assert tuple(empty[0].shape) == (0, 32) and empty[2].numel() == 0
