"""Random walks without a GPU: the host twin (libcogdl_host.so) behind cogdl_amd.operators.walk, the RandomWalker shim
and install(random_walk=True).  The GPU kernels return the same arrays bit for bit (tests/test_walk_gpu.py), so the
distribution tests here cover both.

Distribution tests: Pearson's chi-square of the observed counts against the exact law, failing above the 1 - 1e-6 quantile
of the chi-square law with (cells - 1) degrees of freedom.  Seeds are fixed, so the outcome is deterministic; a correct
generator fails a case with probability 1e-6, one that cannot pick the last neighbour of a row, or carries a modulo bias
of 1e-3, exceeds the quantile by orders of magnitude at 1e6 samples."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.stats import chi2

from _walk_cases import GRAPHS, csr_of, n2v_graph, path_with_sink, random_with_isolated
from cogdl_amd import _lib
from cogdl_amd.operators import node2vec_walk, random_walk
from cogdl_amd.operators import walk as walk_mod
from cogdl_amd.random_walk_compat import RandomWalker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pkg")
REF = STAGED if os.path.isdir(os.path.join(STAGED, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")
QUANTILE = 1.0 - 1e-6


def check_transitions(indptr, indices, n, start, walks, restart):
    """Every consecutive pair (a, b): an edge a -> b, or a == b at a node without out-neighbours, or (restart > 0) b a
    neighbour of the walker's start."""
    indptr_n, indices_n = indptr.numpy(), indices.numpy()
    row = np.repeat(np.arange(n), np.diff(indptr_n))
    keys = np.unique(row * n + indices_n)
    deg = np.diff(indptr_n)
    w = walks.numpy()
    assert w.min() >= 0 and w.max() < n
    a, b = w[:, :-1], w[:, 1:]
    ok = np.isin(a * n + b, keys) | ((a == b) & (deg[a] == 0))
    if restart > 0:
        s = np.broadcast_to(np.asarray(start)[:, None], a.shape)
        ok |= np.isin(s * n + b, keys)
    assert ok.all(), "a transition that is not an edge: %s" % (np.argwhere(~ok)[:5],)


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("restart", [0.0, 0.3])
def test_shape_dtype_first_column_and_transitions(name, restart):
    indptr, indices, n = GRAPHS[name]()
    start = torch.arange(n).repeat(3)[: max(n, 50)]
    walks = random_walk(indptr, indices, start, 20, restart_p=restart, seed=11)
    assert walks.dtype == torch.int64 and tuple(walks.shape) == (start.numel(), 20) and walks.device.type == "cpu"
    assert torch.equal(walks[:, 0], start)
    check_transitions(indptr, indices, n, start.numpy(), walks, restart)
    n2v = node2vec_walk(indptr, indices, start, 20, p=0.5, q=2.0, seed=11)
    assert n2v.dtype == torch.int64 and tuple(n2v.shape) == (start.numel(), 20)
    assert torch.equal(n2v[:, 0], start)
    check_transitions(indptr, indices, n, start.numpy(), n2v, 0.0)


def test_sink_repeats_and_length_one_and_no_walkers():
    indptr, indices, n = path_with_sink()
    walks = random_walk(indptr, indices, torch.tensor([0, 5, 3]), 9, seed=0)
    assert walks[0].tolist() == [0, 1, 2, 3, 4, 5, 5, 5, 5]
    assert walks[1].tolist() == [5] * 9 and walks[2].tolist() == [3, 4, 5] + [5] * 6
    assert node2vec_walk(indptr, indices, torch.tensor([0]), 9, p=2.0, q=0.5, seed=0)[0].tolist() == [0, 1, 2, 3, 4, 5, 5, 5, 5]
    one = random_walk(indptr, indices, torch.tensor([2, 4]), 1, seed=0)
    assert one.tolist() == [[2], [4]]
    assert node2vec_walk(indptr, indices, torch.tensor([2, 4]), 1, seed=0).tolist() == [[2], [4]]
    empty = random_walk(indptr, indices, torch.empty(0, dtype=torch.long), 7, seed=0)
    assert tuple(empty.shape) == (0, 7) and empty.dtype == torch.int64
    assert tuple(node2vec_walk(indptr, indices, torch.empty(0, dtype=torch.long), 7, seed=0).shape) == (0, 7)


def test_restart_one_always_lands_on_a_neighbour_of_the_start():
    indptr, indices, n = random_with_isolated()
    start = torch.arange(300)
    walks = random_walk(indptr, indices, start, 12, restart_p=1.0, seed=3).numpy()
    ip, ix = indptr.numpy(), indices.numpy()
    for s in range(300):
        nb = set(ix[ip[s]:ip[s + 1]].tolist())
        if nb:
            assert set(walks[s, 1:].tolist()) <= nb
        else:
            assert (walks[s] == s).all()


def test_seed_determinism_and_independence_of_batching():
    indptr, indices, n = random_with_isolated()
    start = torch.arange(n).repeat(40)
    a = random_walk(indptr, indices, start, 16, restart_p=0.2, seed=123)
    assert torch.equal(a, random_walk(indptr, indices, start, 16, restart_p=0.2, seed=123))
    assert not torch.equal(a, random_walk(indptr, indices, start, 16, restart_p=0.2, seed=124))
    # walker w depends on (seed, w, start[w]) only: a prefix of the batch, or other walkers starting elsewhere, change nothing
    assert torch.equal(random_walk(indptr, indices, start[:777], 16, restart_p=0.2, seed=123), a[:777])
    other = start.clone()
    other[1::2] = 7
    assert torch.equal(random_walk(indptr, indices, other, 16, restart_p=0.2, seed=123)[0::2], a[0::2])
    b = node2vec_walk(indptr, indices, start, 16, p=0.25, q=4.0, seed=9)
    assert torch.equal(b, node2vec_walk(indptr, indices, start, 16, p=0.25, q=4.0, seed=9))
    assert torch.equal(node2vec_walk(indptr, indices, start[:777], 16, p=0.25, q=4.0, seed=9), b[:777])
    assert not torch.equal(b, node2vec_walk(indptr, indices, start, 16, p=0.25, q=4.0, seed=10))


def test_seed_none_follows_torch_manual_seed():
    indptr, indices, n = random_with_isolated()
    start = torch.arange(300)
    torch.manual_seed(77)
    a1, a2 = random_walk(indptr, indices, start, 10), random_walk(indptr, indices, start, 10)
    torch.manual_seed(77)
    b1, b2 = random_walk(indptr, indices, start, 10), random_walk(indptr, indices, start, 10)
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)
    torch.manual_seed(78)
    c1 = node2vec_walk(indptr, indices, start, 10, p=0.5, q=2.0)
    c2 = node2vec_walk(indptr, indices, start, 10, p=0.5, q=2.0)
    torch.manual_seed(78)
    assert torch.equal(c1, node2vec_walk(indptr, indices, start, 10, p=0.5, q=2.0)) and not torch.equal(c1, c2)


def test_result_does_not_depend_on_the_number_of_openmp_threads():
    code = r'''
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from cogdl_amd.operators import random_walk, node2vec_walk
rng = np.random.default_rng(1)
n = 2000
row = np.sort(rng.integers(0, n, 30000)); col = rng.integers(0, n, 30000)
indptr = np.zeros(n + 1, dtype=np.int64); np.cumsum(np.bincount(row, minlength=n), out=indptr[1:])
indptr, indices = torch.from_numpy(indptr), torch.from_numpy(col)
start = torch.arange(n).repeat(5)
a = random_walk(indptr, indices, start, 40, restart_p=0.1, seed=5)
b = node2vec_walk(indptr, indices, start, 40, p=0.25, q=4.0, seed=5)
print(hashlib.sha256(a.numpy().tobytes() + b.numpy().tobytes()).hexdigest())
'''
    digests = []
    for threads in ("1", "4"):
        out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=threads))
        assert out.returncode == 0, out.stderr[-2000:]
        digests.append(out.stdout.strip())
    assert digests[0] == digests[1] and len(digests[0]) == 64


# ---------------------------------------------------------------------------------------------------- distributions
def unequal_graph():
    """Directed, 1003 nodes: node 0 has degree 3, node 1 degree 1000, node 1002 none; the others 2 to 5."""
    n = 1003
    row, col = [0, 0, 0], [1, 2, 3]
    row += [1] * 1000
    col += list(range(2, 1002))
    row += [2, 2, 3, 3, 3, 3, 3]
    col += [0, 1, 0, 1, 2, 4, 1002]
    for v in range(4, 1002):
        row += [v, v]
        col += [0, 1 if v % 2 else 3]
    return csr_of(row, col, n) + (n,)


def transition_matrix(indptr, indices, n):
    ip, ix = indptr.numpy(), indices.numpy()
    p = np.zeros((n, n), dtype=np.float64)
    for v in range(n):
        nb = ix[ip[v]:ip[v + 1]]
        if nb.size == 0:
            p[v, v] = 1.0
        else:
            np.add.at(p[v], nb, 1.0 / nb.size)
    return p


def assert_chi_square(counts, prob, what):
    """counts over all cells, prob the exact law (zero outside its support, where no count may fall)."""
    counts, prob = np.asarray(counts, dtype=np.float64), np.asarray(prob, dtype=np.float64)
    support = prob > 0
    assert counts[~support].sum() == 0, "%s: samples outside the support" % what
    total = counts.sum()
    expected = prob[support] * total
    stat = float(((counts[support] - expected) ** 2 / expected).sum())
    bound = float(chi2.ppf(QUANTILE, int(support.sum()) - 1))
    print("%s: chi-square %.1f, bound %.1f (%d cells, %d samples)" % (what, stat, bound, int(support.sum()), int(total)))
    assert stat <= bound, "%s: chi-square %.1f above the 1 - 1e-6 quantile %.1f" % (what, stat, bound)


@pytest.mark.parametrize("node", [0, 1, 3])
def test_single_step_is_uniform_over_the_neighbours(node):
    indptr, indices, n = unequal_graph()
    start = torch.full((1_000_000,), node, dtype=torch.long)
    nxt = random_walk(indptr, indices, start, 2, seed=1000 + node)[:, 1]
    assert_chi_square(np.bincount(nxt.numpy(), minlength=n), transition_matrix(indptr, indices, n)[node],
                      "one step from node %d" % node)


@pytest.mark.parametrize("node", [0, 3])
def test_two_steps_with_restart_follow_the_exact_law(node):
    indptr, indices, n = unequal_graph()
    p = transition_matrix(indptr, indices, n)
    restart = 0.3
    first = p[node]
    law = (1.0 - restart) * (first @ p) + restart * first  # a restart lands on a neighbour of the start
    start = torch.full((1_000_000,), node, dtype=torch.long)
    walks = random_walk(indptr, indices, start, 3, restart_p=restart, seed=2000 + node)
    assert_chi_square(np.bincount(walks[:, 2].numpy(), minlength=n), law, "two steps from node %d, restart 0.3" % node)


def third_node_counts(walks, n):
    w = walks.numpy()
    sel = w[:, 1] == 1  # walkers start at 0: (t, v) = (0, 1)
    assert sel.sum() > 400_000
    return np.bincount(w[sel, 2], minlength=n)


def n2v_law(p, q):
    w = np.array([1.0 / p, 0.0, 1.0, 1.0 / q, 1.0 / q])
    return w / w.sum()


@pytest.mark.parametrize("p,q", [(0.25, 4.0), (4.0, 0.25), (1.0, 1.0)])
def test_node2vec_third_node_follows_the_exact_weights(p, q):
    indptr, indices, n = n2v_graph()
    start = torch.zeros(1_000_000, dtype=torch.long)
    walks, fallback = node2vec_walk(indptr, indices, start, 3, p=p, q=q, seed=31, return_fallback=True)
    assert_chi_square(third_node_counts(walks, n), n2v_law(p, q), "node2vec p=%g q=%g" % (p, q))
    assert fallback.dtype == torch.int32 and int(fallback.min()) >= 0 and int(fallback.max()) <= 1


def test_node2vec_exact_fallback_alone_carries_the_law(monkeypatch):
    indptr, indices, n = n2v_graph()
    start = torch.zeros(1_000_000, dtype=torch.long)
    monkeypatch.setattr(walk_mod, "NODE2VEC_TRIALS", 1)
    walks, fallback = node2vec_walk(indptr, indices, start, 3, p=0.25, q=4.0, seed=32, return_fallback=True)
    # at (t, v) = (0, 1) the one trial accepts with probability (4 + 1 + 1/4 + 1/4) / (4 * 4) = 0.34375, so the fallback
    # decides a fraction 0.65625 of those steps: binomial, sigma = 0.0007 at ~5e5 walkers; 0.005 is seven sigma
    at_v = walks[:, 1] == 1
    assert abs(float(fallback[at_v].double().mean()) - 0.65625) < 0.005
    assert_chi_square(third_node_counts(walks, n), n2v_law(0.25, 4.0), "node2vec p=0.25 q=4, one trial")
    w = walks.numpy()
    sel = (w[:, 1] == 1) & (fallback.numpy() == 1)
    assert_chi_square(np.bincount(w[sel, 2], minlength=n), n2v_law(0.25, 4.0), "node2vec, walkers decided by the fallback")


def test_node2vec_with_p_q_one_has_the_law_of_the_first_order_walk():
    indptr, indices, n = n2v_graph()
    start = torch.zeros(1_000_000, dtype=torch.long)
    a = third_node_counts(node2vec_walk(indptr, indices, start, 3, p=1.0, q=1.0, seed=41), n).astype(np.float64)
    b = third_node_counts(random_walk(indptr, indices, start, 3, seed=42), n).astype(np.float64)
    cells = (a + b) > 0
    ta, tb = a.sum(), b.sum()
    stat = float((((np.sqrt(tb / ta) * a - np.sqrt(ta / tb) * b) ** 2)[cells] / (a + b)[cells]).sum())  # homogeneity of two samples
    bound = float(chi2.ppf(QUANTILE, int(cells.sum()) - 1))
    print("node2vec(1, 1) vs random_walk: chi-square %.1f, bound %.1f" % (stat, bound))
    assert int(cells.sum()) == 4 and stat <= bound


def test_unsorted_rows_are_sorted_once_per_structure():
    indptr, indices, n = n2v_graph()
    shuffled = indices.clone()
    ip = indptr.tolist()
    for v in range(n):
        shuffled[ip[v]:ip[v + 1]] = indices[ip[v]:ip[v + 1]].flip(0)
    assert not torch.equal(shuffled, indices)
    start = torch.zeros(1000, dtype=torch.long)
    got = node2vec_walk(indptr, shuffled, start, 5, p=0.25, q=4.0, seed=5)
    assert torch.equal(got, node2vec_walk(indptr, indices, start, 5, p=0.25, q=4.0, seed=5))
    s1 = walk_mod.sorted_rows(indptr, shuffled)
    want = torch.cat([indices[ip[v]:ip[v + 1]].sort().values for v in range(n)])
    assert s1 is walk_mod.sorted_rows(indptr, shuffled) and torch.equal(s1, want)
    assert walk_mod.sorted_rows(indptr, want) is want  # sorted already: used as it is


# ---------------------------------------------------------------------------------------------------- errors
def test_argument_errors_raise_before_anything_runs():
    indptr, indices, n = n2v_graph()
    start = torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError):
        random_walk(indptr, indices, start, 0)
    with pytest.raises(ValueError):
        random_walk(indptr, indices, start, 5, restart_p=1.5)
    with pytest.raises(ValueError):
        random_walk(indptr, indices, start, 5, restart_p=-0.1)
    with pytest.raises(ValueError):
        node2vec_walk(indptr, indices, start, 5, p=0.0)
    with pytest.raises(ValueError):
        node2vec_walk(indptr, indices, start, 5, q=-1.0)
    with pytest.raises(ValueError):
        node2vec_walk(indptr, indices, start, 0)
    with pytest.raises(_lib.BackendError):
        random_walk(indptr.int(), indices, start, 5)
    with pytest.raises(_lib.BackendError):
        random_walk(indptr, indices.int(), start, 5)
    with pytest.raises(_lib.BackendError):
        random_walk(indptr, indices, start.int(), 5)
    with pytest.raises(_lib.BackendError):
        node2vec_walk(indptr, indices, start.float(), 5)
    with pytest.raises(_lib.BackendError):
        random_walk(indptr, indices, start.to("meta"), 5)  # mixed devices


def test_out_of_range_ids_raise():
    indptr, indices, n = n2v_graph()
    with pytest.raises(_lib.BackendError, match="start id"):
        random_walk(indptr, indices, torch.tensor([0, 5]), 4, seed=0)
    with pytest.raises(_lib.BackendError, match="start id"):
        node2vec_walk(indptr, indices, torch.tensor([-1]), 4, seed=0)
    bad = indices.clone()
    bad[:] = 99
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        random_walk(indptr, bad, torch.tensor([0, 1]), 4, seed=0)
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        node2vec_walk(indptr, bad, torch.tensor([0, 1]), 4, seed=0)
    with pytest.raises(_lib.BackendError, match="indptr"):
        random_walk(torch.tensor([0, 2, 400, 401, 402, 403]), indices, torch.tensor([1]), 4, seed=0)
    # the C entry points refuse bad sizes / pointers themselves
    assert _lib.host().cogdl_host_random_walk(None, None, 4, 4, None, 3, 5, 0.0, 1, None, None) == 1
    assert _lib.host().cogdl_host_node2vec_walk(None, None, 4, 4, None, 0, 5, 0.0, 1.0, 0, 1, None, None, None) == 1


# ---------------------------------------------------------------------------------------------------- RandomWalker
def test_random_walker_accepts_the_reference_graph_forms():
    rng = np.random.default_rng(2)
    n = 60
    row, col = rng.integers(0, n, 500), rng.integers(0, n, 500)
    ei = torch.from_numpy(np.stack([row, col]))
    a = RandomWalker(ei, num_nodes=n)
    b = RandomWalker()
    b.build_up((ei[0], ei[1]), n)
    m = sp.csr_matrix((np.ones(500), (row, col)), shape=(n, n))  # scipy sums duplicates and sorts the rows
    c = RandomWalker(m)
    assert np.array_equal(c.indptr.numpy(), m.indptr) and np.array_equal(c.indices.numpy(), m.indices)
    assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices)
    assert a.indptr.dtype == torch.int64 and a.indices.dtype == torch.int64
    ip = a.indptr.tolist()
    assert a.indptr[-1] == 500
    for v in range(n):
        assert sorted(set(a.indices[ip[v]:ip[v + 1]].tolist())) == m.indices[m.indptr[v]:m.indptr[v + 1]].tolist()
    d = RandomWalker(sp.coo_matrix((np.ones(500), (row, col)), shape=(n, n)))
    assert torch.equal(d.indptr, c.indptr) and torch.equal(d.indices, c.indices)
    b.build_up(ei[:, :10], n)  # a second build_up is a no-op, as in the reference
    assert torch.equal(a.indices, b.indices)
    for start in (torch.arange(20), list(range(20)), np.arange(20, dtype=np.int32)):
        out = a.walk(start, 7, restart_p=0.2, seed=4)
        assert isinstance(out, np.ndarray) and out.dtype == np.int64 and out.shape == (20, 7)
        assert np.array_equal(out, a.walk(torch.arange(20), 7, restart_p=0.2, parallel=False, seed=4))
    t = a.walk_tensor(torch.arange(20), 7, restart_p=0.2, seed=4)
    assert torch.is_tensor(t) and np.array_equal(t.numpy(), a.walk(torch.arange(20), 7, restart_p=0.2, seed=4))
    assert tuple(a.node2vec_walk(torch.arange(20), 7, p=0.5, q=2.0, seed=4).shape) == (20, 7)
    assert RandomWalker(ei).indptr.numel() == int(ei.max()) + 2  # num_nodes inferred


INSTALL_SCRIPT = r'''
import os, shutil, sys, tempfile
ROOT, REF = sys.argv[1], sys.argv[2]
scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")          # the reference writes into its own tree when imported
shutil.copytree(os.path.join(REF, "cogdl"), os.path.join(scratch, "cogdl"))
sys.dont_write_bytecode = True
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
import numpy as np, torch
import cogdl_amd
cogdl_amd.install()
import cogdl
import cogdl.utils, cogdl.utils.sampling, cogdl.data.data, cogdl.data.sampler
mods = (cogdl.utils.sampling, cogdl.utils, cogdl.data.data, cogdl.data.sampler)
cogdl_amd.install()
for m in mods:
    assert m.RandomWalker.__module__ == "cogdl.utils.sampling", (m.__name__, "plain install() rebound RandomWalker")
orig = cogdl.utils.sampling.RandomWalker
cogdl_amd.install(random_walk=True)
for m in mods:
    assert m.RandomWalker.__module__ == "cogdl_amd.random_walk_compat", m.__name__
cogdl_amd.install(random_walk=True)                            # idempotent: the original is not lost

from cogdl.data import Graph
n = 200
ei = torch.randint(0, n, (2, 3000), generator=torch.Generator().manual_seed(0))
g = Graph(edge_index=ei, x=torch.randn(n, 4))
torch.manual_seed(3)
walks = g.random_walk(list(range(50)), 8)
assert type(g._adj.__walker__).__module__ == "cogdl_amd.random_walk_compat"
assert isinstance(walks, np.ndarray) and walks.dtype == np.int64 and walks.shape == (50, 8)
assert (walks[:, 0] == np.arange(50)).all()
keys = set((ei[0] * n + ei[1]).tolist())
deg = torch.bincount(ei[0], minlength=n)
for a, b in zip(walks[:, :-1].ravel().tolist(), walks[:, 1:].ravel().tolist()):
    assert a * n + b in keys or (a == b and deg[a] == 0), (a, b)
torch.manual_seed(3)
assert np.array_equal(walks, g.random_walk_with_restart(list(range(50)), 8))

from cogdl.data.sampler import UnsupNeighborSamplerDataset
class DS:                                                      # what the sampler reads of a dataset: .data
    data = g
ds = UnsupNeighborSamplerDataset(DS(), sizes=[3, 3], batch_size=16)
assert type(ds.random_walker).__module__ == "cogdl_amd.random_walk_compat"
batch = ds[0]
assert ds.random_walker.indptr is not None and ds.random_walker.indptr.dtype == torch.int64
assert batch is not None

cogdl_amd.uninstall()
for m in mods:
    assert m.RandomWalker is orig, (m.__name__, "uninstall() did not restore RandomWalker")
print("ok")
'''


def test_install_flag_rebinds_random_walker_and_uninstall_restores_it():
    if not REF or not os.path.isdir(os.path.join(REF, "cogdl")):
        pytest.skip("the reference package is not staged (oracle/_ref/pkg) and COGDL_REFERENCE is not set")
    out = subprocess.run([sys.executable, "-c", INSTALL_SCRIPT, ROOT, REF], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert out.stdout.strip().endswith("ok")
