"""Edge-sampled skip-gram training (LINE, orders 1 and 2) on the host twin (csrc/host_line.cpp, the law of csrc/line_law.h), no
GPU: a float32 numpy replay of the serial mode's trace reproduces both tables; the draws follow their laws (edge weights,
orientation, noise distribution, learning-rate schedule); determinism; flags and argument errors; embedding quality on the
planted-partition graph against the reference's own LINE.

Distribution tests are Pearson chi-square tests at the level tests/test_sgns_host.py uses (the 1 - 1e-6 quantile); seeds are
fixed, so the outcome is deterministic."""
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

from _line_cases import (ALPHA, GRID, QUALITY, SAMPLES_PER_NODE, ZERO_EDGE, graph, grid_id, grid_init, grid_run, quality_edges,
                         reference_purity, twin_purity)
from test_sgns_host import ROOT, assert_chi_square, neighbour_purity


def replay(trace, emb, ctx):
    """The trace's arithmetic again in float32 numpy (dot product in numpy's order).  Per sample: x = emb[u] read once, err = 0;
    per record f = <x, T[t]>, sig = 1 / 0 outside (-6, 6) and EXP_TABLE[int((f + 6) * (1000 / 12))] inside, g = (label - sig) * lr,
    err += g * T[t], T[t] += g * x; err is added to emb[u] when the sample ends.  T is ctx, or emb where ctx is None (order 1).
    -> (emb, ctx, number of records with |f| >= 6)."""
    table = sgns_mod.exp_table().numpy()
    emb = emb.numpy().copy()
    tgt = emb if ctx is None else ctx.numpy().copy()
    scale = np.float32(1000.0) / np.float32(12.0)
    cur, x, err, saturated = None, None, None, 0
    for s, u, t, label, lr in trace.numpy():
        u, t = int(u), int(t)
        if cur is None or cur[0] != s:
            if cur is not None:
                emb[cur[1]] = emb[cur[1]] + err
            cur, x, err = (s, u), emb[u].copy(), np.zeros(emb.shape[1], dtype=np.float32)
        assert u == cur[1]
        f = np.float32(np.dot(x, tgt[t]))
        if f >= 6.0:
            sig, saturated = np.float32(1.0), saturated + 1
        elif f <= -6.0:
            sig, saturated = np.float32(0.0), saturated + 1
        else:
            sig = table[min(999, int((f + np.float32(6.0)) * scale))]
        g = np.float32((np.float32(label) - sig) * np.float32(lr))
        err = err + g * tgt[t]
        tgt[t] = tgt[t] + g * x
    if cur is not None:
        emb[cur[1]] = emb[cur[1]] + err
    return emb, (None if ctx is None else tgt), saturated


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_numpy_replay_of_the_trace_reproduces_both_tables(case):
    name, s, d, k, order = case
    init = grid_init(case)
    out = grid_run(case, init=init, trace=s * (k + 1))
    trace = out[-1]
    emb0, ctx0 = (init, None) if order == 1 else init
    r_emb, r_ctx, saturated = replay(trace, emb0, ctx0)
    np.testing.assert_allclose(out[0].numpy(), r_emb, rtol=1e-5, atol=1e-8)
    if order == 2:
        np.testing.assert_allclose(out[1].numpy(), r_ctx, rtol=1e-5, atol=1e-8)
        assert not torch.equal(out[1], ctx0)
    rec = trace.numpy()
    assert trace.shape[0] >= s and not torch.equal(out[0], emb0)  # (the positive of every sample is applied)
    assert (rec[:, 3] == 1).sum() == s and rec[0, 3] == 1 and (np.diff(rec[:, 0]) >= 0).all()
    if d == 1 and s == 1000:
        assert saturated > 0  # (the scaled init reaches |f| >= 6: the update applies there with the sigmoid at 0 or 1)
    if name == "triangle" and s == 1000:
        neg = rec[rec[:, 3] == 0]
        assert len(neg) < k * s and not (neg[:, 1] == neg[:, 2]).any()  # negatives equal to an endpoint are skipped
        assert (rec[:, 1] == rec[:, 2]).any()  # the self-loop: a positive target that is the input row
        if k == 16:  # three nodes, sixteen negatives: a sample repeats a target
            pairs = neg[:, 0] * 4 + neg[:, 2]
            assert len(np.unique(pairs)) < len(pairs)


# -------------------------------------------------------------------------------------------------------------- laws
def _trace(name, samples, k=5, seed=21, order=2, dim=4):
    edges, v, w = graph(name)
    out = line_train(edges, v, dim, order, samples, negative=k, alpha=0.025, edge_weight=w, seed=seed, workers=1,
                     trace=samples * (k + 1))
    return edges.numpy(), v, w, out[-1].numpy()


def test_edge_frequencies_follow_the_weights_and_orientation_is_fair():
    samples = 200000
    edges, v, w, rec = _trace("weighted", samples, k=1)
    pos = rec[rec[:, 3] == 1]
    assert len(pos) == samples
    # an undirected pair can occur in several table rows: cells are the unordered pairs
    key = np.minimum(edges[:, 0], edges[:, 1]) * v + np.maximum(edges[:, 0], edges[:, 1])
    cells, cell_of = np.unique(key, return_inverse=True)
    law = np.bincount(cell_of, weights=w.numpy(), minlength=len(cells))
    law = law / law.sum()
    u, t = pos[:, 1].astype(np.int64), pos[:, 2].astype(np.int64)
    got = np.searchsorted(cells, np.minimum(u, t) * v + np.maximum(u, t))
    assert (cells[np.minimum(got, len(cells) - 1)] == np.minimum(u, t) * v + np.maximum(u, t)).all()  # every sample is an edge
    assert_chi_square(np.bincount(got, minlength=len(cells)), law, "edge frequencies")
    # the zero-weight edge: its pair occurs in no other row, and is never drawn
    zero = key[ZERO_EDGE]
    assert (key == zero).sum() == 1 and w[ZERO_EDGE] == 0
    assert not (np.minimum(u, t) * v + np.maximum(u, t) == zero).any()
    # orientation: over the edges with two distinct endpoints, u is the table's first endpoint half of the time
    first = dict()
    for a, b in edges:
        first.setdefault((min(a, b), max(a, b)), set()).add(int(a))
    one_way = np.array([a != b and len(first[(min(a, b), max(a, b))]) == 1 for a, b in zip(u, t)])
    as_listed = np.array([int(a) in first[(min(a, b), max(a, b))] for a, b in zip(u[one_way], t[one_way])])
    assert one_way.sum() > samples // 2
    assert_chi_square([as_listed.sum(), (~as_listed).sum()], [0.5, 0.5], "orientation")


def test_unit_weight_edges_are_uniform():
    samples = 100000
    edges, v, w, rec = _trace("random", samples, k=1)
    pos = rec[rec[:, 3] == 1]
    key = np.minimum(edges[:, 0], edges[:, 1]) * v + np.maximum(edges[:, 0], edges[:, 1])
    cells, cell_of = np.unique(key, return_inverse=True)
    law = np.bincount(cell_of, minlength=len(cells)) / len(key)
    u, t = pos[:, 1].astype(np.int64), pos[:, 2].astype(np.int64)
    got = np.searchsorted(cells, np.minimum(u, t) * v + np.maximum(u, t))
    assert_chi_square(np.bincount(got, minlength=len(cells)), law, "unit-weight edge frequencies")


def test_negatives_follow_degree_to_the_three_quarters():
    """Each sample draws K negatives from the quantised noise table and drops those equal to u or v, so over all draws the
    cells are the ids plus one cell for the dropped draws."""
    samples, k = 40000, 5
    edges, v, w, rec = _trace("weighted", samples, k=k)
    deg = line_mod.weighted_degree(torch.from_numpy(edges), v, w)
    assert deg.max() > 8 * deg[deg > 0].min()
    cum = sgns_mod.build_tables(deg, 0, 0.75)[1].numpy()
    noise = np.diff(np.concatenate([[0], cum])) / float(cum[-1])
    np.testing.assert_allclose(noise, deg ** 0.75 / (deg ** 0.75).sum(), atol=1e-8)
    pos, neg = rec[rec[:, 3] == 1], rec[rec[:, 3] == 0]
    assert len(pos) == samples and not (neg[:, 1] == neg[:, 2]).any()
    u, t = pos[:, 1].astype(np.int64), pos[:, 2].astype(np.int64)
    v_of = np.zeros(samples, dtype=np.int64)
    v_of[pos[:, 0].astype(np.int64)] = t
    assert not (v_of[neg[:, 0].astype(np.int64)] == neg[:, 2]).any()
    # expected: node i is available to a sample unless it is u or v
    blocked = np.bincount(u, minlength=v) + np.bincount(t[t != u], minlength=v)
    draws = k * samples
    observed = np.append(np.bincount(neg[:, 2].astype(np.int64), minlength=v), draws - len(neg))
    law = np.append(noise * (samples - blocked), (noise * blocked).sum()) * k / draws
    assert law.sum() == pytest.approx(1.0, abs=1e-9)
    assert_chi_square(observed, law, "negatives")


def test_learning_rate_of_the_first_and_last_sample():
    samples, alpha = 977, 0.03
    edges, v, w = graph("random")
    out = line_train(edges, v, 4, 1, samples, negative=1, alpha=alpha, seed=1, workers=1, trace=samples * 2)
    rec = out[-1].numpy()
    assert rec[0, 0] == 0 and rec[-1, 0] == samples - 1
    assert rec[0, 4] == float(np.float32(alpha))
    assert rec[-1, 4] == float(np.float32(alpha * max(1.0 - (samples - 1) / samples, 1e-4)))
    lr = rec[rec[:, 3] == 1][:, 4]
    assert (np.diff(lr) < 0).all()
    # the floor: 1e-4 * alpha
    out = line_train(edges, v, 4, 1, 20001, negative=1, alpha=alpha, seed=1, workers=1, trace=20001 * 2)
    assert out[-1].numpy()[-1, 4] == float(np.float32(alpha * 1e-4))


# ------------------------------------------------------------------------------------------------------ determinism
def test_same_seed_same_result_and_seed_none_follows_torch_manual_seed():
    case = ("random", 1000, 64, 5, 2)
    a, b, c = grid_run(case, seed=9), grid_run(case, seed=9), grid_run(case, seed=10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    edges, v, _ = graph("random")
    torch.manual_seed(77)
    d1, d2 = line_train(edges, v, 8, 1, 500, workers=1), line_train(edges, v, 8, 1, 500, workers=1)
    torch.manual_seed(77)
    e1, e2 = line_train(edges, v, 8, 1, 500, workers=1), line_train(edges, v, 8, 1, 500, workers=1)
    assert torch.equal(d1, e1) and torch.equal(d2, e2) and not torch.equal(d1, d2)


def test_serial_result_does_not_depend_on_the_number_of_openmp_threads():
    code = r'''
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import torch
from cogdl_amd.operators import line_train
edges = torch.randint(0, 300, (1500, 2), generator=torch.Generator().manual_seed(2))
a, b = line_train(edges, 300, 24, 2, 5000, seed=5, workers=1)
print(hashlib.sha256(a.numpy().tobytes() + b.numpy().tobytes()).hexdigest())
'''
    digests = []
    for threads in ("1", "4"):
        out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS=threads))
        assert out.returncode == 0, out.stderr[-2000:]
        digests.append(out.stdout.strip())
    assert digests[0] == digests[1] and len(digests[0]) == 64


def test_parallel_mode_trains_and_init_is_not_modified():
    case = ("weighted", 1000, 65, 16, 2)
    init = grid_init(case)
    keep = init[0].clone(), init[1].clone()
    for workers in (1, 4):
        a = grid_run(case, init=init, workers=workers)
        assert torch.equal(init[0], keep[0]) and torch.equal(init[1], keep[1])
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all() and not torch.equal(a[0], keep[0])
    single = grid_init(("random", 1000, 7, 5, 1))
    kept = single.clone()
    b = grid_run(("random", 1000, 7, 5, 1), init=single)
    assert torch.equal(single, kept) and not torch.equal(b, kept)


def test_default_tables_are_the_law_s_initialisation_and_samples_0_changes_nothing():
    edges, v, _ = graph("random")
    emb, ctx = line_train(edges, v, 48, 2, 0, seed=5)
    want = sgns_mod.init_tables(v, 48, 5, "cpu")
    assert torch.equal(emb, want[0]) and float(ctx.abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------- errors
def test_argument_errors_raise_before_anything_runs():
    edges, v, _ = graph("triangle")
    base = dict(edges=edges, num_nodes=v, dim=8, order=1, samples=10, seed=1)
    for kw in (dict(dim=0), dict(dim=513), dict(order=0), dict(order=3), dict(samples=-1), dict(negative=0), dict(negative=17),
               dict(alpha=0.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(workers=-1), dict(num_nodes=0),
               dict(edges=edges.int()), dict(edges=edges[:, 0]), dict(edges=edges[:0]), dict(edges=torch.zeros((4, 3), dtype=torch.long)),
               dict(edge_weight=torch.ones(3)), dict(edge_weight=torch.tensor([1.0, -1.0, 1.0, 1.0])), dict(edge_weight=torch.zeros(4)),
               dict(edge_weight=torch.tensor([1.0, float("nan"), 1.0, 1.0])), dict(node_weight=torch.ones(2)),
               dict(init=torch.zeros(3, 9)), dict(init=(torch.zeros(3, 8), torch.zeros(3, 8))), dict(order=2, init=torch.zeros(3, 8)),
               dict(workers=0, trace=10), dict(tables=(None, torch.zeros(2, dtype=torch.long)))):
        with pytest.raises(ValueError):
            line_train(**dict(base, **kw))
    with pytest.raises(ValueError):
        line_train(workers=1, trace=1, **base)  # a trace buffer that is too small


def test_flags_raise_and_leave_the_tables_untouched():
    edges, v, w = graph("weighted")
    m = edges.shape[0]
    init = sgns_mod.init_tables(v, 8, 1, "cpu")
    emb, ctx = init[0].clone(), init[1].clone()
    lib = _lib.host()
    ncum = sgns_mod._u32(sgns_mod.build_tables(line_mod.weighted_degree(edges, v, w), 0, 0.75)[1], "cpu")
    ecum = line_mod.edge_table(w)
    table = sgns_mod.exp_table()
    flags = torch.zeros(1, dtype=torch.int32)

    def train(e, ec, nc, order=2, workers=1):
        eu, ev = e[:, 0].contiguous(), e[:, 1].contiguous()
        return lib.cogdl_host_line_train(_lib.ptr(eu), _lib.ptr(ev), _lib.ptr(ec), m, v, _lib.ptr(nc), _lib.ptr(table), 8, 3, order, 500,
                                         0.025, 1, workers, _lib.ptr(emb), _lib.ptr(ctx), _lib.ptr(flags), None, 0, None)

    bad = edges.clone()
    bad[5, 1] = v
    assert train(bad, ecum, ncum) == 0 and int(flags) == 1
    bad[5, 1] = -1
    assert train(bad, ecum, ncum, workers=0) == 0 and int(flags) == 1
    back = ncum.clone()
    back[100] = back[99] - 1
    assert train(edges, ecum, back) == 0 and int(flags) == 2
    assert train(edges, ecum, torch.zeros(v, dtype=torch.int32)) == 0 and int(flags) == 2
    for spoil in ((10, int(ecum[9]) - 1), (0, -1), (m - 1, 2 ** 52 + 1)):
        ebad = ecum.clone()
        ebad[spoil[0]] = spoil[1]
        assert train(edges, ebad, ncum, order=1) == 0 and int(flags) == 4
    assert train(edges, torch.zeros(m, dtype=torch.long), ncum) == 0 and int(flags) == 4
    ebad = ecum.clone()
    ebad[10] = int(ecum[9]) - 1
    assert train(bad, ebad, back) == 0 and int(flags) == 7
    assert torch.equal(emb, init[0]) and torch.equal(ctx, init[1])
    assert train(edges, ecum, ncum) == 0 and int(flags) == 0 and not torch.equal(emb, init[0]) and not torch.equal(ctx, init[1])
    # invalid and out-of-range arguments are refused by the shared check
    eu, ev = edges[:, 0].contiguous(), edges[:, 1].contiguous()
    for d, k, order, s, alpha, want in ((0, 3, 1, 5, 0.025, 1), (8, 3, 3, 5, 0.025, 1), (8, 3, 1, -1, 0.025, 1), (8, 3, 1, 5, 0.0, 1),
                                        (513, 3, 1, 5, 0.025, 2), (8, 17, 1, 5, 0.025, 2)):
        rc = lib.cogdl_host_line_train(_lib.ptr(eu), _lib.ptr(ev), None, m, v, _lib.ptr(ncum), _lib.ptr(table), d, k, order, s, alpha, 1, 1,
                                       _lib.ptr(emb), _lib.ptr(ctx), _lib.ptr(flags), None, 0, None)
        assert rc == want
    # through the operator
    with pytest.raises(_lib.BackendError, match="outside"):
        line_train(bad, v, 8, 1, 100, seed=1)
    with pytest.raises(_lib.BackendError, match="noise table"):
        line_train(edges, v, 8, 1, 100, seed=1, tables=(None, torch.zeros(v, dtype=torch.long)))
    with pytest.raises(_lib.BackendError, match="edge table"):
        line_train(edges, v, 8, 1, 100, seed=1, tables=(torch.zeros(m, dtype=torch.long), sgns_mod.build_tables(np.ones(v), 0, 0.75)[1]))


def test_edge_table_is_the_documented_quantisation():
    w = np.array([0.5, 0.0, 3.0, 1.0, 0.5])
    ecum = line_mod.edge_table(w).numpy()
    assert ecum.dtype == np.int64 and ecum[-1] == 2 ** 52 and ecum[0] == ecum[1] == round(2 ** 52 / 10)
    assert np.array_equal(ecum, np.round(np.cumsum(w) / 5.0 * 2.0 ** 52).astype(np.int64))
    deg = line_mod.weighted_degree(torch.tensor([[0, 1], [1, 2], [2, 2]]), 4, np.array([0.5, 1.0, 3.0]))
    assert np.array_equal(deg, [0.5, 1.5, 7.0, 0.0])  # the self-loop counts twice


# ---------------------------------------------------------------------------------------------------------- quality
def test_undirected_edge_table_keeps_one_entry_per_pair_and_the_last_weight():
    row = torch.tensor([0, 1, 2, 1, 3, 3, 0])
    col = torch.tensor([1, 0, 1, 2, 3, 3, 1])
    w = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    edges, weight = embedding.undirected_edges(row, col, 4, w)
    assert edges.tolist() == [[0, 1], [1, 2], [3, 3]] and weight.tolist() == [7.0, 4.0, 6.0] and weight.dtype == torch.float64
    assert embedding.undirected_edges(row, col, 4)[1] is None


@pytest.mark.parametrize("order", [1, 2, 3])
def test_serial_twin_embeds_no_worse_than_the_reference(order):
    """dim 32 (order 3: width 64), negative 5, alpha 0.025, 1600 samples per node.  The bar is the purity of the reference's
    own LINE on this graph (tests/golden/line_reference.json) minus 0.05, the margin test_sgns_gpu.py grants."""
    _, n, community = quality_edges()
    assert SAMPLES_PER_NODE == 1600 and QUALITY == dict(dim=32, negative=5, alpha=0.025)
    rand = neighbour_purity(torch.randn(n, 32, generator=torch.Generator().manual_seed(0)), community)
    got, ref = twin_purity(order), reference_purity()[order]
    print("neighbour purity, order %d: serial twin %.4f, reference %.4f, random vectors %.4f" % (order, got, ref, rand))
    assert rand < 0.1
    assert got >= ref - 0.05


def test_embedding_line_shapes_and_normalised_rows():
    edges, v, _ = graph("random")
    indptr = torch.zeros(v + 1, dtype=torch.long)
    order_ = torch.argsort(edges[:, 0], stable=True)
    torch.cumsum(torch.bincount(edges[:, 0], minlength=v), 0, out=indptr[1:])
    csr = (indptr, edges[order_, 1].contiguous())
    for order, dim, width in ((1, 9, 9), (2, 9, 9), (3, 9, 8)):
        emb = embedding.line(csr, dim=dim, walk_length=2, walk_num=2, order=order, seed=3, workers=1)
        assert emb.dtype == torch.float32 and tuple(emb.shape) == (v, width)
        for half in ((emb[:, :4], emb[:, 4:]) if order == 3 else (emb,)):  # (every row is non-zero from the initialisation on)
            assert torch.allclose(half.norm(dim=1), torch.ones(v), atol=1e-5)
    with pytest.raises(ValueError):
        embedding.line(csr, dim=1, order=3)
    with pytest.raises(ValueError):
        embedding.line(csr, dim=8, order=4)
    zero = embedding._unit_rows(torch.tensor([[0.0, 0.0], [3.0, 4.0]]))
    assert zero.tolist() == [[0.0, 0.0], [0.6000000238418579, 0.800000011920929]]
