"""Shared cases of the gen_aggregate tests (tests/test_genaggr_cpu.py, tests/test_genaggr_gpu.py) and of
tools/genconv_bench.py: one small graph, the inputs per width, the float64 oracle and the acceptance rule.

Graph: N = 300 nodes, built with numpy, edges in a shuffled (caller's) order.  Destinations 0 .. 8 have exactly 0, 1, 2, 63, 64,
65, 128, 129 and 1000 edges: they straddle the lane-group chunk (64) and the long-row threshold of a small edge list (128), and
the hub spans several chunks of the chunk-parallel path.  Destinations 20 .. 259 share 2000 random edges, 260 .. 299 receive
nothing.  Source 10 sends 400 edges (a long row of the backward's source-sorted view), sources 280 .. 299 send nothing.  The
list holds duplicate edges and self-loops.

Oracle: the torch composition (gather, relu + eps, per-row softmax with the row maximum subtracted, scatter_add_) in float64 on
the float32 inputs, gradients from its autograd.  Rule, per compared tensor:

    err_new <= 4 * err_ref + 8 * eps32 * max|oracle|

err_ref = the error of the SAME composition in float32 on the CPU under torch's deterministic mode against the oracle, err_new
= the error of the result under test (max |. - oracle|).  Factor 4: the online softmax spends at most about three roundings
per edge where the composition spends one or two, and the device expf may be an ulp looser than libm's.  The floor: some cases
make the float32 composition exact."""
import contextlib
import functools

import numpy as np
import torch

N = 300
WIDTHS = (1, 7, 64, 65, 128)
DEGREES = {0: 0, 1: 1, 2: 2, 3: 63, 4: 64, 5: 65, 6: 128, 7: 129, 8: 1000}
HUB_SOURCE, HUB_SOURCE_EDGES = 10, 400
EPS = 1e-7
EPS32 = float(np.finfo(np.float32).eps)


@contextlib.contextmanager
def edge_order():
    """torch's deterministic mode: CPU scatter_add_ and the autograd of x[col] then run as the sequential loop over the edges."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was)


@functools.lru_cache(maxsize=None)
def graph():
    """(row, col) int64, the caller's (shuffled) edge order."""
    rng = np.random.default_rng(7)
    rows, cols = [], []
    for v, deg in DEGREES.items():
        rows.append(np.full(deg, v))
        cols.append(rng.integers(0, 280, deg))
    rows.append(rng.integers(20, 260, 2000))
    cols.append(rng.integers(0, 280, 2000))
    rows.append(rng.integers(20, 260, HUB_SOURCE_EDGES))
    cols.append(np.full(HUB_SOURCE_EDGES, HUB_SOURCE))
    loops = np.arange(30, 60)  # self-loops ...
    rows.append(loops)
    cols.append(loops)
    row, col = np.concatenate(rows), np.concatenate(cols)
    row, col = np.concatenate([row, row[1500:1540]]), np.concatenate([col, col[1500:1540]])  # ... and duplicates
    order = rng.permutation(row.size)
    row, col = torch.from_numpy(row[order]).long(), torch.from_numpy(col[order]).long()
    deg = torch.bincount(row, minlength=N)
    assert all(int(deg[v]) == d for v, d in DEGREES.items()) and int(deg[260:].sum()) == 0
    out_deg = torch.bincount(col, minlength=N)
    assert int(out_deg[HUB_SOURCE]) >= HUB_SOURCE_EDGES and int(out_deg[280:].sum()) == 0
    return row, col


@functools.lru_cache(maxsize=None)
def inputs(width, with_eterm, scale=1.0):
    """x [N, F] (negative entries), eterm [E, F] or None (x + eterm is exactly 0 at 40 places: the relu mask), G [N, F]."""
    row, col = graph()
    gen = torch.Generator().manual_seed(1000 * width + int(with_eterm))
    x = torch.randn(N, width, generator=gen) * scale
    assert bool((x < 0).any())
    eterm = None
    if with_eterm:
        eterm = torch.randn(row.numel(), width, generator=gen) * (0.5 * scale)
        at = torch.randint(0, row.numel(), (40,), generator=gen)
        f = torch.randint(0, width, (40,), generator=gen)
        eterm[at, f] = -x[col[at], f]
        assert int(((x[col] + eterm) == 0).sum()) >= 40
    return x, eterm, torch.randn(N, width, generator=gen)


def composition(x, row, col, eterm, aggr, beta, eps, num_nodes):
    pre = x[col]
    if eterm is not None:
        pre = pre + eterm
    m = torch.relu(pre) + eps
    idx = row.unsqueeze(-1).expand(-1, m.shape[1])
    zeros = torch.zeros(num_nodes, m.shape[1], dtype=m.dtype)
    if aggr == "softmax":
        z = m if beta is None else beta * m
        top = torch.full_like(zeros, float("-inf")).scatter_reduce(0, idx, z.detach(), "amax", include_self=True)
        p = torch.exp(z - top[row])
        h = m * (p / zeros.scatter_add(0, idx, p)[row])
    elif aggr == "mean":
        inv = torch.bincount(row, minlength=num_nodes).to(m.dtype).pow(-1)
        inv[torch.isinf(inv)] = 0
        h = m * inv[row].unsqueeze(-1)
    else:
        h = m
    return zeros.scatter_add(0, idx, h)


def run(fn, x, eterm, beta, G, learn_beta, device="cpu", dtype=torch.float32):
    """fn(x, eterm, beta) -> out; returns {"out", "g_x", "g_eterm", "g_beta"} (absent inputs left out) on the CPU."""
    xa = x.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    ta = None if eterm is None else eterm.detach().clone().to(device=device, dtype=dtype).requires_grad_()
    ba = beta
    if learn_beta:
        ba = torch.tensor([beta], dtype=torch.float32).to(device=device, dtype=dtype).requires_grad_()  # (the float32 value)
    out = fn(xa, ta, ba)
    out.backward(G.to(device=device, dtype=dtype))
    got = {"out": out.detach(), "g_x": xa.grad}
    if ta is not None:
        got["g_eterm"] = ta.grad
    if learn_beta:
        got["g_beta"] = ba.grad
    return {k: v.cpu() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def reference(width, with_eterm, aggr, beta=None, learn_beta=False, scale=1.0):
    """(oracle, ref32): the composition in float64 and in float32 (CPU, deterministic mode) on the same float32 inputs."""
    row, col = graph()
    x, eterm, G = inputs(width, with_eterm, scale)
    fn = lambda xa, ta, ba: composition(xa, row, col, ta, aggr, ba, EPS, N)
    with edge_order():
        oracle = run(fn, x, eterm, beta, G, learn_beta, dtype=torch.float64)
        ref32 = run(fn, x, eterm, beta, G, learn_beta)
    return oracle, ref32


def errors(got, oracle, ref32):
    """{name: (err_new, err_ref, bound)}"""
    res = {}
    for name, want in oracle.items():
        err_ref = float((ref32[name].double() - want).abs().max())
        err_new = float((got[name].double() - want).abs().max())
        res[name] = (err_new, err_ref, 4 * err_ref + 8 * EPS32 * float(want.abs().max()))
    return res


def check(label, got, oracle, ref32):
    """Print both errors of every tensor, then assert the rule (and that nothing is nan / inf)."""
    res = errors(got, oracle, ref32)
    bad = []
    for name, (err_new, err_ref, bound) in res.items():
        line = "%s %-8s err_new %.3e  err_ref %.3e  bound %.3e" % (label, name, err_new, err_ref, bound)
        print(line)
        if not (bool(torch.isfinite(got[name]).all()) and err_new <= bound):
            bad.append(line)
    assert not bad, bad
    return res
