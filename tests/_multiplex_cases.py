"""Shared cases of the multiplex_embed tests (test_multiplex_cpu.py, test_multiplex_gpu.py): inputs from a seeded generator, and
for each case the composition (cogdl_amd.operators.multiplex.composition, the reference's arithmetic) in float64 -- the oracle --
and in float32, both on the CPU, computed once.  N = 50 unless a case says otherwise.

The accuracy rule is the project's (tests/_gen_cases.py: errors):  err_new <= 4 err_ref + 8 eps32 max|oracle|  per tensor, where
err_ref is the float32 composition's error against the same oracle."""
import functools

import numpy as np
import torch

import _offset as O
from cogdl_amd.operators.multiplex import composition

EPS32 = float(np.finfo(np.float32).eps)
N = 50
NAMES = ("out", "g_node", "g_type", "g_trans", "g_w1", "g_w2")

# name -> (D, U, A, T, S, B): every value of D in {1, 7, 64, 200, 257}, U in {1, 3, 10, 33}, A in {1, 20}, T in {1, 2, 5},
# S in {1, 10}, B in {1, 7, 300} occurs
GRID = {
    "d1_u1_a1_t1_s1_b1": (1, 1, 1, 1, 1, 1),
    "d7_u3_a20_t2_s10_b7": (7, 3, 20, 2, 10, 7),
    "d64_u10_a20_t5_s10_b300": (64, 10, 20, 5, 10, 300),
    "d200_u10_a20_t2_s10_b300": (200, 10, 20, 2, 10, 300),
    "d257_u33_a1_t5_s1_b7": (257, 33, 1, 5, 1, 7),
    "d200_u33_a20_t1_s10_b1": (200, 33, 20, 1, 10, 1),
    "d64_u1_a20_t5_s1_b300": (64, 1, 20, 5, 1, 300),
    "d7_u10_a1_t2_s1_b1": (7, 10, 1, 2, 1, 1),
    "d257_u3_a20_t1_s10_b300": (257, 3, 20, 1, 10, 300),
    "d1_u33_a20_t2_s10_b7": (1, 33, 20, 2, 10, 7),
    "d200_u10_a20_t5_s10_b7": (200, 10, 20, 5, 10, 7),
    "d64_u3_a1_t1_s1_b7": (64, 3, 1, 1, 1, 7),
}
# further cases: name -> ((D, U, A, T, S, B), kind)
SPECIAL = {
    "skewed": ((64, 10, 20, 5, 10, 300), "skewed"),       # one input 200 times, nodes never named, type 3 absent
    "hub": ((64, 10, 20, 2, 10, 300), "hub"),             # node 7 fills every slot of type 1: a list of 3000 > 512
    "int32_ids": ((64, 10, 20, 5, 10, 7), "int32"),
    "offset_tables": ((200, 10, 20, 2, 10, 7), "offset"),  # node_emb 1 float, type_emb 2 floats past a 16-byte boundary
    "zero_norm": ((64, 10, 20, 5, 10, 7), "zero_norm"),   # sample 0: node_emb[x] = 0 and trans_w[t] = 0
    "large_e": ((64, 10, 20, 5, 10, 7), "large_e"),       # att_w2 scaled: 200 <= max|e| <= 2000
    "saturated": ((64, 10, 20, 5, 10, 7), "saturated"),   # att_w1 scaled: every tanh is +-1 exactly
}
CASES = tuple(GRID) + tuple(SPECIAL)
SKEW_NODE, SKEW_ABSENT_TYPE, HUB_NODE, HUB_TYPE = 11, 3, 7, 1
USED_NODES = 40  # skewed: inputs come from [0, 20), neighbours from [0, 40): nodes 40 .. 49 are in no list


def _seed(name):
    return 1000 + CASES.index(name)


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict of CPU tensors: the five float32 operands, neigh / inputs / types (int64, or int32 for the int32 case), G."""
    (d, u, a, t, s, b), kind = SPECIAL[name] if name in SPECIAL else (GRID[name], "plain")
    gen = torch.Generator().manual_seed(_seed(name))
    uni = lambda *shape: torch.rand(*shape, generator=gen) * 2.0 - 1.0
    c = {"node_emb": uni(N, d), "type_emb": uni(N, t, u), "trans_w": 0.3 * torch.randn(t, u, d, generator=gen),
         "att_w1": 0.3 * torch.randn(t, u, a, generator=gen), "att_w2": 0.3 * torch.randn(t, a, generator=gen),
         "neigh": torch.randint(0, N, (N, t, s), generator=gen), "inputs": torch.randint(0, N, (b,), generator=gen),
         "types": torch.randint(0, t, (b,), generator=gen), "G": torch.randn(b, d, generator=gen)}
    if kind == "skewed":
        c["neigh"] = torch.randint(0, USED_NODES, (N, t, s), generator=gen)
        c["inputs"] = torch.randint(0, 20, (b,), generator=gen)
        c["inputs"][torch.randperm(b, generator=gen)[:200]] = SKEW_NODE
        c["types"] = torch.randint(0, t - 1, (b,), generator=gen)
        c["types"][c["types"] >= SKEW_ABSENT_TYPE] += 1
        assert int((c["inputs"] == SKEW_NODE).sum()) >= 200 and not bool((c["types"] == SKEW_ABSENT_TYPE).any())
        assert sorted(c["types"].unique().tolist()) == [0, 1, 2, 4]
    elif kind == "hub":
        c["neigh"][:, HUB_TYPE, :] = HUB_NODE
        assert b * s > 512
    elif kind == "int32":
        for k in ("neigh", "inputs", "types"):
            c[k] = c[k].to(torch.int32)
    elif kind == "zero_norm":
        c["node_emb"][c["inputs"][0]] = 0.0
        c["trans_w"][c["types"][0]] = 0.0
    elif kind == "large_e":
        e = _scores(c).abs().max()
        c["att_w2"] = (c["att_w2"].double() * (1000.0 / e)).float()
        assert 200.0 <= float(_scores(c).abs().max()) <= 2000.0
    elif kind == "saturated":
        c["att_w1"] = c["att_w1"] * 1.0e6
        x = c["inputs"]
        pre = torch.matmul(_neighbour_sums(c)[x].float(), c["att_w1"][c["types"]])
        assert bool((torch.tanh(pre).abs() == 1.0).all())
    return c


def _neighbour_sums(c):
    """c[n, i, :] = SUM_s type_emb[neigh[n, i, s], i, :] in float64, [N, T, U]"""
    t = c["type_emb"].shape[1]
    nb = c["neigh"].long()
    return torch.stack([c["type_emb"].double()[nb[:, i, :], i, :].sum(1) for i in range(t)], dim=1)


def _scores(c):
    """e [B, T] in float64"""
    x, t = c["inputs"].long(), c["types"].long()
    h = torch.tanh(torch.matmul(_neighbour_sums(c)[x], c["att_w1"].double()[t]))
    return torch.matmul(h, c["att_w2"].double()[t].unsqueeze(2)).squeeze(2)


FLOATS = ("node_emb", "type_emb", "trans_w", "att_w1", "att_w2")


def run(fn, name, device="cpu", dtype=torch.float32, rows=None):
    """fn(*operands) -> out; -> {"out", "g_node", "g_type", "g_trans", "g_w1", "g_w2"} on the CPU.  The offset case places
    node_emb 1 float and type_emb 2 floats past a 16-byte boundary.  rows: only the first `rows` samples."""
    c = make(name)
    ops = []
    for i, k in enumerate(FLOATS):
        v = c[k].detach().clone().to(device=device, dtype=dtype)
        if name == "offset_tables" and i < 2:
            v, _ = O.shifted(v, i + 1)
            assert v.data_ptr() % 16 == ((i + 1) * v.element_size()) % 16
        ops.append(v.requires_grad_())
    inputs, types, G = c["inputs"], c["types"], c["G"]
    if rows is not None:
        inputs, types, G = inputs[:rows], types[:rows], G[:rows]
    out = fn(*ops, c["neigh"].to(device), inputs.to(device), types.to(device))
    grads = torch.autograd.grad(out, ops, G.to(device=device, dtype=dtype))
    return {k: v.detach().cpu() for k, v in zip(NAMES, (out,) + grads)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(oracle, ref32): the composition in float64 and in float32 on the CPU, on the same float32 inputs.  Read-only."""
    return run(composition, name, dtype=torch.float64), run(composition, name)


def errors(got, oracle, ref32):
    """{name: (err_new, err_ref, bound)}"""
    res = {}
    for k, want in oracle.items():
        err_ref = float((ref32[k].double() - want).abs().max())
        err_new = float((got[k].double() - want).abs().max())
        res[k] = (err_new, err_ref, 4 * err_ref + 8 * EPS32 * float(want.abs().max()))
    return res


def check(label, got, oracle, ref32):
    """Print both errors of every tensor, then assert the rule and that everything is finite."""
    bad = []
    for k, (err_new, err_ref, bound) in errors(got, oracle, ref32).items():
        line = "%s %-8s err_new %.3e  err_ref %.3e  bound %.3e" % (label, k, err_new, err_ref, bound)
        print(line)
        if not (bool(torch.isfinite(got[k]).all()) and err_new <= bound):
            bad.append(line)
    assert not bad, bad


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))
