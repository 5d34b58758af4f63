"""Shared by the kgscore tests: the cases, the law of cogdl_amd/csrc/kgscore_law.h restated in numpy float32 (slot partials,
butterfly, ordered gradient sums, chunked list sums), a float64 evaluation of the same formulas and the error bounds derived
from them.  Every result is computed once per case and kept (functools.lru_cache); callers do not write into them.

The shapes are the smallest that reach each way the kernels can go wrong: D of 2 and 6 (fewer terms than slots), 66 (not a
multiple of 4: the scalar loads), 250, 256 and 2000 (several terms per slot, RotatE's width); K of 1, 3 and 130 (more j than
one pass of a workgroup's four waves); B of 1 and 70; N of 1, of 40 with entities no id names (zero rows of grad_table) and the
ids 0 and N - 1 present, and of 3 with B = K = 64, where every list holds over 1,300 occurrences and crosses the 512-chunk
boundary at least twice.  Row 0 of q equals the table row of its first candidate exactly (the zero-derivative branches of l1
and cl2); gamma is 12.
"""
import functools

import numpy as np

KINDS = ("dot", "l1", "cl2")
GAMMA = 12.0
CHUNK = 512
U = 2.0 ** -24
# name -> (B, K, N, D)
SHAPES = {
    "one": (1, 1, 1, 2),
    "few_terms": (1, 3, 40, 6),
    "scalar_66": (70, 3, 40, 66),
    "many_j_250": (70, 130, 40, 250),
    "many_j_256": (1, 130, 40, 256),
    "wide_2000": (70, 3, 40, 2000),
    "wide_2000_many_j": (1, 130, 40, 2000),
    "long_lists_6": (64, 64, 3, 6),
    "long_lists_256": (64, 64, 3, 256),
}
CASES = [(name, kind) for name in SHAPES for kind in KINDS]
UNNAMED = (5, 6, 7, 8, 9, 23)  # entities of the N = 40 cases that no id names


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict(q [B, D], table [N, D], idx int64 [B, K], g [B, K]) float32 numpy, read-only."""
    b, k, n, d = SHAPES[name]
    rng = np.random.RandomState(sum(map(ord, name)) + 17 * d)
    table = (rng.standard_normal((n, d)) * 0.5).astype(np.float32)
    q = rng.standard_normal((b, d)).astype(np.float32)
    if n == 40:
        allowed = np.asarray([e for e in range(n) if e not in UNNAMED])
        idx = allowed[rng.randint(len(allowed), size=(b, k))]
        flat = idx.reshape(-1)
        flat[-1] = n - 1
        if flat.size > 1:
            flat[0] = 0
        idx = flat.reshape(b, k)
    else:
        idx = rng.randint(n, size=(b, k))
    idx = idx.astype(np.int64)
    q[0] = table[idx[0, 0]]
    g = rng.standard_normal((b, k)).astype(np.float32)
    out = dict(q=q, table=table, idx=idx, g=g)
    for v in out.values():
        v.setflags(write=False)
    return out


def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays, correctly rounded: the product is exact in float64, the float64 sum is made a
    round-to-odd sum with the TwoSum error term, and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the single
    rounding of the exact a * b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = c + p
    bb = s - c
    err = (c - (s - bb)) + (p - bb)
    even = (s.view(np.int64) & 1) == 0
    nudge = (err != 0) & even
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(nudge, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def _butterfly(p):
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ off]
    return p


def law_scores_rows(kind, qrows, trows, gamma=GAMMA):
    """The law's score of R pairs of rows ([R, D] float32 each) -> [R] float32."""
    r, d = qrows.shape
    half = d // 2
    terms = half if kind == "cl2" else d
    groups = -(-terms // 256)
    pad = groups * 256

    def slots(x):  # [R, terms] -> [R, groups, 64, 4]: term k = 4 (l + 64 i) + c sits at [i][l][c]
        out = np.zeros((r, pad), dtype=np.float32)
        out[:, :terms] = x
        return out.reshape(r, groups, 64, 4)

    qa, ta = slots(qrows[:, :terms]), slots(trows[:, :terms])
    if kind == "cl2":
        qb, tb = slots(qrows[:, half:]), slots(trows[:, half:])
    live = (np.arange(pad) < terms).reshape(groups, 64, 4)
    acc = np.zeros((r, 64), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(groups):
            for c in range(4):
                x, y = qa[:, i, :, c], ta[:, i, :, c]
                if kind == "dot":
                    new = _fma32(x, y, acc)
                elif kind == "l1":
                    new = acc + np.abs(x - y)
                else:
                    re, im = x - y, qb[:, i, :, c] - tb[:, i, :, c]
                    new = acc + np.sqrt(re * re + im * im)
                acc = np.where(live[i, :, c][None, :], new, acc).astype(np.float32)
    total = _butterfly(acc)[:, 0]
    return total if kind == "dot" else (np.float32(gamma) - total).astype(np.float32)


def _partials32(kind, q, t, wrt):
    """ds/dq (wrt "q") or ds/dt (wrt "t") per column, float32 [.., D], one rounding per operation."""
    if kind == "dot":
        return (t if wrt == "q" else q).astype(np.float32)
    if kind == "l1":
        s = np.sign(q - t).astype(np.float32)
        return -s if wrt == "q" else s
    half = q.shape[-1] // 2
    re, im = q[..., :half] - t[..., :half], q[..., half:] - t[..., half:]
    m = np.sqrt(re * re + im * im)
    with np.errstate(invalid="ignore", divide="ignore"):
        d_re = np.where(m == 0, np.float32(0), -(re / m))
        d_im = np.where(m == 0, np.float32(0), -(im / m))
    out = np.concatenate([d_re, d_im], axis=-1).astype(np.float32)
    return out if wrt == "q" else -out


def law_scores(kind, q, table, idx, gamma=GAMMA):
    b, k = idx.shape
    n = table.shape[0]
    valid = (idx >= 0) & (idx < n)
    safe = np.where(valid, idx, 0)
    s = law_scores_rows(kind, np.repeat(q, k, axis=0), table[safe.reshape(-1)], gamma).reshape(b, k)
    return np.where(valid, s, np.float32(np.nan)).astype(np.float32)


def law_grad_q(kind, q, table, idx, g):
    b, k = idx.shape
    n = table.shape[0]
    acc = np.zeros_like(q)
    for j in range(k):
        valid = (idx[:, j] >= 0) & (idx[:, j] < n)
        t = table[np.where(valid, idx[:, j], 0)]
        contribution = g[:, j, None] * _partials32(kind, q, t, "q")
        acc = np.where(valid[:, None], acc + contribution, acc).astype(np.float32)
    return acc


def law_grad_table(kind, q, table, idx, g):
    b, k = idx.shape
    n = table.shape[0]
    flat, gflat = idx.reshape(-1), g.reshape(-1)
    out = np.zeros_like(table)
    for e in range(n):
        pos = np.nonzero(flat == e)[0]  # ascending
        total = np.zeros(table.shape[1], dtype=np.float32)
        for c0 in range(0, len(pos), CHUNK):
            part = np.zeros(table.shape[1], dtype=np.float32)
            chunk = pos[c0:c0 + CHUNK]
            partials = _partials32(kind, q[chunk // k], table[e][None, :], "t")
            contributions = gflat[chunk, None] * partials
            for row in contributions:
                part = part + row
            total = total + part
        out[e] = total
    return out


def gamma_n(n):
    return n * U / (1 - n * U)


@functools.lru_cache(maxsize=None)
def law(name, kind):
    """(scores, grad_q, grad_table) under the restated law, float32."""
    c = make(name)
    out = (law_scores(kind, c["q"], c["table"], c["idx"]), law_grad_q(kind, c["q"], c["table"], c["idx"], c["g"]),
           law_grad_table(kind, c["q"], c["table"], c["idx"], c["g"]))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def exact(name, kind):
    """The same formulas in float64 on the float32 inputs, with the bounds of the float32 evaluation:
    -> (scores, grad_q, grad_table, bound_scores, bound_grad_q, bound_grad_table).

    Derivation.  A float32 sum of n values in any order errs by at most gamma_(n-1) SUM|values| (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2), gamma_n = n u / (1 - n u), u = 2^-24; roundings made on a value before it
    enters the sum multiply it by at most (1 + u)^r and add r to the index.  A score sums at most D terms (D - 1 additions in
    the worst order); a term carries at most 5 roundings of its own (cl2: two differences that act as one relative
    perturbation of the modulus, two squares that act as one, their sum, the square root; the fused dot step has none), the
    finish `gamma - acc` one more, gamma itself counting as a term: n = D + 8 covers D - 1 + 5 + 1 with room.  A gradient element
    sums its contributions (summands - 1 additions); a contribution g * partial carries the product's rounding and at most
    three more in the partial (cl2: the modulus as above, the division; the perturbed differences move re / m by less than
    one u relative each but with opposite signs in numerator and denominator): n = summands + 4."""
    c = make(name)
    q, table, idx, g = (c[k].astype(np.float64) if k != "idx" else c[k] for k in ("q", "table", "idx", "g"))
    b, k = idx.shape
    n, d = table.shape
    half = d // 2
    scores = np.zeros((b, k))
    abs_terms = np.zeros((b, k))
    grad_q, abs_q = np.zeros((b, d)), np.zeros((b, d))
    grad_t, abs_t = np.zeros((n, d)), np.zeros((n, d))
    count_t = np.zeros(n)
    for j in range(k):
        t = table[idx[:, j]]
        if kind == "dot":
            terms = q * t
            dq, dt = t, q
        elif kind == "l1":
            terms = np.abs(q - t)
            dq = -np.sign(q - t)
            dt = -dq
        else:
            re, im = q[:, :half] - t[:, :half], q[:, half:] - t[:, half:]
            m = np.sqrt(re * re + im * im)
            terms = m
            with np.errstate(invalid="ignore", divide="ignore"):
                dq = np.concatenate([np.where(m == 0, 0.0, -re / m), np.where(m == 0, 0.0, -im / m)], axis=1)
            dt = -dq
        total = terms.sum(1)
        scores[:, j] = total if kind == "dot" else GAMMA - total
        abs_terms[:, j] = np.abs(terms).sum(1) + (0.0 if kind == "dot" else GAMMA)
        grad_q += g[:, j, None] * dq
        abs_q += np.abs(g[:, j, None] * dq)
        np.add.at(grad_t, idx[:, j], g[:, j, None] * dt)
        np.add.at(abs_t, idx[:, j], np.abs(g[:, j, None] * dt))
        np.add.at(count_t, idx[:, j], 1.0)
    out = (scores, grad_q, grad_t, gamma_n(d + 8) * abs_terms, gamma_n(k + 4) * abs_q, gamma_n(count_t + 4)[:, None] * abs_t)
    for v in out:
        v.setflags(write=False)
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
