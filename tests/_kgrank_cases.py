"""Shared by the kgrank tests and tests/golden/make_golden_kgrank.py: the golden cases and a float64 numpy restatement of the
three score kinds, of the four models' queries and of the counts.  Nothing here imports cogdl_amd."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kg_rank.npz")
N, NUM_RELS, HIDDEN, GAMMA, NUM_TRUE, NUM_TEST, SCORE_ROWS = 257, 7, 24, 12.0, 2300, 300, 16
EMBEDDING_RANGE = float(np.float32((np.float32(GAMMA) + np.float32(2.0)) / np.float32(HIDDEN)))  # as KGEModel.__init__ computes it
MODES = ("head-batch", "tail-batch")
# (model, family): the exact family leaves RotatE out (cos and sin are never exact)
CASES = [(m, "exact") for m in ("transe", "distmult", "complex")] + [(m, "float") for m in ("transe", "distmult", "complex", "rotate")]
DOUBLE_ENTITY = {"transe": False, "distmult": False, "complex": True, "rotate": True}
DOUBLE_RELATION = {"transe": False, "distmult": False, "complex": True, "rotate": False}
KIND = {"transe": "l1", "distmult": "dot", "complex": "dot", "rotate": "cl2"}
EPS32 = float(np.finfo(np.float32).eps)
AMBIGUOUS_CAP = 0.05
PI = 3.14159265358979323846


def tag(model, family, mode):
    return "%s_%s_%s" % (model, family, mode.split("-")[0])


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def tables(g, model, family):
    """(entity [N, D_e], relation [R, D_r]) float32 of a case: the models share one entity table per family, the narrow ones
    take its first HIDDEN columns."""
    ent = g["entity_" + family]
    ent = np.ascontiguousarray(ent if DOUBLE_ENTITY[model] else ent[:, :HIDDEN])
    return ent, g["relation_%s_%s" % (model, family)]


def scores64(kind, q, table, gamma):
    """[M, N] float64 scores of the three kinds."""
    q, table = np.asarray(q, dtype=np.float64), np.asarray(table, dtype=np.float64)
    if kind == "dot":
        return q @ table.T
    if kind == "l1":
        return gamma - np.abs(q[:, None, :] - table[None, :, :]).sum(-1)
    h = q.shape[1] // 2
    re = q[:, None, :h] - table[None, :, :h]
    im = q[:, None, h:] - table[None, :, h:]
    return gamma - np.sqrt(re * re + im * im).sum(-1)


def query64(model, mode, rows, rel, embedding_range=EMBEDDING_RANGE):
    """The float64 query of a model: what cogdl_amd.kgrank.prepare_query computes in float32."""
    rows, rel = np.asarray(rows, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    head = mode == "head-batch"
    if model == "transe":
        return rows - rel if head else rows + rel
    if model == "distmult":
        return rows * rel
    h = rows.shape[1] // 2
    re_e, im_e = rows[:, :h], rows[:, h:]
    if model == "complex":
        re_r, im_r = rel[:, : rel.shape[1] // 2], rel[:, rel.shape[1] // 2:]
    else:
        phase = rel / (embedding_range / PI)
        re_r, im_r = np.cos(phase), np.sin(phase)
    if head:
        return np.concatenate([re_r * re_e + im_r * im_e, re_r * im_e - im_r * re_e], axis=1)
    return np.concatenate([re_e * re_r - im_e * im_r, re_e * im_r + im_e * re_r], axis=1)


def fixed_free(mode):
    return (2, 0) if mode == "head-batch" else (0, 2)


def model_scores64(model, mode, ent, rel, triples, gamma=GAMMA):
    """[M, N] float64: the model's score of every triple against every entity in the free slot, and the targets."""
    fixed, free = fixed_free(mode)
    q = query64(model, mode, ent[triples[:, fixed]], rel[triples[:, 1]])
    return scores64(KIND[model], q, ent, gamma), triples[:, free]


def counts64(s, target, left_out=None):
    """int64 [M, 3] = (greater, equal_before, equal_after) of a score matrix; left_out: bool [M, N] of filtered candidates
    (the target is a candidate of nobody and is never left out)."""
    m, n = s.shape
    ids = np.arange(n)[None, :]
    t = np.asarray(target).reshape(-1, 1)
    keep = ids != t
    if left_out is not None:
        keep &= ~left_out
    st = np.take_along_axis(s, t, axis=1)
    eq = (s == st) & keep
    return np.stack([((s > st) & keep).sum(1), (eq & (ids < t)).sum(1), (eq & (ids > t)).sum(1)], axis=1).astype(np.int64)


def bracket64(s, target, left_out, delta):
    """(lo, hi) per query: #{s > s_t + delta} and #{s >= s_t - delta} - 1 over the candidates that are not left out (the
    target counts itself in the second, hence the - 1)."""
    m, n = s.shape
    t = np.asarray(target).reshape(-1, 1)
    keep = np.ones((m, n), dtype=bool) if left_out is None else ~left_out
    keep[np.arange(m), t[:, 0]] = True
    st = np.take_along_axis(s, t, axis=1)
    lo = ((s > st + delta) & keep).sum(1)
    hi = ((s >= st - delta) & keep).sum(1) - 1
    return lo, hi


def left_out_mask(g, mode):
    """bool [NUM_TEST, N]: the candidates TestDataset gave a filter_bias of -1 (recorded bit-packed)."""
    bits = np.unpackbits(g["filter_bias_" + mode.split("-")[0]], axis=1)[:, :N]
    return bits.astype(bool)


def lists_from_mask(mask):
    """(filt_ptr int32 [M + 1], filt_idx int32) naming the True entries of each row."""
    lens = mask.sum(1)
    ptr = np.zeros(mask.shape[0] + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(lens)
    return ptr, np.nonzero(mask)[1].astype(np.int32)


def delta_of(ref_err, s64):
    """The project's standing bound on a float32 score against the float64 one."""
    return 4.0 * float(ref_err) + 8.0 * EPS32 * float(np.abs(s64).max())


def mrr_bound(lo, hi):
    """Sum over the ambiguous triples of |1 / (1 + lo) - 1 / (1 + hi)|, divided by the number of triples."""
    amb = lo != hi
    return float(np.abs(1.0 / (1.0 + lo[amb]) - 1.0 / (1.0 + hi[amb])).sum() / len(lo))
