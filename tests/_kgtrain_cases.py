"""Shared by the kgtrain tests and tests/golden/make_golden_kgtrain.py: the golden case, the training loss of
TripleModelWrapper.train_step restated on [B, K] scores, and the error bounds the tests hold the served route to.

The bound.  An expression evaluated in float32 with at most n roundings on any path from an input to the result errs by at
most gamma_n = n u / (1 - n u), u = 2^-24, times its MAJORANT: the same expression with every input replaced by its absolute
value and every difference by a sum (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and 4.2; the same
gamma_n SUM|term| rule as tests/_kgscore_cases.py, applied to the whole score instead of one sum).  majorant_scores builds it
in float64 for the four models: the query of cogdl_amd.kgrank.prepare_query on absolute values (RotatE's cos and sin are
replaced by 1 + |phase|, which also majorises their derivative and their sensitivity to the phase's rounding), then the sum
over the embedding width; for cl2 the modulus is majorised by |re| + |im|, whose derivative 1 majorises re / m.  A score has
D - 1 additions, up to 5 roundings inside a term and up to 8 in the query (RotatE: the division, cos and sin within two ulps
each, two products, one sum): n = D + 16.
Gradients.  d loss / d table[e, k] is a sum of contributions (d loss / d s[b, j]) * (d s[b, j] / d table[e, k]); the majorant
of the sum is the gradient of SUM |d loss / d s| * majorant_score with respect to the absolute inputs, which torch autograd
computes.  Two errors enter: the float32 evaluation of the sum itself, gamma_n of the majorant with n = B (K + 1) summands +
D + 48 roundings per path (the score's, the loss's sigmoid / softmax / weights / means); and the float32 error of the scores
the loss is differentiated AT: d log sigmoid(+-s) / d s = +-sigmoid(-+s) changes by a relative |ds| at most, a detached softmax
weight by 2 max|ds|: a factor 3 max(score bound) on every contribution.  Two float32 routes (the served one and the
reference's) differ by at most twice the bound.
"""
import os

import numpy as np
import torch

import _kgrank_cases as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kg_train.npz")
N, NUM_RELS, HIDDEN, B, K, GAMMA = 30, 5, 8, 6, 7, 12.0
EMBEDDING_RANGE = float(np.float32((np.float32(GAMMA) + np.float32(2.0)) / np.float32(HIDDEN)))  # as KGEModel.__init__ computes it
MODELS = ("transe", "distmult", "complex", "rotate")
MODES = ("head-batch", "tail-batch")
DOUBLE_ENTITY, DOUBLE_RELATION, PI = R.DOUBLE_ENTITY, R.DOUBLE_RELATION, R.PI
REGULARIZATION = 1e-9  # TripleModelWrapper's defaults
U = 2.0 ** -24


def gamma_n(n):
    return n * U / (1 - n * U)


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def tables(g, model):
    ent = g["entity"]
    ent = np.ascontiguousarray(ent if DOUBLE_ENTITY[model] else ent[:, :HIDDEN])
    return ent, g["relation_" + model]


def sample_of(g, mode):
    pos = torch.from_numpy(g["positive"].astype(np.int64))
    if mode == "single":
        return pos
    return pos, torch.from_numpy(g["negative_" + mode.split("-")[0]].astype(np.int64))


def train_loss(negative_score, positive_score, weight, entity, relation, adversarial=False, temperature=1.0,
               regularization=REGULARIZATION):
    """TripleModelWrapper.train_step's loss (triple_link_prediction_mw.py:45-72, uni_weight off) from the two score tensors."""
    F = torch.nn.functional
    if adversarial:
        negative = (F.softmax(negative_score * temperature, dim=1).detach() * F.logsigmoid(-negative_score)).sum(dim=1)
    else:
        negative = F.logsigmoid(-negative_score).mean(dim=1)
    positive = F.logsigmoid(positive_score).squeeze(dim=1)
    loss = (-(weight * positive).sum() / weight.sum() - (weight * negative).sum() / weight.sum()) / 2
    if regularization != 0.0:
        loss = loss + regularization * (entity.norm(p=3) ** 3 + relation.norm(p=3).norm(p=3) ** 3)
    return loss


def majorant_scores(model, mode, ent_abs, rel_abs, sample, embedding_range=EMBEDDING_RANGE):
    """[B, K] ([B, 1] for "single"): the score expression on absolute values, differences as sums; see the module docstring."""
    if mode == "single":
        pos, idx, fixed = sample, sample[:, 2:3], sample[:, 0]
    else:
        pos, idx = sample
        fixed = pos[:, 2] if mode == "head-batch" else pos[:, 0]
    rows, rel, t = ent_abs[fixed], rel_abs[pos[:, 1]], ent_abs[idx]
    if model == "transe":
        return GAMMA + ((rows + rel).unsqueeze(1) + t).sum(-1)
    if model == "distmult":
        return ((rows * rel).unsqueeze(1) * t).sum(-1)
    re_e, im_e = torch.chunk(rows, 2, dim=1)
    if model == "complex":
        re_r, im_r = torch.chunk(rel, 2, dim=1)
    else:
        re_r = im_r = 1.0 + rel * (PI / embedding_range)
    q = torch.cat([re_r * re_e + im_r * im_e, re_r * im_e + im_r * re_e], dim=1).unsqueeze(1)
    return (q * t).sum(-1) if model == "complex" else GAMMA + (q + t).sum(-1)


def bounds(model, mode, ent, rel, positive, negative, weight, score64, adversarial=False, embedding_range=EMBEDDING_RANGE):
    """-> (bound_negative [B, K], bound_positive [B, 1], bound_grad_entity [N, D_e], bound_grad_relation [R, D_r]) float64 numpy,
    for the float32 evaluation of the two score tensors and of the gradients of train_loss.  `score64(sample, mode)` evaluates
    the scores in float64 with autograd (where the loss is differentiated)."""
    ea = torch.from_numpy(np.abs(ent).astype(np.float64)).requires_grad_()
    ra = torch.from_numpy(np.abs(rel).astype(np.float64)).requires_grad_()
    d = ent.shape[1]
    m_neg = majorant_scores(model, mode, ea, ra, (positive, negative), embedding_range)
    m_pos = majorant_scores(model, "single", ea, ra, positive, embedding_range)
    b_neg, b_pos = gamma_n(d + 16) * m_neg.detach(), gamma_n(d + 16) * m_pos.detach()
    # |d loss / d s| at the float64 scores
    s_neg, s_pos = score64((positive, negative), mode), score64(positive, "single")
    e64 = torch.from_numpy(ent.astype(np.float64))
    r64 = torch.from_numpy(rel.astype(np.float64))
    loss = train_loss(s_neg, s_pos, weight.double(), e64, r64, adversarial, regularization=0.0)
    w_neg, w_pos = torch.autograd.grad(loss, (s_neg, s_pos))
    major = (w_neg.abs() * m_neg).sum() + (w_pos.abs() * m_pos).sum() + REGULARIZATION * ((ea ** 3).sum() + (ra ** 3).sum())
    g_ent, g_rel = torch.autograd.grad(major, (ea, ra))
    n = positive.shape[0] * (negative.shape[1] + 1) + d + 48
    factor = gamma_n(n) + 3.0 * float(max(b_neg.max(), b_pos.max()))
    return b_neg.numpy(), b_pos.numpy(), factor * g_ent.numpy(), factor * g_rel.numpy()


def within(got, want, bound, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    print("%s: max |err| %.3e, max err / bound %.3f" % (what, err.max(), float((err / np.maximum(bound, 1e-300)).max())))
    assert float((err - bound).max()) <= 0.0, what


def synthetic_batches(n=200, rels=7, b=32, k=16, steps=3, seed=3):
    """`steps` batches (positive [b, 3], negative [b, k], weight [b], mode) on a synthetic graph, head-batch and tail-batch in
    turn as the reference's BidirectionalOneShotIterator deals them."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for t in range(steps):
        pos = torch.stack([torch.randint(0, n, (b,), generator=gen), torch.randint(0, rels, (b,), generator=gen),
                           torch.randint(0, n, (b,), generator=gen)], dim=1)
        out.append((pos, torch.randint(0, n, (b, k), generator=gen), torch.rand(b, generator=gen) * 0.8 + 0.2, MODES[t % 2]))
    return out


def synthetic_tables(model, n=200, rels=7, hidden=64, seed=4, gamma=GAMMA):
    """(entity, relation, embedding_range) float32, initialised as KGEModel.__init__ does."""
    gen = torch.Generator().manual_seed(seed)
    rng = float(np.float32((np.float32(gamma) + np.float32(2.0)) / np.float32(hidden)))
    de = hidden * (2 if DOUBLE_ENTITY[model] else 1)
    dr = hidden * (2 if DOUBLE_RELATION[model] else 1)
    return (torch.rand(n, de, generator=gen) * 2 - 1) * rng, (torch.rand(rels, dr, generator=gen) * 2 - 1) * rng, rng


def adamw_run(ent, rel, forward, batches, device, lr=1e-3):
    """len(batches) AdamW steps on the two tables under train_loss; forward(sample, mode) scores with them.
    -> (losses, entity, relation) with the losses as Python floats and the final tables on the CPU."""
    opt = torch.optim.AdamW([ent, rel], lr=lr)
    losses = []
    for pos, neg, weight, mode in batches:
        pos, neg, weight = pos.to(device), neg.to(device), weight.to(device=device, dtype=ent.dtype)
        opt.zero_grad()
        loss = train_loss(forward((pos, neg), mode), forward(pos, "single"), weight, ent, rel)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, ent.detach().cpu(), rel.detach().cpu()


def trajectory_tolerances(model, ent0, rel0, rng, batches, score64, ref32, ref64):
    """Per step t the tolerance of a float32 loss trajectory against the float64 one, MEASURED against the reference's float64
    run (not derived beyond step 0): at every step a float32 route may err by the derived bound of the first step's loss (the
    largest score bound, sum |d loss / d s| <= 1, plus the loss's own roundings), and two trajectories drift apart by what the
    reference's own float32 route has drifted from its float64 run, taken 4 times (two routes, each with its own order of
    summation in forward and in backward); both accumulate linearly over the steps: tol_t = (t + 1) (2 bound_0 + 4 |ref32_t -
    ref64_t|)."""
    pos, neg, weight, mode = batches[0]
    b_neg, b_pos, _, _ = bounds(model, mode, ent0.numpy(), rel0.numpy(), pos, neg, weight, score64, embedding_range=rng)
    bound0 = float(max(b_neg.max(), b_pos.max())) + gamma_n(pos.shape[0] + neg.shape[1] + 32) * abs(ref64[0])
    return [(t + 1) * (2 * bound0 + 4 * abs(a - b)) for t, (a, b) in enumerate(zip(ref32, ref64))]
