"""score_triples on the CPU against tests/golden/kg_train.npz, recorded from the reference's own TransE, DistMult, ComplEx and
RotatE: the forward outputs of all three modes and the gradients of both embedding tables under the reference's train_step
loss (plain and self-adversarial), within the bound of tests/_kgtrain_cases.py of the float64 record and within twice that
bound of the float32 record; the float64 torch route reproduces the float64 record."""
import numpy as np
import pytest
import torch

import _kgtrain_cases as C
from cogdl_amd import kgtrain
from cogdl_amd.kgtrain import score_triples

G = C.load()


def params(model, dtype=torch.float32):
    ent, rel = C.tables(G, model)
    return torch.from_numpy(ent).to(dtype).requires_grad_(), torch.from_numpy(rel).to(dtype).requires_grad_()


def scorer(model, ent, rel):
    return lambda sample, mode: score_triples(model, ent, rel, sample, mode, C.EMBEDDING_RANGE, C.GAMMA)


def case_bounds(model, mode, adversarial=False):
    ent, rel = C.tables(G, model)
    e64, r64 = params(model, torch.float64)
    pos, neg = C.sample_of(G, mode)
    return C.bounds(model, mode, ent, rel, pos, neg, torch.from_numpy(G["weight"]), scorer(model, e64, r64), adversarial)


@pytest.mark.parametrize("model", C.MODELS)
def test_forward_matches_the_reference_record(model):
    ent, rel = params(model)
    e64, r64 = params(model, torch.float64)
    for mode in C.MODES:
        b_neg, b_pos, _, _ = case_bounds(model, mode)
        for m, bound in ((mode, b_neg), ("single", b_pos)):
            got = scorer(model, ent, rel)(C.sample_of(G, m), m)
            assert got.dtype == torch.float32 and tuple(got.shape) == (C.B, 1 if m == "single" else C.K)
            tag = "%s_%s" % (model, m.split("-")[0])
            C.within(got.detach().numpy(), G["score_f64_" + tag], bound, tag + " vs float64 record")
            C.within(got.detach().numpy(), G["score_f32_" + tag], 2 * bound, tag + " vs float32 record")
            # the float64 torch route is the reference's arithmetic re-associated
            got64 = scorer(model, e64, r64)(C.sample_of(G, m), m).detach().numpy()
            assert np.abs(got64 - G["score_f64_" + tag]).max() <= 64 * np.finfo(np.float64).eps * np.abs(G["score_f64_" + tag]).max() + 1e-13


@pytest.mark.parametrize("model", C.MODELS)
@pytest.mark.parametrize("mode,adversarial", [("head-batch", False), ("tail-batch", False), ("tail-batch", True)])
def test_train_step_gradients_match_the_reference_record(model, mode, adversarial):
    ent, rel = params(model)
    pos, neg = C.sample_of(G, mode)
    weight = torch.from_numpy(G["weight"])
    score = scorer(model, ent, rel)
    loss = C.train_loss(score((pos, neg), mode), score(pos, "single"), weight, ent, rel, adversarial)
    loss.backward()
    key = "%s_%s%s" % (model, mode.split("-")[0], "_adv" if adversarial else "")
    b_neg, b_pos, b_ent, b_rel = case_bounds(model, mode, adversarial)
    # sum |d loss / d s| <= 1 (normalised weights, a mean or a softmax over j, sigmoid <= 1, the halves): the loss errs by at
    # most the largest score bound, plus its own few roundings
    loss_bound = float(max(b_neg.max(), b_pos.max())) + C.gamma_n(C.B + C.K + 32) * abs(float(G["loss_f64_" + key]))
    C.within(loss.item(), G["loss_f64_" + key], loss_bound, key + " loss")
    C.within(ent.grad.numpy(), G["grad_entity_f64_" + key], b_ent, key + " grad entity vs float64 record")
    C.within(rel.grad.numpy(), G["grad_relation_f64_" + key], b_rel, key + " grad relation vs float64 record")
    C.within(ent.grad.numpy(), G["grad_entity_f32_" + key], 2 * b_ent, key + " grad entity vs float32 record")
    C.within(rel.grad.numpy(), G["grad_relation_f32_" + key], 2 * b_rel, key + " grad relation vs float32 record")


def test_gradients_reach_entity_through_query_and_table_and_modes_raise():
    ent, rel = params("distmult")
    pos, neg = C.sample_of(G, "tail-batch")
    s = score_triples("distmult", ent, rel, (pos, neg), "tail-batch")
    s.sum().backward()
    named = set(neg.reshape(-1).tolist())
    heads = set(pos[:, 0].tolist())
    rows = set(torch.nonzero(ent.grad.abs().sum(1)).reshape(-1).tolist())
    assert rows == named | heads and heads - named  # (a head no negative names still gets its query gradient)
    assert set(torch.nonzero(rel.grad.abs().sum(1)).reshape(-1).tolist()) == set(pos[:, 1].tolist())
    with pytest.raises(ValueError, match="mode other not supported"):
        score_triples("distmult", ent, rel, pos, "other")
    with pytest.raises(ValueError):
        score_triples("conve", ent, rel, pos, "single")
    with pytest.raises(ValueError):
        score_triples("rotate", *params("rotate"), pos, "single")  # no embedding_range
    assert kgtrain.TRAIN_MODES == ("single", "head-batch", "tail-batch")
