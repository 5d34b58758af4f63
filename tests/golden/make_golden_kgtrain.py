"""Writes tests/golden/kg_train.npz: a small batch of triples with negatives, embedding tables for the reference's four
triple-scoring models, the reference's own forward outputs for all three modes and the gradients of both embedding tables
under the reference's own TripleModelWrapper.train_step loss.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs.
CPU only.

N = 30 entities, 5 relations, hidden 8 (16 where the entity / relation dimension is doubled), gamma 12, B = 6 positive triples
with K = 7 negative heads and 7 negative tails each, subsampling weights in (0.2, 1).  One entity table N(0, 0.5^2) serves all
models (the narrow ones take its first 8 columns); relation rows are uniform in the model's embedding_range.
Recorded: the inputs; per model and mode the output of model(sample, mode) from the float32 model (score_f32_*) and from the
same model in float64 (score_f64_*); per model and negative mode the gradients of entity_embedding and relation_embedding
after train_step(...).backward() with the wrapper's default arguments (grad_entity_* / grad_relation_*, f32 and f64) and, for
tail-batch, with negative_adversarial_sampling on (.._adv_..); the loss values.  Asserted while writing: the restatement of the
loss in tests/_kgtrain_cases.py equals the reference's float64 loss to 1e-12.  Only arrays are stored."""
import argparse
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "/root/reference")
MAX_BYTES = 100_000


def main():
    import torch

    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    from cogdl.models.emb.complex import ComplEx
    from cogdl.models.emb.distmult import DistMult
    from cogdl.models.emb.rotate import RotatE
    from cogdl.models.emb.transe import TransE
    from cogdl.wrappers.model_wrapper.link_prediction.triple_link_prediction_mw import TripleModelWrapper

    import _kgtrain_cases as C

    classes = {"transe": TransE, "distmult": DistMult, "complex": ComplEx, "rotate": RotatE}
    rng = np.random.RandomState(20262)
    out = {"entity": (rng.standard_normal((C.N, 2 * C.HIDDEN)) * 0.5).astype(np.float32)}
    positive = np.stack([rng.randint(C.N, size=C.B), rng.randint(C.NUM_RELS, size=C.B), rng.randint(C.N, size=C.B)], axis=1)
    positive[1, 2] = positive[0, 2]  # an entity that is a tail twice
    out["positive"] = positive.astype(np.int16)
    for side in ("head", "tail"):
        neg = rng.randint(C.N, size=(C.B, C.K))
        neg[0, 0], neg[0, 1] = positive[0, 0], neg[0, 2]  # a negative that is the fixed entity; a repeated negative
        out["negative_" + side] = neg.astype(np.int16)
    out["weight"] = rng.uniform(0.2, 1.0, size=C.B).astype(np.float32)
    pos_t, weight = torch.from_numpy(positive.astype(np.int64)), torch.from_numpy(out["weight"])

    def wrapper(model, adversarial):
        mw = TripleModelWrapper.__new__(TripleModelWrapper)  # (its __init__ parses the command line)
        torch.nn.Module.__init__(mw)
        mw.model = model
        mw.args = argparse.Namespace(negative_adversarial_sampling=adversarial, adversarial_temperature=1.0, uni_weight=False,
                                     regularization=C.REGULARIZATION)
        return mw

    for name in C.MODELS:
        rel_dim = C.HIDDEN * (2 if C.DOUBLE_RELATION[name] else 1)
        out["relation_" + name] = rng.uniform(-C.EMBEDDING_RANGE, C.EMBEDDING_RANGE, size=(C.NUM_RELS, rel_dim)).astype(np.float32)
        ent, rel = C.tables(out, name)
        model = classes[name](C.N, C.NUM_RELS, C.HIDDEN, C.GAMMA, C.DOUBLE_ENTITY[name], C.DOUBLE_RELATION[name])
        assert abs(model.embedding_range.item() - C.EMBEDDING_RANGE) == 0 and model.gamma.item() == C.GAMMA
        with torch.no_grad():
            model.entity_embedding.copy_(torch.from_numpy(ent))
            model.relation_embedding.copy_(torch.from_numpy(rel))
        model64 = classes[name](C.N, C.NUM_RELS, C.HIDDEN, C.GAMMA, C.DOUBLE_ENTITY[name], C.DOUBLE_RELATION[name]).double()
        model64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
        for tag, mdl in (("f32", model), ("f64", model64)):
            w = weight.to(mdl.entity_embedding.dtype)
            with torch.no_grad():
                for mode in ("single",) + C.MODES:
                    score = mdl(C.sample_of(out, mode), mode)
                    assert score.dtype == mdl.entity_embedding.dtype and tuple(score.shape) == (C.B, 1 if mode == "single" else C.K)
                    out["score_%s_%s_%s" % (tag, name, mode.split("-")[0])] = score.numpy()
            for mode, adversarial in (("head-batch", False), ("tail-batch", False), ("tail-batch", True)):
                mdl.zero_grad()
                neg_t = C.sample_of(out, mode)[1]
                loss = wrapper(mdl, adversarial).train_step(iter([(pos_t, neg_t, w, mode)]))
                loss.backward()
                key = "%s_%s_%s%s" % (tag, name, mode.split("-")[0], "_adv" if adversarial else "")
                out["loss_" + key] = np.asarray(loss.item())
                out["grad_entity_" + key] = mdl.entity_embedding.grad.numpy().copy()
                out["grad_relation_" + key] = mdl.relation_embedding.grad.numpy().copy()
                if tag == "f64":
                    with torch.no_grad():
                        mine = C.train_loss(mdl((pos_t, neg_t), mode), mdl(pos_t), w, mdl.entity_embedding, mdl.relation_embedding,
                                            adversarial)
                    assert abs(mine.item() - loss.item()) <= 1e-12, (key, mine.item(), loss.item())
                print("%-28s loss %.6f" % (key, loss.item()))
    path = os.path.join(HERE, "kg_train.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < MAX_BYTES, size
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
