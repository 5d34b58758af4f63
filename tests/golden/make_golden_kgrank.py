"""Writes tests/golden/kg_rank.npz: a small knowledge graph, embedding tables for the reference's four triple-scoring models and
the positions the reference's own evaluation gives every test triple.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs.
CPU only.

N = 257 entities, 7 relations, hidden 24 (double entity dimension for ComplEx and RotatE, double relation dimension for ComplEx),
gamma 12, 2300 distinct true triples of which the first 300 are the test triples, both modes.  Two families of tables:
    exact   every entry a multiple of 1/4 in [-2, 2] (TransE, DistMult, ComplEx): every product and sum is exact in float32 in
            any order, so the float32 and float64 positions of the reference agree (asserted) and ties are plentiful;
    float   entity rows N(0, 0.5^2), relation rows uniform in the model's embedding_range (all four models).
One entity table per family serves all models (the narrow ones take its first 24 columns).
Recorded: the tables; the triples; per (model, family, mode) the reference's 0-based positions from its own
model((positive, negative), mode) + filter_bias and argsort, from the float32 model (pos_f32_*) and from the same model in
float64 (pos_f64_*); ref_err_* = max |score_f32 - score_f64|; the float32 scores of the first 16 test triples (scores_f32_*);
for DistMult and ComplEx the query of those 16 triples as the reference's own score() forms it, read out through unit-vector
candidates (q_ref_*; TransE and RotatE put a norm between their intermediate and everything they return, so they expose none);
per mode the candidates TestDataset's filter_bias marks with -1, bit-packed (filter_bias_*).  Asserted while writing: the numpy
restatement of tests/_kgrank_cases.py equals the reference's float64 scores to 1e-12, and in every float case at most 5 % of
the triples are ambiguous under the tests' bracket.  Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "/root/reference")
MAX_BYTES = 400_000


def main():
    import torch

    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    from cogdl.datasets.kg_data import TestDataset
    from cogdl.models.emb.complex import ComplEx
    from cogdl.models.emb.distmult import DistMult
    from cogdl.models.emb.rotate import RotatE
    from cogdl.models.emb.transe import TransE

    import _kgrank_cases as C

    classes = {"transe": TransE, "distmult": DistMult, "complex": ComplEx, "rotate": RotatE}
    rng = np.random.RandomState(20261)
    seen = set()
    while len(seen) < C.NUM_TRUE:
        seen.add((int(rng.randint(C.N)), int(rng.randint(C.NUM_RELS)), int(rng.randint(C.N))))
    true = sorted(seen)
    rng.shuffle(true)
    true = [tuple(t) for t in true]
    test = true[:C.NUM_TEST]
    out = {"true_triples": np.asarray(true, dtype=np.int16), "test_triples": np.asarray(test, dtype=np.int16)}
    out["entity_exact"] = (rng.randint(-8, 9, size=(C.N, 2 * C.HIDDEN)) / 4.0).astype(np.float32)
    out["entity_float"] = (rng.standard_normal((C.N, 2 * C.HIDDEN)) * 0.5).astype(np.float32)
    samples = {}
    for mode in C.MODES:
        ds = TestDataset(test, true, C.N, C.NUM_RELS, mode)
        items = [ds[i] for i in range(len(ds))]
        pos, neg, bias, _ = TestDataset.collate_fn(items)
        samples[mode] = (pos, neg, bias)
        out["filter_bias_" + mode.split("-")[0]] = np.packbits(bias.numpy() == -1, axis=1)
    triples = np.asarray(test, dtype=np.int64)
    for model_name, family in C.CASES:
        rel_dim = C.HIDDEN * (2 if C.DOUBLE_RELATION[model_name] else 1)
        if family == "exact":
            rel = (rng.randint(-8, 9, size=(C.NUM_RELS, rel_dim)) / 4.0).astype(np.float32)
        else:
            rel = rng.uniform(-C.EMBEDDING_RANGE, C.EMBEDDING_RANGE, size=(C.NUM_RELS, rel_dim)).astype(np.float32)
        out["relation_%s_%s" % (model_name, family)] = rel
        ent, _ = C.tables(out, model_name, family)
        model = classes[model_name](C.N, C.NUM_RELS, C.HIDDEN, C.GAMMA, C.DOUBLE_ENTITY[model_name], C.DOUBLE_RELATION[model_name])
        assert abs(model.embedding_range.item() - C.EMBEDDING_RANGE) == 0 and model.gamma.item() == C.GAMMA
        with torch.no_grad():
            model.entity_embedding.copy_(torch.from_numpy(ent))
            model.relation_embedding.copy_(torch.from_numpy(rel))
        model64 = classes[model_name](C.N, C.NUM_RELS, C.HIDDEN, C.GAMMA, C.DOUBLE_ENTITY[model_name],
                                      C.DOUBLE_RELATION[model_name]).double()
        model64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
        for mode in C.MODES:
            pos, neg, bias = samples[mode]
            target = pos[:, 0] if mode == "head-batch" else pos[:, 2]
            got = {}
            with torch.no_grad():
                for name, mdl, b in (("f32", model, bias), ("f64", model64, bias.double())):
                    score = mdl((pos, neg), mode)
                    assert score.dtype == (torch.float32 if name == "f32" else torch.float64)
                    argsort = torch.argsort(score + b, dim=1, descending=True)
                    where = (argsort == target.view(-1, 1)).nonzero()
                    assert where.shape[0] == len(test)
                    got[name] = (score, where[:, 1].numpy())
            key = C.tag(model_name, family, mode)
            s32, s64 = got["f32"][0].numpy(), got["f64"][0].numpy()
            left_out = bias.numpy() == -1
            # (the reference scores a filtered candidate as a second copy of the target: compare where it scores the candidate)
            mine, tgt = C.model_scores64(model_name, mode, ent, rel, triples)
            assert np.array_equal(tgt, target.numpy())
            assert np.abs(mine - s64)[~left_out].max() <= 1e-12, (key, np.abs(mine - s64)[~left_out].max())
            ref_err = float(np.abs(s32.astype(np.float64) - s64).max())
            out["pos_f32_" + key] = got["f32"][1].astype(np.int16)
            out["pos_f64_" + key] = got["f64"][1].astype(np.int16)
            out["ref_err_" + key] = np.asarray(ref_err)
            out["scores_f32_" + key] = s32[:C.SCORE_ROWS]
            if C.KIND[model_name] == "dot":
                # The query as the reference itself forms it: its score() against the D unit vectors as candidates.  Every
                # product with a 0 is 0 and the sum of one value and zeros is that value, so the [rows, D] result is the
                # reference's intermediate bit for bit.  (The two distance models expose no such view: a norm stands between
                # the intermediate and anything score() returns.)
                fixed = C.fixed_free(mode)[0]
                rows = torch.from_numpy(ent[triples[:C.SCORE_ROWS, fixed]]).unsqueeze(1)
                rels = torch.from_numpy(rel[triples[:C.SCORE_ROWS, 1]]).unsqueeze(1)
                units = torch.eye(ent.shape[1]).unsqueeze(0).expand(C.SCORE_ROWS, -1, -1)
                with torch.no_grad():
                    q_ref = model.score(units, rels, rows, mode) if mode == "head-batch" else model.score(rows, rels, units, mode)
                assert tuple(q_ref.shape) == (C.SCORE_ROWS, ent.shape[1]) and q_ref.dtype == torch.float32
                out["q_ref_" + key] = q_ref.numpy()
            lo, hi = C.bracket64(mine, tgt, left_out, C.delta_of(ref_err, mine))
            frac = float((lo != hi).mean())
            agree = int((got["f32"][1] == got["f64"][1]).sum())
            print("%-28s ref_err %.3e  ambiguous %5.2f %%  f32 == f64 positions on %d / %d" % (key, ref_err, 100 * frac, agree,
                                                                                              len(test)))
            if family == "exact":
                assert ref_err == 0.0 and agree == len(test), key
            else:
                assert frac <= C.AMBIGUOUS_CAP, (key, frac)
    path = os.path.join(HERE, "kg_rank.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < MAX_BYTES, size
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
