"""The reference's knowledge-graph link-prediction evaluation on the ranking operator: `install(kg_eval=True)` binds
`TripleModelWrapper.eval_step` (cogdl/wrappers/model_wrapper/link_prediction/triple_link_prediction_mw.py:84-132: transe,
distmult, complex, rotate) and `cal_mrr` (cogdl/utils/link_prediction_utils.py:8-28, with its by-name copy in
cogdl.wrappers.model_wrapper.link_prediction.gnn_kg_link_prediction_mw: compgcn, rgcn).

What changes.  eval_step no longer iterates the two loaders (each item of which walks all entities in Python,
cogdl/datasets/kg_data.py:48-72): it reads `.dataset.triples`, `.triple_set`, `.mode` and `.nentity`, builds the filter lists
once per dataset object with torch sort / unique (memoised on the object), and ranks all triples of a direction with one
prepare_query + rank_all against the whole entity table -- no [B, N, D] gather, no [B, N] sort, no `.item()` per triple.  It
returns the same dict of MRR / MR / HITS@1/3/10.  cal_mrr ranks with DistMultLayer's score as kind "dot" on
q = emb[heads] * rel[rels]; protocol "raw" as the reference, and protocol "filtered" -- which the reference leaves as
NotImplementedError -- when the new optional `seen_triples` argument says what to leave out; without it "filtered" raises as
before.  The return types are the reference's: a numpy float and a list.  cal_mrr has no object to keep lists on: with
protocol "filtered" it builds them on every call, once per direction (torch sort / unique on the device of the embedding).

Ties.  Both report the target's rank as 1 + greater + equal_before (ties="stable").  The reference's position among equal
scores is whatever its sort does, so the two agree exactly where no candidate ties with the target and lie inside the same
bracket [greater, greater + equal] otherwise.  cal_mrr's reference ranks sigmoid(score): the sigmoid is monotone, so it
changes no strict order the other way round -- it only merges distinct scores into ties (float32 saturates); the raw-score
rank therefore always lies inside the reference's own tie bracket.

What does not change: a model that is not a TransE, DistMult, ComplEx or RotatE instance with that class's own `score`
reaches the reference's eval_step; a scoring layer that is not DistMultLayer (ConvELayer) reaches the reference's cal_mrr
(cogdl_amd/_rebind.original).
"""
import sys

import torch

from . import _rebind

_WRAPPER = "cogdl.wrappers.model_wrapper.link_prediction.triple_link_prediction_mw"
_UTILS = "cogdl.utils.link_prediction_utils"
_HOLDER = "cogdl.wrappers.model_wrapper.link_prediction.gnn_kg_link_prediction_mw"
_MODELS = (("transe", "cogdl.models.emb.transe", "TransE"), ("distmult", "cogdl.models.emb.distmult", "DistMult"),
           ("complex", "cogdl.models.emb.complex", "ComplEx"), ("rotate", "cogdl.models.emb.rotate", "RotatE"))
_MEMO = "_cogdl_amd_kg_eval"


def _model_kind(model):
    for kind, modname, clsname in _MODELS:
        cls = getattr(sys.modules.get(modname), clsname, None)
        if cls is not None and isinstance(model, cls) and type(model).score is cls.score:
            return kind
    return None


def _dataset_lists(dataset, device):
    """(triples [M, 3], filt_ptr, filt_idx) on `device`, built once per dataset object, device, mode and the sizes of
    `.triples` and `.triple_set`: a dataset that grows or shrinks gets new lists; one whose triples are replaced by as many
    others keeps the old ones (the reference's TestDataset is not written to after construction) -- delete the attribute
    `_cogdl_amd_kg_eval` of the dataset to force a rebuild."""
    from .kgrank import filter_lists

    memo = dataset.__dict__.setdefault(_MEMO, {})
    key = (str(device), dataset.mode, len(dataset.triples), len(dataset.triple_set))
    hit = memo.get(key)
    if hit is None:
        memo.clear()  # (one entry per dataset: the lists of another size are of no further use)
        triples = torch.tensor(list(dataset.triples), dtype=torch.int64).reshape(-1, 3).to(device)
        seen = torch.tensor(sorted(dataset.triple_set), dtype=torch.int64).reshape(-1, 3).to(device)
        hit = memo[key] = (triples,) + filter_lists(seen, triples, dataset.mode, dataset.nentity)
    return hit


def eval_step(self, subgraph):
    kind = _model_kind(self.model)
    if kind is None:
        return _rebind.original(getattr(sys.modules[_WRAPPER], "TripleModelWrapper"), "eval_step")(self, subgraph)
    from .kgrank import evaluate, kg_metrics

    model, counts = self.model, []
    entity, relation = model.entity_embedding.detach(), model.relation_embedding.detach()
    with torch.no_grad():
        for loader in subgraph:
            dataset = loader.dataset
            if dataset.mode not in ("head-batch", "tail-batch"):
                raise ValueError("mode %s not supported" % dataset.mode)
            triples, filt_ptr, filt_idx = _dataset_lists(dataset, entity.device)
            counts.append(evaluate(kind, entity, relation, triples, dataset.mode, model.embedding_range.item(), model.gamma.item(),
                                   filt_ptr, filt_idx))
    metrics = kg_metrics(counts, "stable", hits=(1, 3, 10))
    print("The Dataset metrics:", metrics)
    return metrics


def _seen_as_triples(seen_triples, device):
    """-> int64 [T, 3] of (head, relation, tail).  Accepted: (edge_index, edge_type) as cal_mrr's own arguments give them, or a
    [T, 3] tensor / array of (head, relation, tail)."""
    if isinstance(seen_triples, (tuple, list)) and len(seen_triples) == 2:
        (row, col), etype = seen_triples
        return torch.stack([torch.as_tensor(row).long(), torch.as_tensor(etype).long(), torch.as_tensor(col).long()], dim=1).to(device)
    seen = torch.as_tensor(seen_triples).long().to(device)
    if seen.dim() != 2 or seen.shape[1] != 3:
        raise ValueError("cal_mrr: seen_triples must be (edge_index, edge_type) or [T, 3] of (head, relation, tail)")
    return seen


def cal_mrr(embedding, rel_embedding, edge_index, edge_type, scoring, protocol="raw", batch_size=1000, hits=[], seen_triples=None):
    utils = sys.modules[_UTILS]
    if type(scoring) is not utils.DistMultLayer:
        return _rebind.original(utils, "cal_mrr")(embedding, rel_embedding, edge_index, edge_type, scoring, protocol=protocol,
                                                  batch_size=batch_size, hits=hits)
    if protocol == "filtered" and seen_triples is None:
        raise NotImplementedError
    if protocol not in ("raw", "filtered"):
        raise ValueError
    import numpy as np

    from .kgrank import filter_lists
    from .operators.kgrank import rank_all, ranks

    with torch.no_grad():
        embedding, rel_embedding = embedding.detach(), rel_embedding.detach()
        dev, n = embedding.device, embedding.shape[0]
        heads, tails, rels = edge_index[0].to(dev).long(), edge_index[1].to(dev).long(), edge_type.to(dev).long()
        queries = torch.stack([heads, rels, tails], dim=1)
        seen = _seen_as_triples(seen_triples, dev) if protocol == "filtered" else None
        out = []
        # (heads -> tails, then tails -> heads: DistMult's score is symmetric in the two entities, get_raw_rank is called twice)
        for fixed, target, mode in ((heads, tails, "tail-batch"), (tails, heads, "head-batch")):
            filt = filter_lists(seen, queries, mode, n) if seen is not None else (None, None)
            counts = rank_all(embedding[fixed] * rel_embedding[rels], embedding, target, "dot", 0.0, *filt)
            out.append(ranks(counts, "stable"))
        r = torch.cat(out).cpu().numpy().astype(np.float64)
    mrr = (1.0 / r).mean()
    hits_count = [np.mean((r <= hit).astype(np.float64)) for hit in hits]
    return mrr, hits_count


def install():
    wrapper, utils, holder = sys.modules[_WRAPPER], sys.modules[_UTILS], sys.modules[_HOLDER]
    _rebind.put("kg_eval", wrapper.TripleModelWrapper, "eval_step", eval_step)
    _rebind.put("kg_eval", utils, "cal_mrr", cal_mrr)
    if getattr(holder, "cal_mrr", None) is not None:
        _rebind.put("kg_eval", holder, "cal_mrr", cal_mrr)
    return True
