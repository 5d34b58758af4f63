"""The reference's knowledge-graph embedding training step on the sampled scoring operator: `install(kg_train=True)` binds
`KGEModel.forward` (cogdl/models/emb/knowledge_base.py:52-101), which TripleModelWrapper.train_step calls twice per step (the
negative scores [B, K] of one mode, the positive scores [B, 1]) for transe, distmult, complex and rotate.

What changes.  forward no longer index_selects a [B, K, D] copy of the entity table and broadcasts the model's score() over it:
it calls cogdl_amd.kgtrain.score_triples -- the [B, D] query with the reference's expressions, then one sampled_scores against
`entity_embedding` -- and returns the same [B, K] / [B, 1] tensor, float32 rounding apart (the sums are re-associated).  The
gradient of `entity_embedding` is a sum in a fixed order instead of an atomic scatter: equal from run to run.

What does not change: the loss, the self-adversarial softmax and the L3 regulariser are the reference's torch code on [B, K];
a model that is not a TransE, DistMult, ComplEx or RotatE instance with that class's own `score` (kgrank_compat._model_kind)
reaches the reference's forward, and so does an unknown mode, which raises the reference's ValueError
(cogdl_amd/_rebind.original).
"""
import sys

from . import _rebind
from .kgrank_compat import _MODELS, _model_kind

_MODULE = "cogdl.models.emb.knowledge_base"
_MODES = ("single", "head-batch", "tail-batch")


def forward(self, sample, mode="single"):
    kind = _model_kind(self)
    if kind is None or mode not in _MODES:
        return _rebind.original(getattr(sys.modules[_MODULE], "KGEModel"), "forward")(self, sample, mode)
    from .kgtrain import score_triples

    return score_triples(kind, self.entity_embedding, self.relation_embedding, sample, mode, self.embedding_range.item(),
                         self.gamma.item())


def install():
    _rebind.put("kg_train", sys.modules[_MODULE].KGEModel, "forward", forward)
    return True
