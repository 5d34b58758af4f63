"""The reference's GRACE wrapper on this library's pairwise log-sum-exp (cogdl_amd/operators/contrast.py):
`install(contrast=True)` binds `GRACEModelWrapper.contrastive_loss` (cogdl/wrappers/model_wrapper/node_classification/
grace_mw.py:64-77).

What changes: the two [N, N] float32 matrices exp(z1 z1^T / tau) and exp(z1 z2^T / tau), their row sums, the diagonal and
everything autograd keeps of them are one `grace_loss` call: the normalisation, then one operator that works in row blocks and
recomputes the scores in its backward, so what it keeps is O(N d).  The diagonal term is left out of the row sum instead of being
subtracted from it, and the sums go through logsumexp, so they are re-associated against the reference's: the same numbers up to
float32 rounding, not the same bits -- and finite where the reference's plain exp overflows (tau below about 0.0113).  The
operator is a torch composition: no HIP kernel serves it, on the GPU it runs torch's kernels (one TorchRouteWarning).

What does not: `batched_loss` (lines 79-91) calls `self.contrastive_loss(z1[idx], z2)` and is served as it stands; `train_step`
and everything else are the reference's.  Inputs that are not 2-D floating tensors of one width, dtype and device reach the
reference's own method (cogdl_amd/_rebind.original), whatever it does with them.
"""
import sys

import torch

from . import _rebind
from .operators.contrast import grace_loss

_MODULE, _CLASS = "cogdl.wrappers.model_wrapper.node_classification.grace_mw", "GRACEModelWrapper"


def _served(z1, z2):
    return (torch.is_tensor(z1) and torch.is_tensor(z2) and z1.dim() == 2 and z2.dim() == 2 and z1.shape[1] == z2.shape[1]
            and z1.shape[1] >= 1 and z1.shape[0] >= 1 and z1.is_floating_point() and z1.dtype == z2.dtype
            and z1.device == z2.device)


def contrastive_loss(self, z1, z2):
    if not _served(z1, z2):
        return _rebind.original(getattr(sys.modules[_MODULE], _CLASS), "contrastive_loss")(self, z1, z2)
    return grace_loss(z1, z2, self.tau)


def install():
    _rebind.put("contrast", getattr(sys.modules[_MODULE], _CLASS), "contrastive_loss", contrastive_loss)
    return True
