"""The reference's GRACE wrapper on this library's pairwise log-sum-exp (cogdl_amd/operators/contrast.py):
`install(contrast=True)` binds `GRACEModelWrapper.contrastive_loss` (cogdl/wrappers/model_wrapper/node_classification/
grace_mw.py:64-77).

What changes: the two [N, N] float32 matrices exp(z1 z1^T / tau) and exp(z1 z2^T / tau), their row sums, the diagonal and
everything autograd keeps of them are one `grace_loss` call: the normalisation, then one operator that works in row blocks and
recomputes the scores in its backward, so what it keeps is O(N d).  The diagonal term is left out of the row sum instead of being
subtracted from it, and the sums go through logsumexp, so they are re-associated against the reference's: the same numbers up to
float32 rounding, not the same bits -- and finite where the reference's plain exp overflows (tau below about 0.0113).  On
float32 GPU tensors with d <= 256 grace_loss runs the streaming MFMA kernels of csrc/contrast.hip, except at the sizes where
they measured slower than the blocked torch composition (profiles/contrast_bench.txt); everything else runs that composition,
on the GPU with one TorchRouteWarning.  Under torch.autocast for the GPU, float32 and 16-bit inputs with d <= 256 are normalised in
float32, cast once to the autocast dtype and run on the fp16 / bf16 kernels of csrc/contrast16.hip (v_mfma_f32_32x32x16) at the
sizes where those measured no slower; the loss is float32 and the gradients come back in the inputs' own dtype.

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
    if z1.is_cuda and torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() in (torch.float16, torch.bfloat16):
        # torch AMP (the Trainer's fp16=True): whatever dtype the projection head handed over, the rows are normalised in float32,
        # cast once to the autocast dtype for this one call and run on the 16-bit kernels; the loss is float32 and the gradient
        # reaches z1, z2 in their own dtype through the cast.  Outside autocast nothing is cast.
        return grace_loss(z1, z2, self.tau, cast=torch.get_autocast_gpu_dtype())
    return grace_loss(z1, z2, self.tau)


def install():
    _rebind.put("contrast", getattr(sys.modules[_MODULE], _CLASS), "contrastive_loss", contrastive_loss)
    return True
