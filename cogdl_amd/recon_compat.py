"""The reference's graph auto-encoders on this library's inner-product decoder loss (cogdl_amd/operators/recon.py):
`install(recon=True)` binds `VGAE.make_loss` (cogdl/models/nn/gae.py:76-84), `DAEGC.recon_loss` (cogdl/models/nn/daegc.py:82-84)
and `GAEModelWrapper.pre_stage` (cogdl/wrappers/model_wrapper/clustering/gae_mw.py:38-46).

What changes: F.binary_cross_entropy(sigmoid(z z^T), adj, reduction="sum") against the [N, N] float32 matrix the wrapper
densifies is one `inner_product_bce(z, row, col)` call over the edges: nothing of size [N, N] exists, forward or backward.
  VGAE.make_loss(data, adj=None)   the encoder, the reparameterisation and the KL term are the reference's lines; `adj` is
      ignored.  The edges are `data.recon_index` where the served pre_stage left it, else data.edge_index as it stands BEFORE
      encode() -- which adds the missing self loops to the graph in place, while the reference's adj_mx is built once from the
      edges of stage 0.  The reference's print of the two terms (a device read-back per step) is left out.
  DAEGC.recon_loss(z, adj=None, edge_index=None)   with adj absent or None and edge_index = (row, col) given it is the operator;
      a dense adj reaches the reference's method.
  GAEModelWrapper.pre_stage   for a VGAE at stage 0: data.adj_mx = None and data.recon_index = the [2, E] edges as they stand
      (an attribute the graph moves between devices with its others).  Any other model gets the reference's method: GAE.make_loss
      has a row-softmax link, which the operator does not compute.
Deviations from the reference's numbers: INTEGRATION.md (no clamp of the logs at -100, another summation order).
"""
import sys

import torch

from . import _rebind
from .operators.recon import inner_product_bce

_MODEL, _DAEGC, _WRAPPER = "cogdl.models.nn.gae", "cogdl.models.nn.daegc", "cogdl.wrappers.model_wrapper.clustering.gae_mw"
MODULES = (_MODEL, _DAEGC, _WRAPPER)


def make_loss(self, data, adj=None):
    index = getattr(data, "recon_index", None)
    row, col = data.edge_index if index is None else index
    mean, log_var = self.encode(data)
    z = self.reparameterize(mean, log_var)
    recon_loss = inner_product_bce(z, row, col)
    var = torch.exp(log_var)
    kl_loss = 0.5 * torch.mean(torch.sum(mean * mean + var - log_var - 1, dim=1))
    return recon_loss + kl_loss


def recon_loss(self, z, adj=None, edge_index=None):
    if adj is not None or edge_index is None:
        return _rebind.original(sys.modules[_DAEGC].DAEGC, "recon_loss")(self, z, adj)
    return inner_product_bce(z, *edge_index)


def pre_stage(self, stage, data_w):
    if not isinstance(self.model, sys.modules[_MODEL].VGAE):
        return _rebind.original(sys.modules[_WRAPPER].GAEModelWrapper, "pre_stage")(self, stage, data_w)
    if stage == 0:
        data = data_w.get_dataset().data
        data.recon_index = torch.stack(data.edge_index)
        data.adj_mx = None


def install():
    _rebind.put("recon", sys.modules[_MODEL].VGAE, "make_loss", make_loss)
    _rebind.put("recon", sys.modules[_DAEGC].DAEGC, "recon_loss", recon_loss)
    _rebind.put("recon", sys.modules[_WRAPPER].GAEModelWrapper, "pre_stage", pre_stage)
    return True
