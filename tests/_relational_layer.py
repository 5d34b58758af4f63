"""The CompGCN layer of tests/golden/compgcn_layer.npz rebuilt on rel_gspmm: the layer math of
cogdl/models/nn/compgcn.py:94-140 with the direction's weight behind the typed aggregation.  Shared by the generator
(tests/golden/make_golden_relational.py, CPU route) and tests/test_relational_layer_gpu.py."""
import torch
import torch.nn.functional as F

OPNS = {"sub": "sub", "mult": "mul"}  # the layer's opn -> rel_gspmm's op
PARAMS = ("weight_in", "weight_out", "weight_rel", "weight_loop", "loop_rel", "bias", "bn_weight", "bn_bias")
NAMES = ("out", "rel_out", "grad_x", "grad_rel_embed", "grad_weight_in", "grad_weight_out", "grad_weight_loop", "grad_weight_rel")


def rebuilt_layer(z, opn, device):
    """z: the golden arrays -> {name: float32 tensor on the CPU} for NAMES (train-mode BatchNorm, dropout 0, identity
    activation; the loss is sum(out * G_out) + sum(rel_out * G_rel))."""
    from cogdl_amd.operators.relational import rel_gspmm

    t = {k: torch.from_numpy(z[k]).to(device) for k in ("x", "rel_embed", "row", "col", "etype", "in_norm", "rev_norm", "G_out",
                                                         "G_rel") + PARAMS}
    leaves = {k: t[k].clone().requires_grad_() for k in ("x", "rel_embed", "weight_in", "weight_out", "weight_loop", "weight_rel")}
    x, n, half = leaves["x"], t["x"].shape[0], t["row"].numel() // 2
    rel = torch.cat((leaves["rel_embed"], t["loop_rel"]), dim=0)
    loop = torch.arange(n, device=device)
    loop_types = torch.full((n,), rel.shape[0] - 1, dtype=torch.long, device=device)
    op = OPNS[opn]
    emb = rel_gspmm(x, rel, t["row"][:half], t["col"][:half], t["etype"][:half], t["in_norm"], op) @ leaves["weight_in"]
    rev = rel_gspmm(x, rel, t["row"][half:], t["col"][half:], t["etype"][half:], t["rev_norm"], op) @ leaves["weight_out"]
    own = rel_gspmm(x, rel, loop, loop, loop_types, None, op) @ leaves["weight_loop"]
    out = 1 / 3 * (emb + rev + own) + t["bias"]
    out = F.batch_norm(out, None, None, t["bn_weight"], t["bn_bias"], True, 0.1, 1e-5)
    rel_out = torch.matmul(rel, leaves["weight_rel"])[:-1]
    ((out * t["G_out"]).sum() + (rel_out * t["G_rel"]).sum()).backward()
    got = {"out": out, "rel_out": rel_out, "grad_x": x.grad, "grad_rel_embed": leaves["rel_embed"].grad}
    for w in ("weight_in", "weight_out", "weight_loop", "weight_rel"):
        got["grad_" + w] = leaves[w].grad
    return {k: v.detach().float().cpu() for k, v in got.items()}
