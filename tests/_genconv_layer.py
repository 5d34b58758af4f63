"""The GENConv layer of tests/golden/genconv_layer.npz rebuilt on gen_aggregate: the layer math of
cogdl/layers/deepergcn_layer.py:58-102 (softmax_sg with a learnable beta, message norm with a learnable scale, residual, a
two-layer relu MLP; the edge encoder is one bias-free linear map) with lines 67-93 as one operator call.  Shared by the generator
(tests/golden/make_golden_genconv.py, CPU route, float64 oracle) and tests/test_genconv_layer_gpu.py."""
import torch
import torch.nn.functional as F

TAGS = {"plain": False, "enc": True}  # recorded layer -> does it carry the edge encoder?
PARAMS = ("beta", "s", "mlp0_weight", "mlp0_bias", "mlp1_weight", "mlp1_bias")
ENC = "enc_weight"
EPS = 1e-7


def names(tag):
    return ("out", "grad_x") + tuple("grad_" + p for p in PARAMS + ((ENC,) if TAGS[tag] else ()))


def rebuilt_layer(z, tag, device, dtype=torch.float32):
    """z: the golden arrays -> {name: tensor of `dtype` on the CPU} for names(tag); the loss is sum(out * G)."""
    from cogdl_amd.operators import gen_aggregate

    row, col = (torch.from_numpy(z[k]).to(device) for k in ("row", "col"))
    t = {k: torch.from_numpy(z[k]).to(device=device, dtype=dtype) for k in ("x", "G", "edge_attr")}
    keys = PARAMS + ((ENC,) if TAGS[tag] else ())
    p = {k: torch.from_numpy(z["%s_%s" % (tag, k)]).to(device=device, dtype=dtype).requires_grad_() for k in keys}
    x = t["x"].clone().requires_grad_()
    eterm = F.linear(t["edge_attr"], p[ENC]) if TAGS[tag] else None
    h = gen_aggregate(x, row, col, eterm, "softmax", p["beta"], EPS, num_nodes=x.shape[0])
    h = x + p["s"] * (F.normalize(h, p=2, dim=1) * torch.norm(x, dim=1, p=2).unsqueeze(-1))  # message_norm
    h = h + x                                                                                 # residual
    out = F.linear(torch.relu(F.linear(h, p["mlp0_weight"], p["mlp0_bias"])), p["mlp1_weight"], p["mlp1_bias"])
    (out * t["G"]).sum().backward()
    got = {"out": out, "grad_x": x.grad}
    got.update({"grad_" + k: v.grad for k, v in p.items()})
    return {k: v.detach().cpu() for k, v in got.items()}
