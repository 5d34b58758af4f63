"""Writes tests/golden/compgcn_layer.npz: one small typed graph, the parameters of a reference CompGCNLayer and what the layer
computes on them, in float32 and in float64.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs.
CPU only.

N = 300 entities, 5 relations plus their reverses, 1500 edges per direction (the second half of the edge list is the first
half reversed, types + 5, as the link-prediction wrapper builds it), 12 -> 20, dropout 0, bias, train-mode BatchNorm, identity
activation; `opn` sub and mult on the same inputs and parameters.  Recorded: the inputs (x, rel_embed, row, col, etype), the
two edge normalisations the layer computes (in_norm, rev_norm), the parameters, the upstream gradients G_out / G_rel of the
loss sum(out * G_out) + sum(rel_out * G_rel), and per opn the layer's two outputs and the gradients with respect to x,
rel_embed and the four weights -- <opn>_<name>_f32 from the float32 layer, <opn>_<name>_f64 from the same layer run in
float64 (default dtype float64, the same parameter values).  ref_err_<opn>_<name> = max |f32 - f64|, the reference's own
float32 error: the yardstick of tests/test_relational_layer_gpu.py.  cpu_err_<opn>_<name> = the same distance for the layer
rebuilt on rel_gspmm (tests/_relational_layer.py) on the CPU, for the record.  Only arrays are stored."""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "/root/reference")
N, NUM_RELS, EDGES, IN, OUT = 300, 5, 1500, 12, 20
MAX_BYTES = 400_000


def main():
    import torch

    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    from cogdl.models.nn.compgcn import CompGCNLayer
    from cogdl.utils import row_normalization

    import _relational_layer as L

    torch.manual_seed(20251)
    src, dst = torch.randint(0, N, (EDGES,)), torch.randint(0, N - 30, (EDGES,))  # (the last 30 entities receive nothing)
    typ = torch.randint(0, NUM_RELS, (EDGES,))
    row, col, etype = torch.cat([dst, src]), torch.cat([src, dst]), torch.cat([typ, typ + NUM_RELS])
    x, rel_embed = torch.randn(N, IN), torch.randn(2 * NUM_RELS, IN)
    g_out, g_rel = torch.randn(N, OUT), torch.randn(2 * NUM_RELS, OUT)
    out = {"x": x, "rel_embed": rel_embed, "row": row, "col": col, "etype": etype, "G_out": g_out, "G_rel": g_rel,
           "in_norm": row_normalization(N, row[:EDGES], col[:EDGES]), "rev_norm": row_normalization(N, row[EDGES:], col[EDGES:])}
    state = None
    for opn in L.OPNS:
        runs = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            torch.set_default_dtype(dtype)  # (the layer allocates its zeros and ones in the default dtype)
            try:
                layer = CompGCNLayer(IN, OUT, NUM_RELS, opn=opn, dropout=0.0, bias=True).train()
                if state is None:  # one set of parameters for every run; a bias and a BatchNorm that are not the identity
                    with torch.no_grad():
                        layer.bias.normal_(0, 0.5)
                        layer.bn.weight.uniform_(0.5, 1.5)
                        layer.bn.bias.normal_(0, 0.5)
                    state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
                layer.load_state_dict(state)
                xa, ra = x.clone().to(dtype).requires_grad_(), rel_embed.clone().to(dtype).requires_grad_()
                graph = types.SimpleNamespace(edge_index=(row, col), edge_attr=etype)
                y, rel_out = layer(graph, xa, ra)
                ((y * g_out.to(dtype)).sum() + (rel_out * g_rel.to(dtype)).sum()).backward()
                runs[tag] = {"out": y, "rel_out": rel_out, "grad_x": xa.grad, "grad_rel_embed": ra.grad}
                for w in ("weight_in", "weight_out", "weight_loop", "weight_rel"):
                    runs[tag]["grad_" + w] = getattr(layer, w).grad
                runs[tag] = {k: v.detach().clone() for k, v in runs[tag].items()}
            finally:
                torch.set_default_dtype(torch.float32)
        for name in L.NAMES:
            assert runs["f32"][name].dtype == torch.float32 and runs["f64"][name].dtype == torch.float64, name
            out["%s_%s_f32" % (opn, name)] = runs["f32"][name]
            out["%s_%s_f64" % (opn, name)] = runs["f64"][name]
            out["ref_err_%s_%s" % (opn, name)] = (runs["f32"][name].double() - runs["f64"][name]).abs().max()
    for k, name in (("bias", "bias"), ("bn_weight", "bn.weight"), ("bn_bias", "bn.bias")):
        out[k] = state[name]
    for k in ("weight_in", "weight_out", "weight_rel", "weight_loop", "loop_rel"):
        out[k] = state[k]
    out = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    print("%-28s %12s %12s" % ("max |. - float64 reference|", "reference", "rel_gspmm"))
    for opn in L.OPNS:
        ours = L.rebuilt_layer(out, opn, "cpu")
        for name in L.NAMES:
            err = float((ours[name].double() - torch.from_numpy(out["%s_%s_f64" % (opn, name)])).abs().max())
            out["cpu_err_%s_%s" % (opn, name)] = np.asarray(err)
            print("%-28s %12.3e %12.3e" % (opn + " " + name, float(out["ref_err_%s_%s" % (opn, name)]), err))
    path = os.path.join(HERE, "compgcn_layer.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < MAX_BYTES, size
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
