"""Writes tests/golden/genconv_layer.npz: one small graph, the parameters of two reference GENConv layers (`plain`: no edge
encoder; `enc`: an EdgeEncoder over 5 edge attributes) and what the reference's own CPU path computes on them in float32.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs, and
NOT rebound: the per-column CPU softmax of cogdl/utils/spmm_utils.py:149-188 runs on the reference's own spmm, on the torch
route of its dispatcher (spmm_scatter, spmm_utils.py:43-52,120-122), which is what the reference runs wherever its C++ spmm_cpu
is not built.  Where that extension IS built the dispatcher calls it as a raw function outside autograd (spmm_utils.py:110-116:
the softmax's denominator is spmm(graph, ones), and ones does not require grad), so the gradient through the denominator is
dropped and grad_x / grad_beta / grad_enc_weight come out O(1) away from the softmax's gradient; the reference's GPU path
(csr_edge_softmax) and its torch route carry the full gradient, and so does this recording.  CPU only.

N = 40 nodes, F = 12, 200 edges (the last 4 nodes receive nothing), the graph holding its CSR before the layer runs;
GENConv(12, 12, aggr="softmax_sg", beta=1.5, learn_beta=True, use_msg_norm=True, learn_msg_scale=True, residual=True,
activation="relu"), loss sum(out * G).  Recorded: the inputs in the graph's (CSR) edge order (x, row, col, edge_attr, G), per
layer the parameters <tag>_<param>, the float32 results <tag>_<name>_f32 (output and every gradient), the float64 oracle
<tag>_<name>_f64 -- the same layer rebuilt on the torch composition (tests/_genconv_layer.py, CPU route) in float64 on the same
float32 values; the reference's CPU softmax itself cannot run in float64, its spmm takes float32 only -- and
ref_err_<tag>_<name> = max |f32 - f64|, the yardstick of tests/test_genconv_layer_gpu.py.  max beta * m is asserted <= 10, so
the reference's halving loop (spmm_utils.py:157-160) stayed out.  Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "")
N, F, E, A, BETA = 40, 12, 200, 5, 1.5
MAX_BYTES = 200_000
STATE = {"beta": "beta", "s": "s", "mlp0_weight": "mlp.mlp.0.weight", "mlp0_bias": "mlp.mlp.0.bias",
         "mlp1_weight": "mlp.mlp.1.weight", "mlp1_bias": "mlp.mlp.1.bias", "enc_weight": "edge_encoder.nn.weight"}


def main():
    import torch

    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "cogdl")):
        raise SystemExit("set COGDL_REFERENCE to a checkout of the reference package")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    from cogdl.data import Graph
    from cogdl.layers.deepergcn_layer import GENConv
    from cogdl.utils import spmm_utils

    spmm_utils.CONFIGS["spmm_cpu_flag"], spmm_utils.CONFIGS["fast_spmm_cpu"] = True, None  # the dispatcher's torch route

    import _genconv_layer as L

    torch.manual_seed(20252)
    row, col = torch.randint(0, N - 4, (E,)), torch.randint(0, N, (E,))
    x, attr, G = torch.randn(N, F) * 0.8, torch.randn(E, A) * 0.5, torch.randn(N, F)
    graph = Graph(x=x, edge_index=torch.stack([row, col]), edge_attr=attr)
    graph.row_indptr  # the CSR is built (and the edges, with their attributes, re-sorted) before the layer runs
    row, col = graph.edge_index
    out = {"x": x, "row": row, "col": col, "edge_attr": graph.edge_attr, "G": G}
    for tag, enc in L.TAGS.items():
        layer = GENConv(F, F, aggr="softmax_sg", beta=BETA, learn_beta=True, use_msg_norm=True, learn_msg_scale=True,
                        residual=True, activation="relu", edge_attr_size=[A] if enc else None).train()
        with torch.no_grad():
            layer.s.fill_(0.7)
        state = layer.state_dict()
        for k, name in STATE.items():
            if name in state:
                out["%s_%s" % (tag, k)] = state[name].detach().clone()
        if not enc:
            graph.edge_attr = None
        else:
            graph.edge_attr = out["edge_attr"]
        xa = x.clone().requires_grad_()
        y = layer(graph, xa)
        (y * G).sum().backward()
        with torch.no_grad():
            m = xa[col] + (layer.edge_encoder(out["edge_attr"]) if enc else 0)
            assert float(BETA * (torch.relu(m) + layer.eps).max()) <= 10
        got = {"out": y.detach(), "grad_x": xa.grad}
        params = dict(layer.named_parameters())
        for k, name in STATE.items():
            if name in params:
                got["grad_" + k] = params[name].grad
        assert sorted(got) == sorted(L.names(tag)), sorted(got)
        for name in L.names(tag):
            assert got[name].dtype == torch.float32
            out["%s_%s_f32" % (tag, name)] = got[name].detach().clone()
    out = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    print("%-28s %12s %12s" % ("max |. - float64 oracle|", "reference", "gen_aggregate"))
    for tag in L.TAGS:
        oracle = L.rebuilt_layer(out, tag, "cpu", torch.float64)
        ours = L.rebuilt_layer(out, tag, "cpu")
        for name in L.names(tag):
            out["%s_%s_f64" % (tag, name)] = oracle[name].numpy()
            err = float(np.abs(out["%s_%s_f32" % (tag, name)].astype(np.float64) - out["%s_%s_f64" % (tag, name)]).max())
            out["ref_err_%s_%s" % (tag, name)] = np.asarray(err)
            print("%-28s %12.3e %12.3e" % (tag + " " + name, err, float((ours[name].double() - oracle[name]).abs().max())))
    path = os.path.join(HERE, "genconv_layer.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < MAX_BYTES, size
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
