"""Writes tests/golden/disengcn_layer.npz: two small graphs, the parameters of two reference DisenGCN layers and what the
reference's own CPU path computes on them, in float32 and in float64.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs, and
NOT rebound: DisenGCNLayer.forward (cogdl/layers/disengcn_layer.py:40-91) runs with the reference's per-channel CPU softmax
(cogdl/utils/spmm_utils.py:149-188) on the torch route of its dispatcher (spmm_scatter) -- where the C++ spmm_cpu is built the
dispatcher calls it outside autograd and drops the gradient through the softmax's denominator (the finding recorded in
make_golden_genconv.py), and it takes float32 only.  On the torch route the layer also runs in float64 (default dtype float64:
its torch.ones / torch.zeros follow the default), which is the oracle.  CPU only.

in_feats 10, the graphs holding their CSR before the layer runs; the layers of tests/_disengcn_layer.py: `small` out 24, K 3,
3 iterations on 60 nodes and 420 edges (the last 6 nodes receive nothing); `wide` out 64, K 16, 7 iterations (the model's
default channel count and depth) on 16 nodes and 100 edges (the last 2 receive nothing) -- float64 records do not compress,
and the file is to stay no larger than genconv_layer.npz; tau 1, leaky_relu, a non-zero bias; loss sum(out * G) with the
exactly representable G of _disengcn_layer.upstream (not stored).  Scores are at most 1 / tau = 1, so the halving loop of the
reference's CPU softmax (spmm_utils.py:157-160) stays out.  Recorded: per layer the inputs in the graph's (CSR) edge order
(<tag>_x, <tag>_row, <tag>_col as int32), <tag>_weight, <tag>_bias, the results <tag>_<name>_f32 and <tag>_<name>_f64 (output
and the gradients of x, weight and bias) and ref_err_<tag>_<name> = max |f32 - f64|, the yardstick of
tests/test_disengcn_layer_gpu.py.  Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "")
IN = 10


def main():
    import torch

    if not os.path.isdir(os.path.join(REFERENCE_ROOT, "cogdl")):
        raise SystemExit("set COGDL_REFERENCE to a checkout of the reference package")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    from cogdl.data import Graph
    from cogdl.layers.disengcn_layer import DisenGCNLayer
    from cogdl.utils import spmm_utils

    spmm_utils.CONFIGS["spmm_cpu_flag"], spmm_utils.CONFIGS["fast_spmm_cpu"] = True, None  # the dispatcher's torch route

    import _disengcn_layer as L

    torch.manual_seed(20253)
    out = {}
    for tag, (width, K, iterations) in L.TAGS.items():
        N, E, bare = L.GRAPHS[tag]
        row, col = torch.randint(0, N - bare, (E,)), torch.randint(0, N, (E,))
        x = torch.randn(N, IN)
        layer = DisenGCNLayer(IN, width, K, iterations, tau=L.TAU).train()
        with torch.no_grad():
            layer.bias.copy_(torch.randn(width) * 0.1)
        state = {k: v.detach().clone() for k, v in layer.state_dict().items()}
        G = L.upstream(N, width)
        out.update({tag + "_x": x, tag + "_weight": state["weight"], tag + "_bias": state["bias"]})
        for dtype, suffix in ((torch.float32, "f32"), (torch.float64, "f64")):
            torch.set_default_dtype(dtype)
            try:
                layer = DisenGCNLayer(IN, width, K, iterations, tau=L.TAU).train()
                layer.load_state_dict({k: v.to(dtype) for k, v in state.items()})
                graph = Graph(x=x.to(dtype), edge_index=torch.stack([row, col]))
                graph.row_indptr  # the CSR is built (and the edges re-sorted) before the layer runs
                assert graph._adj.row_ptr is not None
                xa = graph.x.clone().requires_grad_()
                y = layer(graph, xa)
                (y * G.to(dtype)).sum().backward()
            finally:
                torch.set_default_dtype(torch.float32)
            got = {"out": y.detach(), "grad_x": xa.grad, "grad_weight": layer.weight.grad, "grad_bias": layer.bias.grad}
            assert sorted(got) == sorted(L.NAMES) and all(v.dtype == dtype for v in got.values())
            out.update({"%s_%s_%s" % (tag, name, suffix): got[name].clone() for name in L.NAMES})
            out[tag + "_row"], out[tag + "_col"] = (t.int() for t in graph.edge_index)
    out = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    print("%-24s %12s %12s" % ("max |. - float64 record|", "reference", "rebuilt"))
    for tag in L.TAGS:
        ours = L.rebuilt_layer(out, tag, "cpu")
        ours64 = L.rebuilt_layer(out, tag, "cpu", torch.float64)
        for name in L.NAMES:
            f32, f64 = out["%s_%s_f32" % (tag, name)], out["%s_%s_f64" % (tag, name)]
            err = float(np.abs(f32.astype(np.float64) - f64).max())
            out["ref_err_%s_%s" % (tag, name)] = np.asarray(err)
            # the rebuilt layer in float64 is the record to rounding: the two float64 layers compute the same function
            assert float((ours64[name] - torch.from_numpy(f64)).abs().max()) <= 1e-12 * max(1.0, float(np.abs(f64).max()))
            print("%-24s %12.3e %12.3e" % (tag + " " + name, err, float((ours[name].double() - torch.from_numpy(f64)).abs().max())))
    path = os.path.join(HERE, "disengcn_layer.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size <= os.path.getsize(os.path.join(HERE, "genconv_layer.npz")), size
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
