"""Times one DisenGCN layer (in 64 -> K * d, leaky_relu, `iterations` routing steps) on the GPU with its routing as
install(disengcn=True) binds it -- one neighbor_routing call, a disen_route operator per iteration (cogdl_amd/disengcn_compat.py,
csrc/disen.hip) -- against the parent route: the reference package's own DisenGCNLayer.forward under a plain install() (its
K-head edge softmax then runs on this library's csr_edge_softmax; everything else is its torch composition with scatter_add_
atomics).  The reference package is taken from oracle/_ref/pkg (staged by build()) or $COGDL_REFERENCE; where neither is present
only the fused route is timed and the header says so.  Writes profiles/disengcn_bench.txt.

    python tools/disengcn_bench.py [--out profiles/disengcn_bench.txt] [--K 16] [--d 4] [--iterations 7] [--repeats 20] [--rounds 3]

Part 1, accuracy: every case of tests/_disen_cases.py on the GPU, err_new and err_ref against the float64 oracle and the bound
4 err_ref + 8 eps32 max|oracle| of the tests.
Part 2, time and memory: a Cora-shaped graph (2,708 nodes) and the arxiv-shaped graphs of cogdl_amd/synth.py (169,343 nodes,
2.5 M edges; uniform and R-MAT), forward and forward + backward of the layer.  Device events around one step; per round
`--warmup` steps, then the median of `--repeats`; the two routes alternate inside a round and the table gives the median round
with the range over the rounds.  Peak memory: the peak of torch's allocator over one step above what is allocated before it.
For the fused route the table also gives the bytes the routing needs per step (computed from the shapes, below) over the step
time: a rate of the whole layer step, matmul included, not a kernel's share of peak.  Before anything is timed the two routes
are compared on the same inputs."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cogdl_amd  # noqa: E402
from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators.disen import neighbor_routing  # noqa: E402

IN = 64


def algorithmic_bytes(n, e, K, d, iterations, backward):
    """Per routing step.  Forward: colind + one source row per edge, rowptr, c and z read, out, nrm and lse written.  Backward:
    the g_c pass like the forward (ga, lse, dl rows instead of the outputs), the g_z pass dst ids + the c and ga rows and the
    lse, dl entries of the destination per edge."""
    f = K * d
    fwd = 4 * e + 4 * f * e + 4 * (n + 1) + 3 * 4 * f * n + 2 * 4 * K * n
    bwd_c = 4 * e + 4 * f * e + 4 * (n + 1) + 4 * 4 * f * n + 2 * 4 * K * n
    bwd_z = 4 * e + (8 * f + 8 * K) * e + 4 * (n + 1) + 3 * 4 * f * n
    return iterations * (fwd + (bwd_c + bwd_z if backward else 0))


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def peak_mb(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def accuracy_lines(dev):
    import _disen_cases as C
    from cogdl_amd.operators.disen import disen_route

    row, col = (t.to(dev) for t in C.graph())
    lines = ["# part 1: disen_route on the GPU against the float64 oracle (tests/_disen_cases.py: %d nodes, %d edges)" % (C.N, row.numel()),
             "# case | tensor | err_new | err_ref | bound = 4 err_ref + 8 eps32 max|oracle| | within"]
    for K, d, tau in C.CASES:
        c, z, G = C.inputs(K, d)
        oracle, ref32 = C.reference(K, d, tau)
        got = C.run(lambda a, b: disen_route(a, b, row, col, K, tau), c, z, G, device=dev)
        for name, (err_new, err_ref, bound) in C.G.errors(got, oracle, ref32).items():
            lines.append("K=%d d=%d tau=%g | %s | %.3e | %.3e | %.3e | %s"
                         % (K, d, tau, name, err_new, err_ref, bound, "yes" if err_new <= bound else "NO"))
    return lines


def reference_layer_class():
    """The reference's DisenGCNLayer and Graph under a plain install(), or (None, None, why)."""
    staged = os.path.join(ROOT, "oracle", "_ref", "pkg")
    ref = staged if os.path.isdir(os.path.join(staged, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "cogdl")):
        return None, None, "reference package not present"
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")  # the reference writes into its own tree when imported
    shutil.copytree(os.path.join(ref, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
    cogdl_amd.install()
    try:
        from cogdl.data import Graph
        from cogdl.layers.disengcn_layer import DisenGCNLayer
    except Exception as e:  # (a dependency of the package that this machine lacks)
        return None, None, "reference package does not import: %s" % e
    return DisenGCNLayer, Graph, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "disengcn_bench.txt"))
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the arxiv-shaped graphs (rehearsals only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("disengcn_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    K, d, iterations = args.K, args.d, args.iterations
    width = K * d
    layer_cls, graph_cls, why = reference_layer_class()
    lines = ["# DisenGCN layer (in %d, K = %d, d = %d, %d iterations, tau 1): neighbor_routing vs the parent route on %s"
             % (IN, K, d, iterations, torch.cuda.get_device_name(0)),
             "# the parent route is the reference package's DisenGCNLayer.forward under a plain install()" if layer_cls is not None
             else "# NO parent route was timed (%s): the fused route alone" % why]
    lines += accuracy_lines(dev)
    lines += ["# part 2: ms per step (device events), median of %d, median [min .. max] over %d alternating rounds; peak MB above "
              "the step's inputs; GB/s = algorithmic bytes of the routing / step time of the fused layer" % (args.repeats, args.rounds),
              "# graph | pass | fused ms | parent ms | parent / fused | fused peak MB | parent peak MB | fused GB/s"]
    graphs = [("Cora-shaped", synth.cora_like(seed=0))]
    for topology in ("uniform", "rmat"):
        g = synth.arxiv_like(seed=0, topology=topology) if args.scale == 1.0 else \
            synth.scaled(max(64, int(169_343 * args.scale)), 13.8, seed=0, topology=topology)
        graphs.append(("arxiv-shaped %s" % topology, g))
    for label, g in graphs:
        n, rowptr, col = g.num_nodes, g.rowptr.to(dev), g.colind.long().to(dev)
        e = col.numel()
        row = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).long())
        gen = torch.Generator().manual_seed(1)
        x = torch.randn(n, IN, generator=gen).to(dev).requires_grad_()
        grad_out = torch.randn(n, width, generator=gen).to(dev)
        weight = (torch.randn(IN, width, generator=gen) * (2.0 / (IN + width)) ** 0.5).to(dev).requires_grad_()
        bias = (torch.randn(width, generator=gen) * 0.1).to(dev).requires_grad_()
        params = [x, weight, bias]
        layer = graph = None
        if layer_cls is not None:
            layer = layer_cls(IN, width, K, iterations, tau=1.0).to(dev)
            layer.weight, layer.bias = torch.nn.Parameter(weight.detach().clone()), torch.nn.Parameter(bias.detach().clone())
            graph = graph_cls(edge_index=torch.stack([row, col]))
            graph.row_indptr  # the graph holds its CSR before the layer runs (the edges are in CSR order already)
            params_ref = [x, layer.weight, layer.bias]

        def fused(backward):
            def run():
                for p in params:
                    p.grad = None
                h = torch.nn.functional.leaky_relu(torch.matmul(x, weight) + bias)
                out = neighbor_routing(h, row, col, K, iterations, 1.0)
                if backward:
                    out.backward(grad_out)
            return run

        def parent(backward):
            def run():
                for p in params_ref:
                    p.grad = None
                out = layer(graph, x)
                if backward:
                    out.backward(grad_out)
            return run

        if layer is not None:  # faster and different is not faster
            fused(True)()
            got = [p.grad.clone() for p in params]
            parent(True)()
            want = [p.grad.clone() for p in params_ref]
            for a, b in zip(got, want):
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max())), float((a - b).abs().max())
        for name, backward in (("forward", False), ("forward + backward", True)):
            ours = fused(backward)
            base = parent(backward) if layer is not None else None
            t_ours, t_base = [], []
            for _ in range(args.rounds):
                t_ours.append(median_ms(ours, args.warmup, args.repeats))
                if base is not None:
                    t_base.append(median_ms(base, args.warmup, args.repeats))
            mo = statistics.median(t_ours)
            rate = "%.0f" % (algorithmic_bytes(n, e, K, d, iterations, backward) / (mo * 1e-3) / 1e9)
            if base is not None:
                mb = statistics.median(t_base)
                theirs = "%.3f [%.3f .. %.3f] | %.2fx" % (mb, min(t_base), max(t_base), mb / mo)
                their_peak = "%.1f" % peak_mb(base)
            else:
                theirs, their_peak = "- | -", "-"
            lines.append("%s (%d nodes, %d edges) | %s | %.3f [%.3f .. %.3f] | %s | %.1f | %s | %s"
                         % (label, n, e, name, mo, min(t_ours), max(t_ours), theirs, peak_mb(ours), their_peak, rate))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
