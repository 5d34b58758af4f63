"""Times one GENConv layer (DeeperGCN: aggr softmax_sg, F = 128, residual, two-layer MLP) on the GPU with its aggregation as
install(genconv=True) binds it -- one gen_aggregate call (cogdl_amd/genconv_compat.py, csrc/genaggr.hip) -- against the same
layer on the parent route: what the reference's GENConv.forward runs under a plain install(), written out here as the calls it
makes (gather x[col] into [E, F], relu + eps, beta *, this library's per-row csr_edge_softmax with H = F, multiply,
scatter_add_ with atomics).  It is not the reference package's layer itself -- the tool needs no copy of the reference -- and the
output file's header says so.  Writes profiles/genconv_bench.txt.

    python tools/genconv_bench.py [--out profiles/genconv_bench.txt] [--repeats 20] [--rounds 3]

Part 1, accuracy: every case of tests/_gen_cases.py on the GPU, err_new and err_ref against the float64 oracle and the bound
4 err_ref + 8 eps32 max|oracle| of the tests.
Part 2, time and memory: the arxiv-shaped graphs of cogdl_amd/synth.py (169,343 nodes, 2.5 M edges after symmetrisation and
self-loops; uniform and R-MAT), forward and forward + backward of the layer, and of the aggregation alone.  Device events
around one step; per round `--warmup` steps, then the median of `--repeats`; the two routes alternate inside a round and the
table gives the median round with the range over the rounds.  Peak memory: the peak of torch's allocator over one step above
what is allocated before it.  For the aggregation alone the table also gives the bytes the algorithm needs (computed from the
shapes, below) over the call time: a call rate, not a kernel's share of peak.  Before anything is timed the two routes are
compared on the same inputs."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators.edge_softmax import csr_edge_softmax  # noqa: E402
from cogdl_amd.operators.genaggr import gen_aggregate  # noqa: E402

F, EPS, BETA = 128, 1e-7, 1.0


def parent_aggregation(x, row, col, rowptr32, beta):
    """deepergcn_layer.py:67-93 for softmax_sg as it runs on a GPU under install(): five [E, F] tensors."""
    edge_msg = torch.relu(x[col]) + EPS
    h = csr_edge_softmax(rowptr32, beta * edge_msg.contiguous())
    h = edge_msg * h
    return torch.zeros_like(x).scatter_add_(0, row.unsqueeze(-1).repeat(1, x.shape[1]), h)


def fused_aggregation(x, row, col, rowptr32, beta):
    return gen_aggregate(x, row, col, None, "softmax", beta, EPS, num_nodes=x.shape[0])


def algorithmic_bytes(n, e, f, backward):
    """Forward: colind + one source row per edge, rowptr, out and lse written.  Backward: dst ids + the gradient, output and
    log-sum-exp rows per edge, rowptr, x read and g_x written."""
    fwd = 4 * e + 4 * f * e + 4 * (n + 1) + 2 * 4 * f * n
    bwd = 4 * e + 3 * 4 * f * e + 4 * (n + 1) + 2 * 4 * f * n
    return fwd + (bwd if backward else 0)


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
    import _gen_cases as C

    row, col = (t.to(dev) for t in C.graph())
    lines = ["# part 1: gen_aggregate on the GPU against the float64 oracle (tests/_gen_cases.py: %d nodes, %d edges)" % (C.N, row.numel()),
             "# case | tensor | err_new | err_ref | bound = 4 err_ref + 8 eps32 max|oracle| | within"]
    cases = [(w, t, a, b, lb, 1.0) for w in C.WIDTHS for t in (False, True)
             for a, b, lb in (("softmax", 0.75, True), ("softmax", 3.0, False), ("sum", None, False), ("mean", None, False))]
    cases += [(w, True, "softmax", 25.0, True, 10.0) for w in (7, 128)]
    for width, with_eterm, aggr, beta, learn, scale in cases:
        x, eterm, G = C.inputs(width, with_eterm, scale)
        oracle, ref32 = C.reference(width, with_eterm, aggr, beta, learn, scale)
        fn = lambda xa, ta, ba: gen_aggregate(xa, row, col, ta, aggr, ba, C.EPS, num_nodes=C.N)  # noqa: E731
        got = C.run(fn, x, eterm, beta, G, learn, device=dev)
        for name, (err_new, err_ref, bound) in C.errors(got, oracle, ref32).items():
            lines.append("F=%d eterm=%d %s beta=%s scale=%g | %s | %.3e | %.3e | %.3e | %s"
                         % (width, with_eterm, aggr, beta, scale, name, err_new, err_ref, bound, "yes" if err_new <= bound else "NO"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genconv_bench.txt"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsals only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("genconv_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    lines = ["# GENConv layer (softmax_sg, F = %d): gen_aggregate vs the parent route on %s" % (F, torch.cuda.get_device_name(0)),
             "# the parent route is NOT the reference layer run under install(): it is written out in this tool as the calls that layer "
             "makes on a GPU (gather, relu + eps, beta *, cogdl_amd's csr_edge_softmax at H = F, multiply, scatter_add_), around the "
             "same residual and MLP"]
    lines += accuracy_lines(dev)
    lines += ["# part 2: ms per step (device events), median of %d, median [min .. max] over %d alternating rounds; peak MB above "
              "the step's inputs; GB/s = algorithmic bytes / call time (aggregation alone)" % (args.repeats, args.rounds),
              "# graph | what | pass | fused ms | parent ms | parent / fused | fused peak MB | parent peak MB | fused GB/s"]
    for topology in ("uniform", "rmat"):
        if args.scale == 1.0:
            g = synth.arxiv_like(seed=0, topology=topology)
        else:
            g = synth.scaled(max(64, int(169_343 * args.scale)), 13.8, seed=0, topology=topology)
        n, rowptr32, col = g.num_nodes, g.rowptr.to(dev), g.colind.long().to(dev)
        e = col.numel()
        row = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr32[1:] - rowptr32[:-1]).long())
        gen = torch.Generator().manual_seed(1)
        x = torch.randn(n, F, generator=gen).to(dev).requires_grad_()
        grad_out = torch.randn(n, F, generator=gen).to(dev)
        beta = torch.nn.Parameter(torch.tensor([BETA], device=dev), requires_grad=False)  # (the reference's default: learn_beta False)
        torch.manual_seed(2)
        mlp = torch.nn.Sequential(torch.nn.Linear(F, 2 * F), torch.nn.ReLU(), torch.nn.Linear(2 * F, F)).to(dev)
        params = [x] + list(mlp.parameters())

        def step(aggregation, layer, backward):
            def run():
                for p in params:
                    p.grad = None
                h = aggregation(x, row, col, rowptr32, beta)
                if layer:
                    h = mlp(h + x)
                if backward:
                    h.backward(grad_out)
            return run

        step(fused_aggregation, True, True)()
        got = [p.grad.clone() for p in params]
        step(parent_aggregation, True, True)()
        want = [p.grad.clone() for p in params]
        for a, b in zip(got, want):  # faster and different is not faster
            assert torch.allclose(a, b, rtol=1e-3, atol=1e-4 * float(b.abs().max())), float((a - b).abs().max())
        label = "arxiv-shaped %s (%d nodes, %d edges)" % (topology, n, e)
        for what, layer in (("layer", True), ("aggregation", False)):
            for name, backward in (("forward", False), ("forward + backward", True)):
                ours, base = step(fused_aggregation, layer, backward), step(parent_aggregation, layer, backward)
                t_ours, t_base = [], []
                for _ in range(args.rounds):
                    t_ours.append(median_ms(ours, args.warmup, args.repeats))
                    t_base.append(median_ms(base, args.warmup, args.repeats))
                mo, mb = statistics.median(t_ours), statistics.median(t_base)
                rate = "%.0f" % (algorithmic_bytes(n, e, F, backward) / (mo * 1e-3) / 1e9) if not layer else "-"
                lines.append("%s | %s | %s | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.2fx | %.1f | %.1f | %s"
                             % (label, what, name, mo, min(t_ours), max(t_ours), mb, min(t_base), max(t_base), mb / mo,
                                peak_mb(ours), peak_mb(base), rate))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
