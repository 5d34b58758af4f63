"""Times gen_aggregate (softmax, the aggregation of GENConv) on fp16 / bf16 tensors -- the kernels of csrc/genaggr16.hip, what
the layer reaches under torch AMP -- against (a) the fp32 kernels of csrc/genaggr.hip on the same values and (b) the torch
composition that 16-bit GPU tensors took before the 16-bit kernels existed (operators/genaggr.py: _composition, five [E, F]
tensors and an atomic scatter_add_).  A sibling of tools/genconv_bench.py, whose fp32 numbers keep their meaning.  Writes
profiles/genconv16_bench.txt.

    python tools/genconv16_bench.py [--out profiles/genconv16_bench.txt] [--dtypes fp16,bf16] [--widths 64,128,256]
                                    [--lib another/libcogdl_hip.so]     (time another build of the library: A/B of build flags)

Graphs: the arxiv-shaped graphs of cogdl_amd/synth.py (169,343 nodes, 2.5 M edges; uniform and R-MAT).  Cases: F in 64 / 128 /
256, with and without an edge term (which then wants its gradient, as the layer's edge encoder does), forward and forward +
backward.  A sample is a window of `--calls` back-to-back calls between two device events, divided by their number (one call of
0.2 - 1 ms would be measured with the host's gaps between launches in it; the composition, tens of ms, is one call per window);
per round `--warmup` windows, then the median of `--repeats`; the three routes alternate inside a round and the table gives the
median round with the range over the rounds.  Next to every measured
fp32 / 16-bit ratio stands the ratio of the bytes per edge the two algorithms need, computed from the shapes below: what a
purely bandwidth-bound pair of kernels would show.  Before anything is timed the 16-bit results are compared with the fp32
ones on the same values."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators import genaggr as GA  # noqa: E402

EPS, BETA = 1e-7, 1.0
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def bytes_per_edge(f, size, with_eterm, backward):
    """Forward: colind + the source row [+ the edge-term row].  Backward of the softmax: the destination id + the gradient row
    (element size) + the output and log-sum-exp rows (fp32 either way) [+ the edge id, the edge-term row read and its gradient
    row written].  `size`: bytes per element of x / eterm / grad."""
    fwd = 4 + size * f + (size * f if with_eterm else 0)
    bwd = 4 + size * f + 8 * f + (4 + 2 * size * f if with_eterm else 0)
    return fwd + (bwd if backward else 0)


def median_ms(fn, warmup, repeats, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genconv16_bench.txt"))
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--widths", default="64,128,256")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10, help="kernel calls per timed window")
    ap.add_argument("--lib", default=None, help="path of another build of libcogdl_hip.so")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsals only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("genconv16_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    if args.lib:
        from cogdl_amd import _lib

        _lib.HIP_LIB_PATH = os.path.abspath(args.lib)
    lines = ["# gen_aggregate, softmax, beta = %g: 16-bit kernels vs the fp32 kernels vs the torch composition on 16-bit tensors, %s"
             % (BETA, torch.cuda.get_device_name(0)),
             "# ms per call (device events around %d calls; the composition: 1), median of %d, median [min .. max] over %d alternating "
             "rounds; 'bytes' = fp32 / 16-bit bytes per edge from the shapes (a bandwidth-bound pair would show it), 'measured' = "
             "fp32 ms / 16-bit ms" % (args.calls, args.repeats, args.rounds),
             "# graph | dtype | F | eterm | pass | 16-bit ms | fp32 ms | composition ms | bytes | measured | composition / 16-bit"]
    slower = []
    for topology in ("uniform", "rmat"):
        if args.scale == 1.0:
            g = synth.arxiv_like(seed=0, topology=topology)
        else:
            g = synth.scaled(max(64, int(169_343 * args.scale)), 13.8, seed=0, topology=topology)
        n, rowptr, col = g.num_nodes, g.rowptr.to(dev), g.colind.long().to(dev)
        e = col.numel()
        row = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).long())
        label = "arxiv-shaped %s (%d nodes, %d edges)" % (topology, n, e)
        for f in [int(w) for w in args.widths.split(",")]:
            gen = torch.Generator().manual_seed(f)
            x32 = torch.randn(n, f, generator=gen).to(dev)
            t32 = (torch.randn(e, f, generator=gen) * 0.5).to(dev)
            g32 = torch.randn(n, f, generator=gen).to(dev)
            for name in args.dtypes.split(","):
                dt = DTYPES[name]
                for with_eterm in (False, True):
                    ops = {}
                    for key, d in (("new", dt), ("fp32", torch.float32)):  # the fp32 route runs on the values the 16-bit one holds
                        ops[key] = (x32.to(dt).to(d).requires_grad_(), t32.to(dt).to(d).requires_grad_() if with_eterm else None,
                                    g32.to(dt).to(d))

                    def step(key, backward, fn=GA.gen_aggregate):
                        x, t, go = ops[key]

                        def run():
                            x.grad = None
                            if t is not None:
                                t.grad = None
                            out = fn(x, row, col, t, "softmax", BETA, EPS, num_nodes=n)
                            if backward:
                                out.backward(go)
                            return out
                        return run

                    out16, out32 = step("new", True)(), step("fp32", True)()
                    assert out16.dtype == dt
                    tol = 2.0 ** (-7 if dt == torch.bfloat16 else -10)  # two units roundoff of the 16-bit store
                    for a, b in ((out16.detach(), out32.detach()), (ops["new"][0].grad, ops["fp32"][0].grad)):
                        err, top = float((a.float() - b).abs().max()), float(b.abs().max())  # faster and different is not faster
                        assert err <= tol * top, (name, f, with_eterm, err, top)
                    for pass_name, backward in (("forward", False), ("forward + backward", True)):
                        routes = (step("new", backward), step("fp32", backward), step("new", backward, GA._composition))
                        times = ([], [], [])
                        for _ in range(args.rounds):
                            for ts, fn, calls in zip(times, routes, (args.calls, args.calls, 1)):
                                ts.append(median_ms(fn, args.warmup, args.repeats, calls))
                        m16, m32, mc = (statistics.median(ts) for ts in times)
                        want = bytes_per_edge(f, 4, with_eterm, backward) / bytes_per_edge(f, 2, with_eterm, backward)
                        lines.append("%s | %s | %d | %s | %s | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.2fx | "
                                     "%.2fx | %.2fx" % (label, name, f, "yes" if with_eterm else "no", pass_name, m16, min(times[0]),
                                                        max(times[0]), m32, min(times[1]), max(times[1]), mc, min(times[2]),
                                                        max(times[2]), want, m32 / m16, mc / m16))
                        print(lines[-1], flush=True)
                        if m16 > m32:
                            slower.append(lines[-1])
    lines.append("# rows where the 16-bit kernels are slower than the fp32 kernels: %d" % len(slower))
    lines += ["#   " + s for s in slower]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
