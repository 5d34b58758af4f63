"""LINE benchmark (cogdl_amd.operators.line) on the arxiv-shaped graph: the training kernel's samples/s in the GPU's
throughput mode for orders 1 and 2 over a sweep of samples_in_flight, beside the float-atomic bound; the reference's own
`_train_line` rate; whole embedding.line beside whole embedding.deepwalk on the same graph.

The kernel rate is taken through the library's entry point (cogdl_hip_line_train) on prebuilt tables, in windows of at
least --window seconds between device events after a warm-up call, --repeats times; the median and the spread are reported.
The bound: a sample adds (negative + 2) rows of 4 * dim bytes with float atomics (negative + 1 target rows and the input
row), and the chip adds ~1.3e12 bytes/s that way.  The reference's rate is measured in this process over a few dozen batches
of its unchanged `_train_line` (it does not depend on the graph's size), where the reference package is staged; otherwise it
is reported as unmeasured.  Writes a plain-text report to --out.  Needs a GPU.

    python tools/line_bench.py --out profiles/line_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cogdl_amd import _lib, embedding, synth  # noqa: E402
from cogdl_amd.operators import line as line_mod  # noqa: E402
from cogdl_amd.operators import sgns as sgns_mod  # noqa: E402

ATOMIC_BYTES_PER_S = 1.3e12


def kernel_rate(lib, ops, order, samples, in_flight):
    """One timed call of `samples` samples -> samples/s."""
    eu, ev, ncum, table, emb, ctx, flags, m, n, dim, negative = ops
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    rc = lib.cogdl_hip_line_train(_lib.ptr(eu), _lib.ptr(ev), None, m, n, _lib.ptr(ncum), _lib.ptr(table), dim, negative, order, samples,
                                  0.025, 3, 0, in_flight, _lib.ptr(emb), _lib.ptr(ctx), _lib.ptr(flags), _lib.stream_of(eu))
    t1.record()
    torch.cuda.synchronize()
    assert rc == 0 and int(flags) == 0
    return samples / (t0.elapsed_time(t1) * 1e-3)


def reference_rate(batches):
    """samples/s of the reference's own LINE._train_line over `batches` batches of 1000, or None where it is not staged."""
    from tools import refpkg

    if not refpkg.available():
        return None
    refpkg.setup(install=False)
    if not hasattr(np, "int"):
        np.int = int
    from cogdl.data import Graph
    from cogdl.models.emb.line import LINE

    n = 2048
    gen = torch.Generator().manual_seed(0)
    graph = Graph(edge_index=torch.randint(0, n, (2, 8 * n), generator=gen), num_nodes=n)
    took = []
    inner = LINE._train_line

    def timed(self, order):
        t = time.perf_counter()
        inner(self, order)
        took.append(time.perf_counter() - t)

    LINE._train_line = timed
    try:
        walk_length = (batches * 1000 + n - 1) // n
        model = LINE(64, walk_length, 1, 5, 1000, 0.025, 1)
        model.forward(graph)
    finally:
        LINE._train_line = inner
    return int(walk_length * n / 1000) * 1000 / took[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--samples-in-flight", default="16384,65536,262144,1048576")
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window, at least")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reference-batches", type=int, default=30)
    ap.add_argument("--whole", type=int, default=1, help="0 skips the whole-model comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "line_bench needs a GPU"
    dev = torch.device("cuda:0")
    lib = _lib.hip()
    g = synth.arxiv_like(seed=0, topology="uniform")
    n = g.num_nodes
    ip, ix = g.rowptr.long().to(dev), g.colind.long().to(dev)
    row = torch.repeat_interleave(torch.arange(n, device=dev), ip[1:] - ip[:-1])
    edges, _ = embedding.undirected_edges(row, ix, n)
    m = edges.shape[0]
    eu, ev = edges[:, 0].contiguous(), edges[:, 1].contiguous()
    ncum = sgns_mod._u32(sgns_mod.build_tables(line_mod.weighted_degree(edges, n), 0, 0.75)[1], dev)
    table = sgns_mod.exp_table().to(dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    bound = ATOMIC_BYTES_PER_S / ((args.negative + 2) * 4 * args.dim)
    lines = ["line_bench on %s: %d nodes, %d undirected edges, dim %d, negative %d, throughput mode"
             % (torch.cuda.get_device_name(0), n, m, args.dim, args.negative),
             "float-atomic bound: %.3g samples/s (%d row updates of %d bytes per sample at %.2g bytes/s)"
             % (bound, args.negative + 2, 4 * args.dim, ATOMIC_BYTES_PER_S)]
    best = {}
    for order in (1, 2):
        for in_flight in [int(v) for v in args.samples_in_flight.split(",")]:
            emb, ctx = sgns_mod.init_tables(n, args.dim, 1, dev)
            ops = (eu, ev, ncum, table, emb, ctx, flags, m, n, args.dim, args.negative)
            warm = kernel_rate(lib, ops, order, 1 << 24, in_flight)  # warm-up, and the size of a window
            samples = max(1 << 24, int(warm * args.window * 1.25))
            rates = [kernel_rate(lib, ops, order, samples, in_flight) for _ in range(args.repeats)]
            assert bool(torch.isfinite(emb).all()) and samples / max(rates) >= args.window
            med = statistics.median(rates)
            lines.append("order %d samples_in_flight %8d: %.3e samples/s (median of %d windows of %.2f s; min %.3e, max %.3e), "
                         "%.1f %% of the bound" % (order, in_flight, med, len(rates), samples / med, min(rates), max(rates), 100.0 * med / bound))
            print(lines[-1], flush=True)
            if order not in best or med > best[order][0]:
                best[order] = (med, in_flight)
    for order in (1, 2):
        lines.append("best, order %d: samples_in_flight %d, %.3e samples/s = %.1f %% of the bound"
                     % (order, best[order][1], best[order][0], 100.0 * best[order][0] / bound))
    ref = reference_rate(args.reference_batches)
    if ref is None:
        lines.append("reference _train_line: unmeasured (the reference package is not staged)")
    else:
        lines.append("reference _train_line (interpreted, one CPU thread, %d batches of 1000): %.3e samples/s; the kernel is %.0f x (order 1)"
                     % (args.reference_batches, ref, best[1][0] / ref))
    if args.whole:
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = embedding.line((ip, ix), dim=128, order=3, seed=1)
        torch.cuda.synchronize()
        took = time.perf_counter() - t
        lines.append("whole embedding.line (dim 128, order 3, 80 * 20 samples per node and order = %.3g samples): %.2f s"
                     % (2.0 * 1600 * n, took))
        assert tuple(out.shape) == (n, 128)
        t = time.perf_counter()
        out = embedding.deepwalk((ip, ix), dim=128, walk_length=80, walk_num=40, window=5, epochs=1, seed=1)
        torch.cuda.synchronize()
        took = time.perf_counter() - t
        lines.append("whole embedding.deepwalk (dim 128, walk_length 80, walk_num 40, window 5, ONE epoch of the default 5): %.2f s" % took)
        assert tuple(out.shape) == (n, 128)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
