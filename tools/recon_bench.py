"""Forward + backward of the inner-product decoder loss on one GPU: cogdl_amd.operators.recon.inner_product_bce(route="hip")
against the reference's dense composition, F.binary_cross_entropy(sigmoid(z z^T), adj, reduction="sum") with adj densified
once (cogdl/models/nn/gae.py:76-84), at Cora and PubMed shapes, and the kernels alone at the arxiv shape, where one [N, N]
float32 tensor is 115 GB.  Per shape and route: the median of --repeats whole calls (forward, backward, one synchronisation)
after two warm-up calls, timed with device events, one route after the other; and the peak memory above the inputs (z and the
edges, and for the dense composition its [N, N] adjacency, which is not counted).

    python tools/recon_bench.py [--repeats 7] [--out profiles/recon_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES = (("cora", 2708, 64, 10556, True), ("pubmed", 19717, 64, 88648, True), ("arxiv", 169343, 64, 1166243, False))


def measure(step, repeats):
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base, times = torch.cuda.memory_allocated(), []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        step()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    from cogdl_amd.operators.recon import inner_product_bce

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, lines = "cuda:0", ["inner-product decoder loss, forward + backward, %s, median of %d" % (torch.cuda.get_device_name(0), args.repeats)]
    for name, n, d, e, dense in SHAPES:
        gen = torch.Generator().manual_seed(0)
        z = (torch.randn(n, d, generator=gen) * d ** -0.25).to(dev).requires_grad_()
        src, dst = torch.randint(0, n, (e // 2,), generator=gen), torch.randint(0, n, (e // 2,), generator=gen)
        row, col = torch.cat([src, dst]).to(dev), torch.cat([dst, src]).to(dev)

        def ours():
            z.grad = None
            inner_product_bce(z, row, col, route="hip").backward()

        routes = [("kernels", ours)]
        if dense:
            adj = torch.sparse_coo_tensor(torch.stack([row, col]), torch.ones(row.numel(), device=dev), (n, n)).to_dense().clamp_(max=1)

            def reference():
                z.grad = None
                torch.nn.functional.binary_cross_entropy(torch.sigmoid(torch.mm(z, z.t())), adj, reduction="sum").backward()

            routes.append(("dense composition", reference))
        for label, step in routes:
            ms, mib = measure(step, args.repeats)
            lines.append("%-7s N = %6d d = %3d E = %7d  %-17s %9.3f ms  peak above the inputs %9.1f MiB" % (name, n, d, e, label, ms, mib))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
