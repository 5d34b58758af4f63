"""Times the top-k PPR operator: GPU kernel against the host twin of the same commit, on the arxiv-shaped and the
products-shaped synthetic graph, with PPRGo's (alpha 0.5, eps 1e-4, topk 32) and MVGRL's (0.4, 1e-4, 8) parameters, for
1 k / 16 k / "all train nodes" (a tenth of the graph) sources.  Writes profiles/ppr_bench.txt.

GPU: event-timed, median of --reps runs after one warm-up.  Host: wall clock of one call at the OpenMP thread count of the
process.  Also recorded: rounds and touched nodes per source, and which table placement (LDS / workspace) served the case.

    python tools/ppr_bench.py [--graphs arxiv,products] [--reps 5] [--out profiles/ppr_bench.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators import ppr as ppr_mod  # noqa: E402
from cogdl_amd.operators import topk_ppr  # noqa: E402

PARAMS = (("pprgo", 0.5, 1e-4, 32), ("mvgrl", 0.4, 1e-4, 8))


def graph(name):
    if name == "arxiv":
        g = synth.arxiv_like(seed=0)
    else:  # products-shaped: 2.4 M nodes, average degree 50, R-MAT
        g = synth.scaled(2_449_029, 50, seed=0, topology="rmat", self_loops=False)
    return g.rowptr.long(), g.colind.long(), g.num_nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="arxiv,products")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max-sources", type=int, default=16384, help="the host twin is timed up to this many sources")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppr_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# tools/ppr_bench.py on %s, %d host threads, median of %d" % (torch.cuda.get_device_name(0), torch.get_num_threads(), args.reps),
             "# graph params sources | gpu_ms sources/s | host_ms | rounds mean/max | touched mean/max | table"]
    for gname in args.graphs.split(","):
        indptr, indices, n = graph(gname)
        ip, ix = indptr.to(dev), indices.to(dev)
        deg = indptr[1:] - indptr[:-1]
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
        for pname, alpha, eps, topk in PARAMS:
            for s in (1024, 16384, n // 10):
                src = perm[:s].contiguous()
                maxdeg = int(deg[src].max())
                plan = ppr_mod.plan(n, indices.numel(), maxdeg, alpha, eps)
                src_d = src.to(dev)
                *_, stats = topk_ppr(ip, ix, src_d, alpha, eps, topk, max_source_degree=maxdeg, return_stats=True)  # warm-up
                times = []
                for _ in range(args.reps):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    topk_ppr(ip, ix, src_d, alpha, eps, topk, check=False, max_source_degree=maxdeg)
                    t1.record()
                    t1.synchronize()
                    times.append(t0.elapsed_time(t1))
                gpu_ms = sorted(times)[len(times) // 2]
                host_ms = float("nan")
                if s <= args.host_max_sources:
                    t = time.perf_counter()
                    topk_ppr(indptr, indices, src, alpha, eps, topk, max_source_degree=maxdeg)
                    host_ms = (time.perf_counter() - t) * 1e3
                st = stats.float().cpu()
                line = ("%-8s %-5s %7d | %9.3f %11.0f | %9.1f | %5.1f %4d | %7.0f %6d | %s (%d slots)"
                        % (gname, pname, s, gpu_ms, s / gpu_ms * 1e3, host_ms, st[:, 0].mean(), int(st[:, 0].max()),
                           st[:, 1].mean(), int(st[:, 1].max()), "LDS" if plan["lds"] else "workspace", plan["table_slots"]))
                print(line, flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
