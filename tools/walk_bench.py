"""Random-walk benchmark (cogdl_amd.operators.walk) on the arxiv-shaped uniform graph and the arxiv-sized R-MAT graph:

  (a) random_walk, every node a start, L = 80, restart_p 0 and 0.5   vs a plain torch composition of the same walk
                                                                       and vs the host twin (OpenMP, the threads of the box)
  (b) node2vec_walk, same starts, (p, q) = (0.25, 4) and (1, 1), with the fraction of steps decided by the exact fallback
      (--trials sweeps the cap on rejection trials)
  (c) the 2-step walk of 1024 starts that the unsupervised GraphSAGE sampler makes per batch (cogdl/data/sampler.py:162-165)

Timed with device events after warm-up; the calls are the public ones (flag read-back included).  Prints one JSON document
and writes it to --out.  Needs a GPU.

    python tools/walk_bench.py --out profiles/walk_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators import walk as walk_mod  # noqa: E402
from cogdl_amd.operators.walk import node2vec_walk, random_walk  # noqa: E402


def torch_walk(indptr, indices, start, length, restart_p):
    """What a user writes without the kernel: per step gather the row pointers, torch.rand, multiply, floor, gather."""
    w = start.numel()
    out = torch.empty(w, length, dtype=torch.long, device=start.device)
    out[:, 0] = start
    cur = start
    last = indices.numel() - 1
    for i in range(1, length):
        src = cur if restart_p == 0 else torch.where(torch.rand(w, device=start.device) < restart_p, start, cur)
        beg = indptr[src]
        deg = indptr[src + 1] - beg
        off = (torch.rand(w, device=start.device) * deg).long()
        nxt = indices[(beg + torch.minimum(off, deg - 1)).clamp(0, last)]
        cur = torch.where(deg > 0, nxt, cur)
        out[:, i] = cur
    return out


def time_gpu(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def time_host(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def entry(ms, steps):
    med, lo, hi = ms
    return {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "steps_per_s": round(steps / (med * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="abc", help="which parts to run (letters of a, b, c)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--length", type=int, default=80)
    ap.add_argument("--trials", default="0", help="comma-separated caps on node2vec rejection trials (0 = library default)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "walk_bench needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "length": args.length, "reps": args.reps,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(), "graphs": {}}
    for topo in ("uniform", "rmat"):
        g = synth.arxiv_like(seed=0, topology=topo)
        n = g.num_nodes
        ip_h, ix_h = g.rowptr.long(), g.colind.long()
        ip, ix = ip_h.to(dev), ix_h.to(dev)
        start = torch.arange(n, device=dev)
        steps = n * (args.length - 1)
        out = {"num_nodes": n, "num_edges": int(ix.numel()), "max_degree": int(g.degrees().max())}
        if "a" in args.only:
            for rp in (0.0, 0.5):
                row = {"kernel": entry(time_gpu(lambda: random_walk(ip, ix, start, args.length, restart_p=rp, seed=1), args.reps), steps)}
                if not args.no_torch:
                    row["torch"] = entry(time_gpu(lambda: torch_walk(ip, ix, start, args.length, rp), max(3, args.reps // 2), 1), steps)
                    row["torch_over_kernel"] = round(row["torch"]["ms"] / row["kernel"]["ms"], 2)
                if not args.no_host:
                    st_h = start.cpu()
                    row["host"] = entry(time_host(lambda: random_walk(ip_h, ix_h, st_h, args.length, restart_p=rp, seed=1), 3), steps)
                    row["host_over_kernel"] = round(row["host"]["ms"] / row["kernel"]["ms"], 2)
                out["random_walk_restart_%g" % rp] = row
        if "b" in args.only:
            for p, q in ((0.25, 4.0), (1.0, 1.0)):
                for cap in [int(c) for c in args.trials.split(",")]:
                    walk_mod.NODE2VEC_TRIALS = cap
                    _, fb = node2vec_walk(ip, ix, start, args.length, p=p, q=q, seed=1, return_fallback=True)
                    row = entry(time_gpu(lambda: node2vec_walk(ip, ix, start, args.length, p=p, q=q, seed=1), args.reps), steps)
                    row["fallback_fraction"] = round(float(fb.double().sum()) / steps, 6)
                    out["node2vec_p%g_q%g_trials%d" % (p, q, cap)] = row
                walk_mod.NODE2VEC_TRIALS = 0
        if "c" in args.only:
            batch = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:1024].to(dev)
            row = {"kernel": entry(time_gpu(lambda: random_walk(ip, ix, batch, 2, seed=1), 50, 5), 1024)}
            if not args.no_torch:
                row["torch"] = entry(time_gpu(lambda: torch_walk(ip, ix, batch, 2, 0.0), 50, 5), 1024)
                row["torch_over_kernel"] = round(row["torch"]["ms"] / row["kernel"]["ms"], 2)
            out["sampler_2step_1024"] = row
        res["graphs"][topo] = out
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
