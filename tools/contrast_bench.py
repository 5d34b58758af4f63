"""Times GRACE's contrastive loss, grace_loss, on the kernels of csrc/contrast.hip (route="hip") against the blocked composition
on torch's kernels (route="torch", what the operator ran on GPU tensors before the kernels existed), same process, same GPU.
Needs a GPU.  Writes profiles/contrast_bench.txt.

    python tools/contrast_bench.py [--out profiles/contrast_bench.txt] [--repeats 7] [--only NAME] [--dtype float32,float16,bfloat16]

--dtype: one section per operand dtype.  For float16 / bfloat16 route="hip" is csrc/contrast16.hip and route="torch" is what such
inputs ran before those kernels existed: the blocked composition in their own dtype.  Their share of peak is taken against the
dense 16-bit matrix peak of 2516.6 TFLOP/s.

Shapes: Cora-like M = 2708 at d = 128 and 256, PubMed-like M = 19717 at d = 256 (keys: both views, N' = 2 M), and the reference's
batched form, B = 1024 queries against arxiv's 169343 + B keys at d = 256.  tau = 0.5, rows N(0, 1) (grace_loss normalises them).
Per shape and route: forward + backward (loss, gradients of both inputs) and forward alone (no_grad).  The two routes alternate,
each call between device synchronisations on the host clock; two warm-up rounds, then `--repeats` rounds: the median, and the
spread as (max - min) / median of the repeats.  Peak: torch.cuda.max_memory_allocated over one forward + backward above what was
allocated before it (inputs excluded).  Share of peak: the products the algorithm needs -- 2 M N' d FLOP per product, one for the
forward, three more for the backward (scores again, grad_q, grad_k) -- over the median time of the WHOLE call (normalisation,
concatenation and the mean included) against the fp32 matrix peak of 157.3 TFLOP/s: a whole-call rate.  (The kernels recompute
the scores once per gradient, five products in all; the rate counts four.)"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from cogdl_amd.operators.contrast import grace_loss  # noqa: E402

PEAK = {"float32": 157.3e12, "float16": 2516.6e12, "bfloat16": 2516.6e12}
TAU = 0.5
# name, rows of z1, rows of z2, d
SHAPES = (("tiny-24", 70, 70, 24), ("small-64", 256, 256, 64), ("1024-128", 1024, 1024, 128), ("1024-256", 1024, 1024, 256), ("cora-128", 2708, 2708, 128), ("cora-256", 2708, 2708, 256), ("8192-128", 8192, 8192, 128), ("8192-256", 8192, 8192, 256), ("pubmed-256", 19717, 19717, 256),
          ("arxiv-batched-256", 1024, 169343, 256))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast_bench.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", default=None)
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("contrast_bench: needs a GPU")
    dev = torch.device("cuda:0")
    import warnings

    from cogdl_amd.operators.ops import TorchRouteWarning

    warnings.simplefilter("ignore", TorchRouteWarning)
    lines = []
    for dtype_name in args.dtype.split(","):
        dtype = getattr(torch, dtype_name)
        lines += ["grace_loss, tau %.1f, %s, %s; median of %d alternated repeats, spread = (max - min) / median"
                 % (TAU, dtype_name, torch.cuda.get_device_name(0), args.repeats),
                 "%-18s %-6s %-8s %10s %8s %10s %8s %9s %9s" % ("shape", "route", "pass", "ms", "spread", "TFLOP/s", "of peak", "peak MiB",
                                                              "hip/torch")]
        for name, m, n, d in SHAPES:
            if args.only and args.only != name:
                continue
            gen = torch.Generator().manual_seed(1)
            z1 = torch.randn(m, d, generator=gen).to(dev, dtype).requires_grad_()
            z2 = torch.randn(n, d, generator=gen).to(dev, dtype).requires_grad_()

            def fwd_bwd(route):
                z1.grad = z2.grad = None
                grace_loss(z1, z2, TAU, route=route).backward()

            def fwd(route):
                with torch.no_grad():
                    grace_loss(z1, z2, TAU, route=route)

            flops = 2.0 * m * (m + n) * d
            for label, fn, products in (("fwd+bwd", fwd_bwd, 4), ("fwd", fwd, 1)):
                times = {"hip": [], "torch": []}
                for rnd in range(2 + args.repeats):
                    for route in ("hip", "torch"):
                        t = timed(lambda: fn(route))
                        if rnd >= 2:
                            times[route].append(t)
                peak = {}
                for route in ("hip", "torch"):
                    z1.grad = z2.grad = None
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    fn(route)
                    torch.cuda.synchronize()
                    peak[route] = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
                med = {r: statistics.median(times[r]) for r in times}
                for route in ("hip", "torch"):
                    spread = (max(times[route]) - min(times[route])) / med[route]
                    rate = products * flops / med[route]
                    lines.append("%-18s %-6s %-8s %10.3f %7.1f%% %10.2f %7.1f%% %9.1f %9s"
                                 % (name, route, label, med[route] * 1e3, spread * 100, rate / 1e12, rate / PEAK[dtype_name] * 100, peak[route],
                                    "%.2fx" % (med["hip"] / med["torch"]) if route == "hip" else ""))
                print("\n".join(lines[-2:]), flush=True)
            del z1, z2
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
