"""Skip-gram benchmark (cogdl_amd.operators.sgns) on the arxiv-shaped graph: walks from every node (random_walk on the
GPU), then one epoch of skip-gram with negative sampling in the GPU's throughput mode, for both row-update variants and a
sweep of rows_in_flight, against the host twin with the threads of the box on a slice of the same corpus.

Reports tokens/s per epoch, and the share of the float-atomic floor reached: an epoch makes about
tokens * (window + 1) * (negative + 2) row updates of 4 * dim bytes each (mean window span (window + 1) / 2 on both sides;
negative + 1 target rows plus the input row per pair), and the chip adds ~1.3e12 bytes/s by memory-side float atomics.
Timed with device events after one warm-up chunk; the calls are the public ones (table build and flag read-back
included).  Writes a plain-text report to --out.  Needs a GPU.

    python tools/sgns_bench.py --out profiles/sgns_bench.txt
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cogdl_amd import _lib, synth  # noqa: E402
from cogdl_amd.operators import sgns as sgns_mod  # noqa: E402
from cogdl_amd.operators.sgns import skipgram  # noqa: E402
from cogdl_amd.operators.walk import random_walk  # noqa: E402

ATOMIC_BYTES_PER_S = 1.3e12
VARIANTS = ((0, "atomicAdd"), (1, "sc1 stores"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walks-per-node", type=int, default=4, help="the reference's default is 40; tokens/s does not depend on it")
    ap.add_argument("--length", type=int, default=80)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--rows-in-flight", default="2048,8192,32768")
    ap.add_argument("--host-rows", type=int, default=20000, help="rows of the corpus the host twin trains on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sgns_bench needs a GPU"
    dev = torch.device("cuda:0")
    g = synth.arxiv_like(seed=0, topology="uniform")
    n = g.num_nodes
    ip, ix = g.rowptr.long().to(dev), g.colind.long().to(dev)
    start = torch.arange(n, device=dev).repeat(args.walks_per_node)
    walks = random_walk(ip, ix, start, args.length, seed=1)
    tokens = walks.numel()
    updates_per_token = (args.window + 1) * (args.negative + 2)
    floor_tokens = ATOMIC_BYTES_PER_S / (updates_per_token * 4 * args.dim)
    kw = dict(dim=args.dim, window=args.window, negative=args.negative, epochs=1, seed=2)
    lines = ["sgns_bench on %s: %d nodes, %d walks of %d = %d tokens per epoch, dim %d, window %d, negative %d"
             % (torch.cuda.get_device_name(0), n, walks.shape[0], args.length, tokens, args.dim, args.window, args.negative),
             "float-atomic floor: %.3g tokens/s (%d row updates of %d bytes per token at %.2g bytes/s)"
             % (floor_tokens, updates_per_token, 4 * args.dim, ATOMIC_BYTES_PER_S)]
    best = None
    for key, name in VARIANTS:
        _lib.hip().cogdl_hip_set_tuning(17, key)
        for rif in [int(r) for r in args.rows_in_flight.split(",")]:
            sgns_mod.ROWS_IN_FLIGHT = rif
            skipgram(walks[:rif], n, **kw)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            syn0, _ = skipgram(walks, n, **kw)
            t1.record()
            torch.cuda.synchronize()
            rate = tokens / (t0.elapsed_time(t1) * 1e-3)
            assert bool(torch.isfinite(syn0).all())
            lines.append("gpu  %-10s rows_in_flight %6d: %8.1f ms per epoch, %.3e tokens/s, %.1f %% of the atomic floor"
                         % (name, rif, t0.elapsed_time(t1), rate, 100.0 * rate / floor_tokens))
            print(lines[-1], flush=True)
            if best is None or rate > best[0]:
                best = (rate, name, rif)
    _lib.hip().cogdl_hip_set_tuning(17, 0)
    sgns_mod.ROWS_IN_FLIGHT = 0
    host_walks = walks[:args.host_rows].cpu()
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count())
    skipgram(host_walks[:1000], n, workers=threads, **kw)
    t = time.perf_counter()
    skipgram(host_walks, n, workers=threads, **kw)
    host_rate = host_walks.numel() / (time.perf_counter() - t)
    lines.append("host twin, %d threads, %d rows: %.3e tokens/s" % (threads, host_walks.shape[0], host_rate))
    lines.append("best: %s at rows_in_flight %d, %.3e tokens/s = %.1f x the host twin" % (best[1], best[2], best[0], best[0] / host_rate))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
