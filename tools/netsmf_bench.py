"""NetSMF benchmark (cogdl_amd.operators.netsmf) on the arxiv-shaped synthetic graph of cogdl_amd/synth.py (N = 169,343,
about 2.5 M CSR entries, symmetric), window 10:

  (a) the path-sampling kernel alone (cogdl_hip_netsmf_sample through path_pairs, flag read-back included): pairs / s
  (b) path_counts: sampling + canonicalisation (coalesce) + merge, for the largest `passes` whose pairs fit one batch
  (c) sparsifier on that count matrix
  (d) randomized_svd of the sparsifier's matrix, k = 128, n_iter = 5
  (e) the host twin's pairs / s on the threads of the box, for scale

Timed with device events after a warm-up, median of --reps.  Prints a plain-text report and writes it to --out.  Needs a GPU.

    python tools/netsmf_bench.py --out profiles/netsmf_bench.txt
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators import netsmf as ns  # noqa: E402


def time_gpu(fn, reps, warmup=1):
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
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "netsmf_bench.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--dim", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "netsmf_bench needs a GPU"
    dev = torch.device("cuda:0")
    g = synth.arxiv_like(seed=0)
    indptr_h, indices_h = g.rowptr.long(), g.colind.long()
    indptr, indices = indptr_h.to(dev), indices_h.to(dev)
    n, e, window = g.num_nodes, g.nnz, args.window
    passes = max(1, ns.DEFAULT_BATCH // (window * e))  # the largest number of passes whose pairs fit one batch
    samples = passes * e
    lines = []

    def emit(line):  # (printed as it is measured: a slow phase shows in the log)
        lines.append(line)
        print(line, flush=True)

    emit("netsmf_bench on %s: N = %d, E = %d, window %d, passes %d (%d pairs, one batch of at most %d)"
             % (torch.cuda.get_device_name(0), n, e, window, passes, samples * window, ns.DEFAULT_BATCH))

    ms = time_gpu(lambda: ns.path_pairs(indptr, indices, window, 0, samples, seed=1), args.reps)
    emit("path_pairs (kernel + flag read-back)   %9.3f ms   %.3e pairs/s" % (ms, samples * window / (ms * 1e-3)))
    ms = time_gpu(lambda: ns.path_counts(indptr, indices, window, passes, seed=1), args.reps)
    emit("path_counts (sample, coalesce, merge)  %9.3f ms   %.3e pairs/s" % (ms, samples * window / (ms * 1e-3)))
    rowptr, col, count = ns.path_counts(indptr, indices, window, passes, seed=1)
    emit("count matrix: %d cells" % col.numel())
    ms = time_gpu(lambda: ns.sparsifier(indptr, rowptr, col, count, window, passes, 1), args.reps)
    m = ns.sparsifier(indptr, rowptr, col, count, window, passes, 1)
    emit("sparsifier                             %9.3f ms   (%d entries kept)" % (ms, m[1].numel()))
    ms = time_gpu(lambda: ns.randomized_svd(m[0], m[1], m[2], n, args.dim, seed=2), max(1, args.reps // 2))
    emit("randomized_svd k = %d, n_iter = 5      %9.3f ms" % (args.dim, ms))

    host_samples = e  # one pass
    ns.path_pairs(indptr_h, indices_h, window, 0, host_samples, seed=1)
    t = time.perf_counter()
    ns.path_pairs(indptr_h, indices_h, window, 0, host_samples, seed=1)
    sec = time.perf_counter() - t
    emit("host twin, %d threads                  %9.3f ms   %.3e pairs/s"
                 % (torch.get_num_threads(), sec * 1e3, host_samples * window / sec))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
