"""Times one RGCN layer's message passing on the GPU, forward + backward -- the bodies install(rgcn=True) binds
(cogdl_amd/rgcn_compat.py: rgcn_basis_aggregate + one matmul; rgcn_bdd_aggregate) -- against the correct torch composition of
the same law written out here, and writes profiles/rgcn_bench.txt.

    python tools/rgcn_bench.py [--out profiles/rgcn_bench.txt] [--repeats 30] [--rounds 3]

Shape: an FB15k-237-sized synthetic typed graph -- 14,541 entities, 474 types (237 relations and their inverses), 2 x 310,000
edges, hidden 200, row-normalised edge weights; `basis` with B = 5 (the reference's default), `bdd` with 40 blocks of 5 x 5.
The composition: basis forms x @ W[t] for every type ([R, N, out]), gathers one row per edge, scales and index_add_s it; bdd
gathers W[etype] ([E, B, bi, bo]), multiplies per edge (a broadcast product and a sum: as an einsum it is a batched matmul of
E * B batches, which this shape does not survive) and index_add_s.  Timed: device events around one forward + backward (gradients
of x and of every weight); per round `--warmup` steps, then the median of `--repeats`; the two bodies alternate
inside a round and the table gives the median round with the range over the rounds.  Peak memory: the peak of torch's
allocator over one step above what is allocated before it.  Before anything is timed the two bodies are compared on the same
inputs.  The baseline is the composition, not this library."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cogdl_amd.operators import rgcn_basis_aggregate, rgcn_bdd_aggregate  # noqa: E402

N, TYPES, EDGES, HIDDEN, BASES, BLOCKS = 14541, 474, 310000, 200, 5, 40


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgcn_bench.txt"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsals only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgcn_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    n, e = max(8, int(N * args.scale)), max(8, int(EDGES * args.scale))
    gen = torch.Generator().manual_seed(0)
    src, dst = torch.randint(0, n, (e,), generator=gen), torch.randint(0, n, (e,), generator=gen)
    typ = torch.randint(0, TYPES // 2, (e,), generator=gen)
    row, col, etype = (torch.cat([dst, src]).to(dev), torch.cat([src, dst]).to(dev), torch.cat([typ, typ + TYPES // 2]).to(dev))
    norm = torch.bincount(row, minlength=n).float().reciprocal()[row]
    x = torch.randn(n, HIDDEN, generator=gen).to(dev).requires_grad_()
    grad_out = torch.randn(n, HIDDEN, generator=gen).to(dev)
    bi = HIDDEN // BLOCKS
    alpha = torch.randn(TYPES, BASES, generator=gen).to(dev).requires_grad_()
    V = (torch.randn(BASES, HIDDEN, HIDDEN, generator=gen) * 0.1).to(dev).requires_grad_()
    W = (torch.randn(TYPES, BLOCKS, bi, bi, generator=gen) * 0.1).to(dev).requires_grad_()

    def basis_ours():
        return rgcn_basis_aggregate(x, alpha, row, col, etype, norm).view(n, -1) @ V.view(-1, HIDDEN)

    def basis_torch():
        h = torch.matmul(x, (alpha @ V.view(BASES, -1)).view(TYPES, HIDDEN, HIDDEN))  # [R, N, out]
        return torch.zeros(n, HIDDEN, device=dev).index_add_(0, row, h[etype, col] * norm.unsqueeze(-1))

    def bdd_ours():
        return rgcn_bdd_aggregate(x, W, row, col, etype, norm)

    def bdd_torch():
        msg = (x[col].view(-1, BLOCKS, bi, 1) * W[etype]).sum(2).reshape(-1, HIDDEN)  # (no E * B-batch matmul)
        return torch.zeros(n, HIDDEN, device=dev).index_add_(0, row, msg * norm.unsqueeze(-1))

    lines = ["# RGCN message passing, forward + backward: cogdl_amd.operators.rgcn vs the torch composition of the same law on %s"
             % torch.cuda.get_device_name(0),
             "# %d entities, %d types, %d edges, hidden %d; ms per step (device events), median of %d, median [min .. max] over %d "
             "alternating rounds; peak MB above the step's inputs" % (n, TYPES, 2 * e, HIDDEN, args.repeats, args.rounds),
             "# regulariser | ours ms | composition ms | speedup | ours peak MB | composition peak MB"]
    for label, ours_body, base_body, params in (("basis B=%d" % BASES, basis_ours, basis_torch, (x, alpha, V)),
                                                ("bdd %dx%dx%d" % (BLOCKS, bi, bi), bdd_ours, bdd_torch, (x, W))):
        def step(body):
            def run():
                for p in params:
                    p.grad = None
                body().backward(grad_out)
            return run

        ours, base = step(ours_body), step(base_body)
        ours()
        got = [p.grad.clone() for p in params]
        base()
        want = [p.grad.clone() for p in params]
        for a, b in zip(got, want):  # faster and different is not faster
            assert torch.allclose(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max())), float((a - b).abs().max())
        t_ours, t_base = [], []
        for _ in range(args.rounds):
            t_ours.append(median_ms(ours, args.warmup, args.repeats))
            t_base.append(median_ms(base, args.warmup, args.repeats))
        mo, mb = statistics.median(t_ours), statistics.median(t_base)
        lines.append("%s | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.2fx | %.1f | %.1f"
                     % (label, mo, min(t_ours), max(t_ours), mb, min(t_base), max(t_base), mb / mo, peak_mb(ours), peak_mb(base)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
