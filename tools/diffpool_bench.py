"""Forward + backward time and peak memory of the reference's BatchedDiffPoolLayer, served by install(diffpool=True) against
the reference's own forward on the same GPU, at three synthetic batch shapes.  Writes profiles/diffpool_bench.txt.

    python tools/diffpool_bench.py [--ref oracle/_ref/pkg] [--iters 20] [--out profiles/diffpool_bench.txt]

Times are device-event times around `iters` steps after 3 warm-up steps, the two forwards alternating per shape in rounds;
memory is torch.cuda.max_memory_allocated over the timed steps.  A GPU is required: there is no CPU figure to report."""
import argparse
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("PROTEINS-like", 20, 39, 93, 64), ("COLLAB-like", 20, 75, 73, 64), ("REDDIT-BINARY-like", 20, 430, 567, 64))
F_IN, DEGREE = 64, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.path.join(ROOT, "oracle", "_ref", "pkg"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffpool_bench.txt"))
    args = ap.parse_args()
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")  # the reference writes into its own tree when imported
    shutil.copytree(os.path.join(args.ref, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("diffpool_bench: no GPU")
    import cogdl_amd
    from cogdl_amd import diffpool_compat

    cogdl_amd.install()
    from cogdl.data import Graph
    from cogdl.models.nn.diffpool import BatchedDiffPoolLayer

    original = BatchedDiffPoolLayer.__dict__["forward"]
    dev = "cuda:0"

    def steps(layer, graph, x, batch, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            layer.zero_grad(set_to_none=True)
            adj_new, h = layer(graph, x, batch)
            (adj_new.sum() + h.sum() + layer.get_loss()).backward()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / n

    lines = ["# tools/diffpool_bench.py on %s, torch %s; forward + backward of one BatchedDiffPoolLayer, link loss on, %d steps"
             % (torch.cuda.get_device_name(0), torch.__version__, args.iters),
             "# shape: B graphs x about n_g nodes, K clusters per graph, F features; ms per step (the better of 3 rounds), peak MiB"]
    for name, b, n_g, k, f in SHAPES:
        gen = torch.Generator().manual_seed(b * n_g + k)
        sizes = torch.randint(max(1, n_g * 3 // 4), n_g * 5 // 4 + 1, (b,), generator=gen)
        n = int(sizes.sum())
        base = torch.repeat_interleave(torch.cumsum(sizes, 0) - sizes, sizes * DEGREE)
        span = torch.repeat_interleave(sizes, sizes * DEGREE)
        row = base + (torch.rand(base.numel(), generator=gen) * span).long()
        col = base + (torch.rand(base.numel(), generator=gen) * span).long()
        row, col = torch.cat([row, torch.tensor([n - 1])]), torch.cat([col, torch.tensor([n - 1])])
        batch = torch.repeat_interleave(torch.arange(b), sizes).to(dev)
        x = torch.randn(n, F_IN, generator=gen).to(dev).requires_grad_()
        torch.manual_seed(0)
        layer = BatchedDiffPoolLayer(F_IN, f, b * k, b, link_pred_loss=True).to(dev)
        graph = Graph(x=x.detach(), edge_index=torch.stack([row, col])).to(dev)
        best, peak, outs = {}, {}, {}
        for rnd in range(3):
            for tag, fwd in (("served", diffpool_compat.forward), ("reference", original)):
                BatchedDiffPoolLayer.forward = fwd
                steps(layer, graph, x, batch, 3)
                torch.cuda.reset_peak_memory_stats()
                ms = steps(layer, graph, x, batch, args.iters)
                best[tag] = min(ms, best.get(tag, ms))
                peak[tag] = torch.cuda.max_memory_allocated() / 2 ** 20
                outs[tag] = layer(graph, x, batch)[1].detach()
        diff = float((outs["served"] - outs["reference"]).abs().max() / outs["reference"].abs().max())
        lines.append("%-19s B=%d N=%d E=%d K=%d F=%d   served %8.3f ms %8.1f MiB   reference %8.3f ms %8.1f MiB   x%.2f time, "
                     "x%.2f memory   max|h - h_ref| / max|h_ref| = %.1e"
                     % (name, b, n, row.numel(), k, f, best["served"], peak["served"], best["reference"], peak["reference"],
                        best["reference"] / best["served"], peak["reference"] / peak["served"], diff))
        print(lines[-1], flush=True)
    BatchedDiffPoolLayer.forward = original
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
