"""Times CompGCN's typed message passing on the GPU -- the body install(relational=True) binds
(cogdl_amd/relational_compat.py: one rel_gspmm aggregation to [N, in], then one [N, in] x [in, out] matmul) -- against the
body of the reference's CompGCNLayer.message_passing, written out here as the torch calls it makes (gather x[col], gather
rel_embed[edge_types], combine, matmul to [E, out], scale per edge, scatter_add_), and writes profiles/relational_bench.txt.

    python tools/relational_bench.py [--out profiles/relational_bench.txt] [--repeats 30] [--rounds 3]

Shape: an FB15k-237-sized synthetic typed graph -- 14,541 entities, 237 relations plus their reverses (and the self-loop
relation: a table of 475 rows), 272,115 edges per direction, 100 -> 200, `opn` sub and mult.  Timed: forward + backward
(gradients of x, the relation table and the weight) of one direction ("in", row-normalised edge weights), and of the three
calls a layer makes (in, out, loop).  Device events around one step; per round `--warmup` steps, then the median of
`--repeats`; the two bodies alternate inside a round and the table gives the median round with the range over the rounds.
Peak memory: the peak of torch's allocator over one step above what is allocated before it.  Before anything is timed the
two bodies are compared on the same inputs (same numbers up to float32 re-association).  The baseline is the composition,
not this library."""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cogdl_amd import relational_compat  # noqa: E402

N, RELS, EDGES, IN, OUT = 14541, 237, 272115, 100, 200


def composition_body(layer, x, rel_embed, edge_index, edge_types, mode, edge_weight=None):
    """What the reference's method does, call for call (dropout 0 here)."""
    tail = x[edge_index[1]]
    rel = rel_embed[edge_types]
    trans = tail - rel if layer.opn == "sub" else tail * rel
    trans = torch.matmul(trans, getattr(layer, "weight_%s" % mode))
    if edge_weight is not None:
        trans = trans * edge_weight.unsqueeze(-1)
    dim = trans.shape[1]
    return torch.zeros(x.shape[0], dim, device=x.device).scatter_add_(0, edge_index[0].unsqueeze(-1).repeat(1, dim), trans)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relational_bench.txt"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graph (rehearsals only)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("relational_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    n, e = max(8, int(N * args.scale)), max(8, int(EDGES * args.scale))
    gen = torch.Generator().manual_seed(0)
    src, dst = torch.randint(0, n, (e,), generator=gen), torch.randint(0, n, (e,), generator=gen)
    typ = torch.randint(0, RELS, (e,), generator=gen)
    row, col, etype = (torch.cat([dst, src]).to(dev), torch.cat([src, dst]).to(dev), torch.cat([typ, typ + RELS]).to(dev))
    loop = torch.arange(n, device=dev)
    loop_types = torch.full((n,), 2 * RELS, dtype=torch.long, device=dev)
    deg_in = torch.bincount(row[:e], minlength=n).float()
    deg_out = torch.bincount(row[e:], minlength=n).float()
    calls = {"in": ((row[:e], col[:e]), etype[:e], (1 / deg_in.clamp(min=1))[row[:e]]),
             "out": ((row[e:], col[e:]), etype[e:], (1 / deg_out.clamp(min=1))[row[e:]]),
             "loop": ((loop, loop), loop_types, None)}
    x = torch.randn(n, IN, generator=gen).to(dev).requires_grad_()
    rel = torch.randn(2 * RELS + 1, IN, generator=gen).to(dev).requires_grad_()
    grad_out = torch.randn(n, OUT, generator=gen).to(dev)
    lines = ["# CompGCN message passing, forward + backward: rel_gspmm + one matmul vs the reference's torch composition on %s"
             % torch.cuda.get_device_name(0),
             "# %d entities, %d relations + reverses, %d edges per direction, %d -> %d; ms per step (device events), median of %d, "
             "median [min .. max] over %d alternating rounds; peak MB above the step's inputs"
             % (n, RELS, e, IN, OUT, args.repeats, args.rounds),
             "# opn | calls | ours ms | composition ms | speedup | ours peak MB | composition peak MB"]
    for opn in ("sub", "mult"):
        layer = types.SimpleNamespace(opn=opn, dropout=0.0, training=True)
        for mode in calls:
            w = torch.randn(IN, OUT, generator=gen).to(dev) * 0.1
            setattr(layer, "weight_%s" % mode, w.requires_grad_())
        params = [x, rel] + [getattr(layer, "weight_%s" % m) for m in calls]

        def step(body, modes):
            def run():
                for p in params:
                    p.grad = None
                total = None
                for m in modes:
                    idx, types_, weight = calls[m]
                    y = body(layer, x, rel, idx, types_, m, weight)
                    total = y if total is None else total + y
                total.backward(grad_out)
            return run

        for label, modes in (("in", ("in",)), ("in + out + loop", ("in", "out", "loop"))):
            ours, base = step(relational_compat.message_passing, modes), step(composition_body, modes)
            ours()
            got = [p.grad.clone() for p in params if p.grad is not None]
            base()
            want = [p.grad.clone() for p in params if p.grad is not None]
            for a, b in zip(got, want):  # faster and different is not faster
                assert torch.allclose(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max())), float((a - b).abs().max())
            t_ours, t_base = [], []
            for _ in range(args.rounds):
                t_ours.append(median_ms(ours, args.warmup, args.repeats))
                t_base.append(median_ms(base, args.warmup, args.repeats))
            mo, mb = statistics.median(t_ours), statistics.median(t_base)
            lines.append("%s | %s | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.2fx | %.1f | %.1f"
                         % (opn, label, mo, min(t_ours), max(t_ours), mb, min(t_base), max(t_base), mb / mo, peak_mb(ours),
                            peak_mb(base)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
