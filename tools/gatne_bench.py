"""Measures the GATNE model step on the GPU as install(gatne=True) runs it -- one multiplex_embed call (csrc/multiplex.hip) and one
sampled_scores call -- against the reference's arithmetic written out as the torch composition
(cogdl_amd.operators.multiplex.composition: the [B, T, S, T, U] gather and its diagonal, then NSLoss's gather and bmm).  Writes
profiles/gatne_bench.txt.

    python tools/gatne_bench.py [--out profiles/gatne_bench.txt] [--repeats 20] [--rounds 3] [--skip-forward]

Part 1, accuracy: every case of tests/_multiplex_cases.py on the GPU, err_new and err_ref against the float64 oracle and the bound
4 err_ref + 8 eps32 max|oracle| of the tests.
Part 2, step time and memory: one step (forward + loss + backward, without Adam) at the shapes of the reference's two datasets,
N = 10,166, T = 2 (Amazon) and N = 2,000, T = 5 (YouTube), D = 200, U = 10, A = 20, S = 10, five negatives, at B = 256 and
B = 4096.  Device events around one step; per round `--warmup` steps, then the median of `--repeats`; the two routes alternate
inside a round and the table gives the median round with the range over the rounds.  Peak memory: the peak of torch's allocator
over one step above what is allocated before it.  Before anything is timed the two routes are compared on the same inputs.
Part 3, whole forward: the wall time of cogdl_amd.embedding.gatne for one epoch on a synthetic two-layer network of the Amazon
shape (10,166 nodes, 148,865 edges), and -- where the staged reference package is present -- the reference's own GATNE.forward
against the shim's on a network small enough for the reference to finish in about a minute."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cogdl_amd.operators.kgscore import sampled_scores  # noqa: E402
from cogdl_amd.operators.multiplex import composition, multiplex_embed  # noqa: E402

D, U, A, S, NEG = 200, 10, 20, 10, 5
SHAPES = (("Amazon", 10166, 2), ("YouTube", 2000, 5))
BATCHES = (256, 4096)


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


def ns_loss(scores):
    logsig = torch.nn.functional.logsigmoid
    return -(logsig(scores[:, 0]) + logsig(-scores[:, 1:]).sum(1)).mean()


def fused_step(params, ctx_w, neigh32, x, t, idx):
    embs = multiplex_embed(*params, neigh32, x, t, check=False)
    return ns_loss(sampled_scores(embs, ctx_w, idx, "dot", check=False))


def composed_step(params, ctx_w, neigh, x, t, idx):
    """GATNEModel.forward and NSLoss.forward (gatne.py:221-270) as torch runs them."""
    embs = composition(*params, neigh, x, t)
    return ns_loss(torch.bmm(ctx_w[idx], embs.unsqueeze(2)).squeeze(2))


def accuracy_lines(dev):
    import _multiplex_cases as C

    lines = ["# part 1: multiplex_embed on the GPU against the float64 oracle (tests/_multiplex_cases.py, N = %d)" % C.N,
             "# case | tensor | err_new | err_ref | bound = 4 err_ref + 8 eps32 max|oracle| | within"]
    for name in C.CASES:
        oracle, ref32 = C.reference(name)
        got = C.run(multiplex_embed, name, device=dev)
        for k, (err_new, err_ref, bound) in C.errors(got, oracle, ref32).items():
            lines.append("%s | %s | %.3e | %.3e | %.3e | %s" % (name, k, err_new, err_ref, bound, "yes" if err_new <= bound else "NO"))
    return lines


def step_lines(dev, args):
    lines = ["# part 2: ms per step (forward + loss + backward, no optimizer; device events), median of %d, median [min .. max] over "
             "%d alternating rounds; peak MB above the step's operands" % (args.repeats, args.rounds),
             "# shape | B | fused ms | composition ms | composition / fused | fused peak MB | composition peak MB"]
    for label, n, t_count in SHAPES:
        gen = torch.Generator().manual_seed(1)
        std = D ** -0.5
        params = [torch.rand(n, D, generator=gen) * 2 - 1, torch.rand(n, t_count, U, generator=gen) * 2 - 1,
                  torch.randn(t_count, U, D, generator=gen) * std, torch.randn(t_count, U, A, generator=gen) * std,
                  torch.randn(t_count, A, generator=gen) * std]
        params = [p.to(dev).requires_grad_() for p in params]
        ctx_w = (torch.randn(n, D, generator=gen) * std).to(dev).requires_grad_()
        neigh = torch.randint(0, n, (n, t_count, S), generator=gen).to(dev)
        neigh32 = neigh.to(torch.int32)
        for b in BATCHES:
            x, t = torch.randint(0, n, (b,), generator=gen).to(dev), torch.randint(0, t_count, (b,), generator=gen).to(dev)
            idx = torch.randint(0, n, (b, 1 + NEG), generator=gen).to(dev)

            def step(route, table):
                def run():
                    for p in params + [ctx_w]:
                        p.grad = None
                    route(params, ctx_w, table, x, t, idx).backward()
                return run

            ours, base = step(fused_step, neigh32), step(composed_step, neigh)
            ours()
            got = [p.grad.clone() for p in params + [ctx_w]]
            base()
            want = [p.grad.clone() for p in params + [ctx_w]]
            for g, w in zip(got, want):  # faster and different is not faster
                assert torch.allclose(g, w, rtol=1e-3, atol=1e-4 * float(w.abs().max())), float((g - w).abs().max())
            t_ours, t_base = [], []
            for _ in range(args.rounds):
                t_ours.append(median_ms(ours, args.warmup, args.repeats))
                t_base.append(median_ms(base, args.warmup, args.repeats))
            mo, mb = statistics.median(t_ours), statistics.median(t_base)
            lines.append("%s (N = %d, T = %d) | %d | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.2fx | %.1f | %.1f"
                         % (label, n, t_count, b, mo, min(t_ours), max(t_ours), mb, min(t_base), max(t_base), mb / mo,
                            peak_mb(ours), peak_mb(base)))
            print(lines[-1], flush=True)
    return lines


def random_layers(n, edges_per_layer, layers, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(0, n, (edges_per_layer, 2), generator=gen) for _ in range(layers)]


def reference_forward_seconds(layers, kwargs):
    """The reference's own GATNE.forward on `layers` (from the staged copy of the reference package) and the shim's -> (seconds,
    seconds), or a string saying why it was not measured."""
    import shutil
    import tempfile

    ref = os.path.join(ROOT, "oracle", "_ref", "pkg")
    if not os.path.isdir(os.path.join(ref, "cogdl")):
        return "not measured: the reference package is not staged (oracle/_ref/pkg)"
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")  # (the reference writes into its own tree when imported)
    shutil.copytree(os.path.join(ref, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.path[:0] = [os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
    try:
        import cogdl_amd
        from cogdl_amd import _rebind

        cogdl_amd.install(gatne=True)
        from cogdl.models.emb.gatne import GATNE

        data = {str(k): [tuple(e) for e in layer.tolist()] for k, layer in enumerate(layers)}
        model = GATNE(kwargs["dim"], kwargs["walk_length"], kwargs["walk_num"], 5, 1, kwargs["epochs"], kwargs["batch_size"], U, A, NEG,
                      S, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.forward(data)
        torch.cuda.synchronize()
        shim = time.perf_counter() - t0
        t0 = time.perf_counter()
        _rebind.original(GATNE, "forward")(model, data)
        torch.cuda.synchronize()
        return shim, time.perf_counter() - t0
    except Exception as e:  # (a missing dependency of the reference module: say so, the other parts stand)
        return "not measured: %s: %s" % (type(e).__name__, e)
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


def forward_lines(dev, args):
    from cogdl_amd import embedding

    lines = ["# part 3: wall seconds of the whole forward (walks, vocabulary, pairs, neighbour table, training, final embeddings)"]
    n, per_layer = 10166, 148865 // 2
    layers = random_layers(n, per_layer, 2, seed=3)
    embedding.gatne(random_layers(200, 800, 2, seed=4), epochs=1, seed=0, device=dev)  # (code objects loaded before the clock)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    emb, nodes, losses = embedding.gatne(layers, epochs=1, seed=0, device=dev, return_loss=True)
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    lines.append("embedding.gatne, Amazon-shaped synthetic network (%d nodes, 2 layers of %d random edges), the reference's defaults "
                 "(dim 200, batch 256), 1 epoch | %.1f s | mean loss %.4f | %d nodes embedded"
                 % (n, per_layer, took, losses[0], nodes.numel()))
    print(lines[-1], flush=True)
    small = random_layers(300, 1500, 2, seed=5)
    kwargs = dict(dim=D, walk_length=10, walk_num=2, epochs=1, batch_size=256)
    res = reference_forward_seconds(small, kwargs)
    what = "GATNE.forward, 300 nodes, 2 layers of 1500 random edges, walk_num 2, 1 epoch"
    if isinstance(res, str):
        lines.append("%s | %s" % (what, res))
    else:
        lines.append("%s | shim %.2f s | the reference's own forward %.2f s | reference / shim %.1fx" % (what, res[0], res[1], res[1] / res[0]))
    print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gatne_bench.txt"))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-forward", action="store_true", help="parts 1 and 2 only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gatne_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    lines = ["# GATNE model step (D = %d, U = %d, A = %d, S = %d, %d negatives): multiplex_embed + sampled_scores vs the torch "
             "composition on %s" % (D, U, A, S, NEG, torch.cuda.get_device_name(0)),
             "# the composition is NOT the reference package's module: it is the reference's arithmetic written out in "
             "cogdl_amd/operators/multiplex.py (the [B, T, S, T, U] gather, its diagonal, matmuls, softmax, normalize) and NSLoss's "
             "gather + bmm"]
    lines += accuracy_lines(dev)
    lines += step_lines(dev, args)
    if not args.skip_forward:
        lines += forward_lines(dev, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
