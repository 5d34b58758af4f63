"""Times the fused polynomial filter step (cogdl_hip_csr_filter_step, csrc/polyfilter.hip) against the same arithmetic as
csrspmm plus torch's elementwise kernels, both at this commit, and the whole cogdl_amd.embedding.prone against the reference
package's ProNE.forward on the host.  Needs a GPU.  Writes profiles/prone_bench.txt.

    python tools/prone_bench.py [--out profiles/prone_bench.txt] [--repeats 20] [--rounds 3] [--no-reference]

Part 1: one Gaussian / ProNE iteration with M = (1 - mu) I - D^-1 (A + I) on an [N, F] matrix,
    u = M Lx1;  Lx2 = (M u - 2 Lx1) - Lx0;  conv += c Lx2
fused (two filter_step launches) and unfused (two csrspmm launches and a dozen elementwise kernels), on the arxiv-shaped graphs of
cogdl_amd/synth.py (169,343 nodes, 2.5 M entries with the self loops; uniform and R-MAT) at F = 128 and F = 32.  Before anything
is timed the two routes are compared bit for bit on the same inputs.  Device events around one iteration; per round `--warmup`
iterations, then the median of `--repeats`; the two routes alternate inside a round and the table gives the median round with
the range over the rounds.  GB/s = the bytes the fused iteration needs (computed from the shapes, below) over its time: a rate
of the whole iteration, not a kernel's share of peak.
Part 2: embedding.prone (dim 128, step 5) on the GPU, median of three runs with the host clock around a synchronise, against
one run of the reference's ProNE.forward on the same graph on the host (networkx, scipy, sklearn; the reference package from
oracle/_ref/pkg or $COGDL_REFERENCE -- where it is absent, or with --no-reference, the line says so)."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import cogdl_amd  # noqa: E402
from cogdl_amd import embedding, synth  # noqa: E402
from cogdl_amd.operators.spectral import filter_step  # noqa: E402
from cogdl_amd.operators.spmm import csrspmm  # noqa: E402

MU, COEF = 0.2, 0.0515


def fused_bytes(n, e, f):
    """One fused iteration: each step reads colind and one gathered row per entry, rowptr and dst_scale; the first reads its
    own x row again and writes u; the second reads u's row, Lx1, Lx0 and conv and writes Lx2 and conv."""
    per_step = 4 * e + 4 * f * e + 4 * (n + 1) + 4 * n
    return 2 * per_step + 4 * f * n * (2 + 6)


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


def iteration_routes(rp, ci, scale, lx0, lx1, conv_f, conv_u):
    n, f = lx1.shape
    u, lx2 = torch.empty_like(lx1), torch.empty_like(lx1)
    col = scale.unsqueeze(1)
    one_mu, two, c = (torch.tensor(v, dtype=torch.float32, device=lx1.device) for v in (1.0 - MU, -2.0, COEF))

    def fused():
        filter_step(rp, ci, None, lx1, a=-1.0, dst_scale=scale, b=1.0 - MU, out=u)
        filter_step(rp, ci, None, u, a=-1.0, dst_scale=scale, b=1.0 - MU, z1=lx1, c1=-2.0, z2=lx0, c2=-1.0, acc=conv_f, d=COEF, out=lx2)
        return lx2

    def unfused():
        v = -(col * csrspmm(rp, ci, lx1, None)) + one_mu * lx1
        y = -(col * csrspmm(rp, ci, v, None)) + one_mu * v
        y = y + two * lx1
        y = y - lx0
        conv_u.add_(c * y)
        return y

    return fused, unfused


def reference_model():
    staged = os.path.join(ROOT, "oracle", "_ref", "pkg")
    ref = staged if os.path.isdir(os.path.join(staged, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "cogdl")):
        return None, None, "reference package not present"
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")  # the reference writes into its own tree when imported
    shutil.copytree(os.path.join(ref, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
    cogdl_amd.install()
    try:
        from cogdl.data import Graph
        from cogdl.models.emb.prone import ProNE
    except Exception as e:  # (a dependency of the package that this machine lacks)
        return None, None, "reference package does not import: %s" % e
    return ProNE, Graph, None


def simple_adjacency(g):
    """The synthetic graph without its self loops -> int64 (indptr, indices) on the CPU."""
    n = g.num_nodes
    row = torch.repeat_interleave(torch.arange(n), g.degrees())
    col = g.colind.long()
    keep = row != col
    indptr = torch.zeros(n + 1, dtype=torch.long)
    torch.cumsum(torch.bincount(row[keep], minlength=n), 0, out=indptr[1:])
    return indptr, col[keep].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prone_bench.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the arxiv-shaped graphs (rehearsals only)")
    ap.add_argument("--no-reference", action="store_true", help="skip the host run of the reference's ProNE.forward")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prone_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda:0")
    lines = ["# fused filter step vs csrspmm + torch elementwise, one Gaussian iteration (mu %.1f) on %s" % (MU, torch.cuda.get_device_name(0)),
             "# ms per iteration (device events), median of %d, median [min .. max] over %d alternating rounds; GB/s = algorithmic "
             "bytes of the fused iteration / its time" % (args.repeats, args.rounds),
             "# graph | F | fused ms | unfused ms | unfused / fused | fused GB/s"]
    graphs = {}
    for topology in ("uniform", "rmat"):
        graphs[topology] = synth.arxiv_like(seed=0, topology=topology) if args.scale == 1.0 else \
            synth.scaled(max(64, int(169_343 * args.scale)), 13.8, seed=0, topology=topology)
    for topology, g in graphs.items():
        n, e = g.num_nodes, g.nnz
        rp, ci = g.rowptr.to(dev), g.colind.to(dev)
        scale = (1.0 / g.degrees().float()).to(dev)
        for f in (128, 32):
            gen = torch.Generator().manual_seed(f)
            lx0, lx1, conv = (torch.randn(n, f, generator=gen).to(dev) for _ in range(3))
            conv_f, conv_u = conv.clone(), conv.clone()
            fused, unfused = iteration_routes(rp, ci, scale, lx0, lx1, conv_f, conv_u)
            with torch.no_grad():
                a, b = fused(), unfused()  # faster and different is not faster
                assert torch.equal(a, b) and torch.equal(conv_f, conv_u), "the two routes differ"
                t_f, t_u = [], []
                for _ in range(args.rounds):
                    t_f.append(median_ms(fused, args.warmup, args.repeats))
                    t_u.append(median_ms(unfused, args.warmup, args.repeats))
            mf, mu_ = statistics.median(t_f), statistics.median(t_u)
            lines.append("arxiv-shaped %s (%d nodes, %d entries) | %d | %.3f [%.3f .. %.3f] | %.3f [%.3f .. %.3f] | %.2fx | %.0f"
                         % (topology, n, e, f, mf, min(t_f), max(t_f), mu_, min(t_u), max(t_u), mu_ / mf,
                            fused_bytes(n, e, f) / (mf * 1e-3) / 1e9))
            print(lines[-1], flush=True)

    g = graphs["uniform"]
    indptr, indices = simple_adjacency(g)
    csr = (indptr.to(dev), indices.to(dev))
    dim = min(128, g.num_nodes - 1)
    times = []
    for i in range(4):  # (the first run warms every shape up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        emb = embedding.prone(csr, dim=dim, step=5, mu=0.2, theta=0.5, seed=1)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert torch.isfinite(emb).all()
    ours = statistics.median(times[1:])
    lines += ["# whole ProNE (dim %d, step 5, mu 0.2, theta 0.5) on the arxiv-shaped uniform graph without self loops (%d nodes, %d "
              "entries): seconds, host clock around a synchronise" % (dim, g.num_nodes, indices.numel()),
              "embedding.prone on the GPU | %.3f s (median of 3 after a warm-up run; %.3f .. %.3f)" % (ours, min(times[1:]), max(times[1:]))]
    print(lines[-1], flush=True)
    model_cls, graph_cls, why = (None, None, "--no-reference") if args.no_reference else reference_model()
    if model_cls is None:
        lines.append("reference ProNE.forward on the host | unmeasured (%s)" % why)
    else:
        row = torch.repeat_interleave(torch.arange(g.num_nodes), indptr[1:] - indptr[:-1])
        keep = row < indices
        graph = graph_cls(edge_index=torch.stack([row[keep], indices[keep]]), num_nodes=g.num_nodes)
        print("running the reference's ProNE.forward on the host ...", flush=True)
        t0 = time.perf_counter()
        ref = model_cls(dim, 5, 0.2, 0.5).forward(graph)
        theirs = time.perf_counter() - t0
        assert ref.shape == (g.num_nodes, dim)
        lines.append("reference ProNE.forward on the host | %.1f s (one run) | %.0fx" % (theirs, theirs / ours))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
