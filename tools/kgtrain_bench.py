"""Times the forward + backward of a batch of negative scores through sampled_scores (cogdl_hip_kg_score*, csrc/kgscore.hip)
against the reference's own KGEModel.forward + autograd on the same GPU, in the same process, both at this commit.  Needs a
GPU.  Writes profiles/kgtrain_bench.txt.

    python tools/kgtrain_bench.py [--out profiles/kgtrain_bench.txt] [--repeats 5] [--inner 20] [--no-reference]

Shape: FB15k-237 (14541 entities, 237 relations), hidden 1000, gamma 12, B = 1024 positives with K = 128 negatives each (the
reference's defaults), the four models with the reference's default widths (entity rows 1000 for transe and distmult, 2000 for
complex and rotate), head-batch and tail-batch.  Tables as KGEModel.__init__ draws them; ids uniform.
New route: cogdl_amd.kgtrain.score_triples(...).backward(g) with a fixed upstream gradient g [B, K]: the [B, D] query in torch,
the three kernels, the inverted index (one stable sort per backward), the validation read-back, torch's [B, D] index backward
into both tables -- everything a training step pays for its negative scores.
Reference route: the reference package's own model class (oracle/_ref/pkg or $COGDL_REFERENCE; without it, or with
--no-reference, the columns say so): model((positive, negative), mode).backward(g) on the same tensors.
Timing: the host clock around `--inner` iterations that end in a device synchronise; every shape is warmed up first; the two
routes alternate window by window and the median of `--repeats` windows is reported with the spread (min .. max).  Both routes
score the same inputs before anything is timed and the table gives the largest differences.
Bytes: what the new route's three kernels must move, computed from the shapes -- forward and grad_q each read B K rows of D
floats, grad_table reads B K query rows and the table and writes the table once -- over the time of the WHOLE call: a
whole-call rate, not a kernel's share of peak.  Peak memory: torch.cuda.max_memory_allocated over one forward + backward of
each route, tables and their gradients included."""
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

from cogdl_amd.kgtrain import score_triples  # noqa: E402

N, RELS, HIDDEN, GAMMA, B, K = 14541, 237, 1000, 12.0, 1024, 128
MODELS = (("transe", "TransE", False, False), ("distmult", "DistMult", False, False), ("complex", "ComplEx", True, True),
          ("rotate", "RotatE", True, False))
MODES = ("head-batch", "tail-batch")


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def reference_classes():
    ref = os.path.join(ROOT, "oracle", "_ref", "pkg")
    ref = ref if os.path.isdir(os.path.join(ref, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "cogdl")):
        return None, None
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")  # the reference writes into its own tree when imported
    shutil.copytree(os.path.join(ref, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
    import importlib

    return {name: getattr(importlib.import_module("cogdl.models.emb." + name), cls) for name, cls, *_ in MODELS}, scratch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kgtrain_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kgtrain_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    classes, scratch = (None, None) if args.no_reference else reference_classes()
    lines = ["kgtrain_bench on %s: forward + backward of the negative scores, N %d, hidden %d, B %d, K %d; ms per call, median of %d "
             "windows of %d calls (min .. max), the two routes alternating" % (torch.cuda.get_device_name(0), N, HIDDEN, B, K,
                                                                             args.repeats, args.inner),
             "reference route: %s" % ("the reference package's model classes, forward + autograd" if classes
                                      else "not measured (reference package absent or --no-reference)"), ""]
    head = "%-9s %-10s %5s | %8s %17s %8s %9s | %8s %17s %9s | %8s %8s %9s %9s" % (
        "model", "mode", "D", "new ms", "(min .. max)", "GB/s", "peak MiB", "ref ms", "(min .. max)", "peak MiB", "speed-up", "mem x",
        "d score", "d grad")
    lines += [head, "-" * len(head)]
    print("\n".join(lines), flush=True)
    verdict = []
    for name, cls, dbl_e, dbl_r in MODELS:
        d_e, d_r = HIDDEN * (2 if dbl_e else 1), HIDDEN * (2 if dbl_r else 1)
        gen = torch.Generator().manual_seed(1)
        emb_range = (GAMMA + 2.0) / HIDDEN
        model = None
        if classes:
            model = classes[name](N, RELS, HIDDEN, GAMMA, dbl_e, dbl_r).to(dev)
            entity, relation = model.entity_embedding, model.relation_embedding
            emb_range = model.embedding_range.item()
        else:
            entity = ((torch.rand(N, d_e, generator=gen) * 2 - 1) * emb_range).to(dev).requires_grad_()
            relation = ((torch.rand(RELS, d_r, generator=gen) * 2 - 1) * emb_range).to(dev).requires_grad_()
        positive = torch.stack([torch.randint(0, N, (B,), generator=gen), torch.randint(0, RELS, (B,), generator=gen),
                                torch.randint(0, N, (B,), generator=gen)], dim=1).to(dev)
        negative = torch.randint(0, N, (B, K), generator=gen).to(dev)
        g = torch.randn(B, K, generator=gen).to(dev)
        bytes_moved = 4 * (3 * B * K * d_e + 2 * N * d_e)
        for mode in MODES:
            def ours():
                entity.grad = relation.grad = None
                s = score_triples(name, entity, relation, (positive, negative), mode, emb_range, GAMMA)
                s.backward(g)
                return s

            def theirs():
                entity.grad = relation.grad = None
                s = model((positive, negative), mode)
                s.backward(g)
                return s

            s_new = ours().detach()
            grad_new = entity.grad.clone()
            d_score = d_grad = float("nan")
            if model is not None:
                s_ref = theirs().detach()
                d_score = float((s_new - s_ref).abs().max())
                d_grad = float((grad_new - entity.grad).abs().max())
                del s_ref
            del grad_new
            t_new, t_ref = [], []
            for _ in range(args.repeats + 1):  # (the first pair of windows is the warm-up)
                t_new.append(window(ours, args.inner))
                if model is not None:
                    t_ref.append(window(theirs, args.inner))
            t_new, t_ref = t_new[1:], t_ref[1:]
            entity.grad = relation.grad = None
            mem_new = peak_of(ours)
            entity.grad = relation.grad = None
            med = statistics.median(t_new)
            ref_cols = "%8s %17s %9s | %8s %8s %9s %9s" % ("-", "-", "-", "-", "-", "-", "-")
            if model is not None:
                mem_ref = peak_of(theirs)
                entity.grad = relation.grad = None
                med_ref = statistics.median(t_ref)
                ref_cols = "%8.2f %17s %9.0f | %7.1fx %7.1fx %9.2e %9.2e" % (
                    med_ref * 1e3, "(%.2f .. %.2f)" % (min(t_ref) * 1e3, max(t_ref) * 1e3), mem_ref / 2 ** 20, med_ref / med,
                    mem_ref / mem_new, d_score, d_grad)
                verdict.append((name, mode, med <= med_ref, mem_new < mem_ref))
            line = "%-9s %-10s %5d | %8.2f %17s %8.0f %9.0f | %s" % (
                name, mode, d_e, med * 1e3, "(%.2f .. %.2f)" % (min(t_new) * 1e3, max(t_new) * 1e3), bytes_moved / med / 1e9,
                mem_new / 2 ** 20, ref_cols)
            print(line, flush=True)
            lines.append(line)
        del model, entity, relation
        torch.cuda.empty_cache()
    lines += ["", "GB/s: 4 (3 B K D + 2 N D) bytes -- what the three kernels must move -- over the whole call's time (query, sort, index",
              "  backward and read-back included): a whole-call rate, not a kernel's share of the 8 TB/s HBM peak.",
              "peak MiB: torch.cuda.max_memory_allocated over one forward + backward, tables and gradients included.",
              "d score / d grad: largest |difference| of the scores and of the entity table's gradient between the two routes (float32",
              "  sums in another order).  speed-up: reference ms over new ms.  mem x: reference peak over new peak."]
    if verdict:
        slow = ["%s %s" % (n, m) for n, m, fast, _ in verdict if not fast]
        big = ["%s %s" % (n, m) for n, m, _, small in verdict if not small]
        lines.append("not slower than the reference for every model and mode: %s" % ("yes" if not slow else "NO -- " + ", ".join(slow)))
        lines.append("smaller peak than the reference for every model and mode: %s" % ("yes" if not big else "NO -- " + ", ".join(big)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if scratch:
        shutil.rmtree(scratch, ignore_errors=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
