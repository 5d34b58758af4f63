"""Times knowledge-graph link-prediction evaluation on rank_all (cogdl_hip_kg_rank, csrc/kgrank.hip) against the reference's own
route on the same GPU, both at this commit.  Needs a GPU.  Writes profiles/kgrank_bench.txt.

    python tools/kgrank_bench.py [--out profiles/kgrank_bench.txt] [--repeats 3] [--ref-triples 256] [--no-reference]

Shapes: FB15k-237 (N = 14541 entities, 237 relations, 20466 test triples among 310116 true ones) and WN18 (N = 40943, 18
relations, 5000 test triples among 151442), hidden 1000, gamma 12, the four models with the reference's default widths
(entity rows 1000 for transe and distmult, 2000 for complex and rotate).  The triples are synthetic: (head, relation) pairs are
drawn from a pool so that a pair has several true tails, as in the real data; the tables are N(0, 0.5^2) entities and
relations uniform in the embedding range.
New route: prepare_query + rank_all over ALL test triples of a direction in one call, both directions, without and with the
filter lists (built once by filter_lists, outside the timed window, as the reference's TestDataset is built outside its loop).
The host clock around a device synchronise; one warm-up, then the median of `--repeats`.
Reference route: the reference package's own model class (oracle/_ref/pkg or $COGDL_REFERENCE; without it, or with
--no-reference, the columns say so) doing what TripleModelWrapper.eval_step does per batch on the device -- model((positive,
negative), mode) on [B, N] candidates, + filter_bias, argsort, position of the target -- with positive, negative and filter_bias
prebuilt on the device, so only device work is compared (the reference's per-triple Python walk over all entities and its
`.item()` per triple are left out, in its favour).  It runs `--ref-triples` triples per direction at its default
test_batch_size 4 and at the largest B whose [B, N, D] temporaries fit a fixed budget; the table scales that time to all test
triples (stated as such: "scaled").  Both routes rank those triples before anything is timed; the table says how many reference
positions fall outside the new route's tie bracket and by how many places at the most (float32 sums taken in another order
reorder near-ties at D = 1000; more than 16 places ends the run).
Share of peak: the operations the scoring needs, computed from the shapes -- dot: one fma = two FLOP per (query, candidate, k),
reported as TFLOP/s against the fp32 matrix peak of 157.3 TFLOP/s; l1: two vector operations (subtract, add of the magnitude), cl2: seven and a square root per
complex k, against the fp32 vector peak of 78.6 T lane-operations/s (157.3 TFLOP/s counts an fma as two) -- over the time of
the whole unfiltered call (query preparation, the target pass and the validation read-back included): a whole-call rate, not a
kernel's share.  Peak memory: torch.cuda.max_memory_allocated over each route, tables included."""
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

from cogdl_amd.kgrank import evaluate, filter_lists  # noqa: E402
from cogdl_amd.operators.kgrank import ranks  # noqa: E402

SHAPES = (("FB15k-237", 14541, 237, 20466, 310116), ("WN18", 40943, 18, 5000, 151442))
HIDDEN, GAMMA = 1000, 12.0
MODELS = (("transe", "TransE", False, False, 2.0, "vector"), ("distmult", "DistMult", False, False, 2.0, "matrix"),
          ("complex", "ComplEx", True, True, 2.0, "matrix"), ("rotate", "RotatE", True, False, 7.0, "vector"))
PEAK = {"matrix": 157.3e12, "vector": 78.65e12}
REF_BUDGET = 48 << 30  # bytes of [B, N, D] temporaries the large reference batch may take (about eight of them live at once)
MODES = ("head-batch", "tail-batch")


def synth_triples(n, rels, n_true, n_test, gen):
    pool_h = torch.randint(0, n, (max(n_true // 8, 1),), generator=gen)
    pool_r = torch.randint(0, rels, (pool_h.numel(),), generator=gen)
    pick = torch.randint(0, pool_h.numel(), (n_true,), generator=gen)
    true = torch.unique(torch.stack([pool_h[pick], pool_r[pick], torch.randint(0, n, (n_true,), generator=gen)], dim=1), dim=0)
    return true, true[torch.randperm(true.shape[0], generator=gen)[:n_test]]


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


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


def reference_inputs(triples, mode, filt_ptr, filt_idx, n):
    """positive [m, 3], negative [m, N], filter_bias [m, N] as TestDataset yields them, built on the device."""
    m, dev = triples.shape[0], triples.device
    free = 0 if mode == "head-batch" else 2
    target = triples[:, free]
    negative = torch.arange(n, device=dev).repeat(m, 1)
    bias = torch.zeros((m, n), device=dev)
    owner = torch.repeat_interleave(torch.arange(m, device=dev), (filt_ptr[1:] - filt_ptr[:-1]).long())
    ids = filt_idx.long()
    negative[owner, ids] = target[owner]
    bias[owner, ids] = -1.0
    rows = torch.arange(m, device=dev)
    negative[rows, target] = target
    bias[rows, target] = 0.0
    return triples, negative, bias, target


def reference_route(model, inputs, mode, batch):
    positive, negative, bias, target = inputs
    out = []
    with torch.no_grad():
        for lo in range(0, positive.shape[0], batch):
            score = model((positive[lo:lo + batch], negative[lo:lo + batch]), mode)
            score += bias[lo:lo + batch]
            argsort = torch.argsort(score, dim=1, descending=True)
            out.append((argsort == target[lo:lo + batch].view(-1, 1)).nonzero()[:, 1])
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kgrank_bench.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-triples", type=int, default=256)
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kgrank_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    classes, scratch = (None, None) if args.no_reference else reference_classes()
    lines = ["kgrank_bench on %s: all test triples, both directions; ms are medians of %d after one warm-up" %
             (torch.cuda.get_device_name(0), args.repeats),
             "reference route: %s" % ("the reference package's model classes, %d triples per direction, scaled to all" % args.ref_triples
                                      if classes else "not measured (reference package absent or --no-reference)"), ""]
    head = "%-10s %-9s %5s %9s | %9s %9s %7s %7s %9s | %11s %11s %6s %9s %8s %8s" % (
        "shape", "model", "D", "filt.ent", "raw ms", "filt ms", "Tflop|op", "% peak", "peak MiB", "ref B=4 ms", "ref B=big", "big B", "peak MiB", "speed-up", "moved")
    lines += [head, "-" * len(head)]
    print("\n".join(lines), flush=True)
    for shape, n, rels, n_test, n_true in SHAPES:
        gen = torch.Generator().manual_seed(1)
        true, test = synth_triples(n, rels, n_true, n_test, gen)
        true, test = true.to(dev), test.to(dev)
        lists = {mode: filter_lists(true, test, mode, n) for mode in MODES}
        entries = sum(int(v[1].numel()) for v in lists.values())
        for name, cls, dbl_e, dbl_r, ops, unit in MODELS:
            d_e, d_r = HIDDEN * (2 if dbl_e else 1), HIDDEN * (2 if dbl_r else 1)
            emb_range = (GAMMA + 2.0) / HIDDEN
            entity = (torch.randn(n, d_e, generator=gen) * 0.5).to(dev)
            relation = ((torch.rand(rels, d_r, generator=gen) * 2 - 1) * emb_range).to(dev)

            def ours(filtered, triples=test, which=lists):
                return [evaluate(name, entity, relation, triples, mode, emb_range, GAMMA, *(which[mode] if filtered else (None, None)))
                        for mode in MODES]

            t_raw = timed(lambda: ours(False), args.repeats)
            t_filt = timed(lambda: ours(True), args.repeats)
            mem = peak_of(lambda: ours(True))
            k_dim = d_e // 2 if name in ("rotate",) else d_e
            rate = ops * 2 * n_test * n * k_dim / t_raw
            ref_cols = "%11s %11s %6s %9s %8s %8s" % ("-", "-", "-", "-", "-", "-")
            if classes:
                model = classes[name](n, rels, HIDDEN, GAMMA, dbl_e, dbl_r).to(dev)
                with torch.no_grad():
                    model.entity_embedding.copy_(entity)
                    model.relation_embedding.copy_(relation)
                sub = test[:args.ref_triples]
                sub_lists = {mode: filter_lists(true, sub, mode, n) for mode in MODES}
                inputs = {mode: reference_inputs(sub, mode, *sub_lists[mode], n) for mode in MODES}
                big = int(max(4, min(sub.shape[0], REF_BUDGET // (8 * n * d_e * 4))))
                # the same triples on both routes: the reference's position inside the new route's tie bracket
                counts = ours(True, sub, sub_lists)
                moved, far = 0, 0
                for mode, c in zip(MODES, counts):
                    pos = reference_route(model, inputs[mode], mode, big)
                    lo, hi = ranks(c, "optimistic") - 1, ranks(c, "pessimistic") - 1
                    dist = torch.clamp(lo - pos, min=0) + torch.clamp(pos - hi, min=0)
                    moved, far = moved + int((dist > 0).sum()), max(far, int(dist.max()))
                    if far > 16:  # (float32 sums in another order move near-ties by a few places at D = 1000, never by many)
                        raise SystemExit("%s %s %s: a reference position %d places outside the tie bracket" % (shape, name, mode, far))
                scale = n_test / sub.shape[0]
                t4 = timed(lambda: [reference_route(model, inputs[mode], mode, 4) for mode in MODES], args.repeats) * scale
                tb = timed(lambda: [reference_route(model, inputs[mode], mode, big) for mode in MODES], args.repeats) * scale
                mem_ref = peak_of(lambda: [reference_route(model, inputs[mode], mode, big) for mode in MODES])
                ref_cols = "%11.1f %11.1f %6d %9.0f %7.1fx %5d/%-2d" % (t4 * 1e3, tb * 1e3, big, mem_ref / 2 ** 20, min(t4, tb) / t_filt, moved, far)
                del model, inputs
            line = "%-10s %-9s %5d %9d | %9.1f %9.1f %7.2f %7.1f %9.0f | %s" % (
                shape, name, d_e, entries, t_raw * 1e3, t_filt * 1e3, rate / 1e12, 100 * rate / PEAK[unit], mem / 2 ** 20, ref_cols)
            print(line, flush=True)
            lines.append(line)
            del entity, relation
            torch.cuda.empty_cache()
    lines += ["", "Tflop|op: per second over the whole unfiltered call -- dot: TFLOP/s, an fma counted as two (T fma/s is half of it);",
              "  l1 / cl2: T vector operations/s (l1: 2, cl2: 7 per complex k, the square root counted as nothing).",
              "% peak against 157.3 TFLOP/s (fp32 matrix) for dot and 78.65 T lane-operations/s (fp32 vector) for l1 / cl2.",
              "speed-up: the faster of the two reference batch sizes (scaled) over the filtered new route.",
              "moved a/b: of the 2 x %d triples both routes ranked, a reference positions lie outside the new route's tie bracket" % args.ref_triples,
              "  [greater, greater + equal], the farthest by b places: float32 sums taken in another order reorder near-ties.",
              "peak MiB: torch.cuda.max_memory_allocated of the filtered route, tables included; the reference's at the large B."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if scratch:
        shutil.rmtree(scratch, ignore_errors=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
