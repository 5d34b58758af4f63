"""Times the making of knowledge-graph training batches through cogdl_amd.kgsample.TrainBatches (cogdl_hip_kg_train_batch,
csrc/kgsample.hip) against the reference's own loader -- TripleDataWrapper.output_iter: two TrainDatasets behind two CPU
DataLoaders and BidirectionalOneShotIterator, plus the host-to-device copy train_step performs -- in the same process, both at
this commit.  Needs a GPU and the reference package (oracle/_ref/pkg or $COGDL_REFERENCE).  Writes profiles/kgsample_bench.txt.

    python tools/kgsample_bench.py [--out profiles/kgsample_bench.txt] [--repeats 5] [--inner 4] [--no-steps]

Shape: FB15k-237's (14541 entities, 237 relations, 272115 training triples), B = 1024 positives with K = 128 negatives each (the
reference's defaults).  The dataset itself is not at hand: heads and tails are drawn independently with probability
proportional to (rank + 1)^-1.0 over a random ranking of the entities, relations with (rank + 1)^-1.0 (Zipf laws; seed 1), so
a few (relation, tail) groups collect thousands of true heads, as the real graph's do.
Per batch: next(iterator) and, for the reference, the three .to(device) of train_step; the two routes alternate window by
window, the host clock around `--inner` batches that end in a device synchronise, the median of `--repeats` windows with the
spread (min .. max).  One-off: train_tables on the device against TrainDataset.__init__ twice (one per mode), once each.
Per training step (unless --no-steps): the reference's TripleModelWrapper.train_step + backward at hidden 1000 with
install(kg_train=True) in both routes, for the four models, fed by the reference's loader or by TrainBatches."""
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
from cogdl_amd.kgsample import TrainBatches, train_tables  # noqa: E402
from cogdl_amd.operators.kgsample import LDS_LIST  # noqa: E402

N, RELS, T, HIDDEN, GAMMA, B, K = 14541, 237, 272115, 1000, 12.0, 1024, 128
ENTITY_EXPONENT, RELATION_EXPONENT = 1.0, 1.0
MODELS = (("transe", "TransE", False, False), ("distmult", "DistMult", False, False), ("complex", "ComplEx", True, True),
          ("rotate", "RotatE", True, False))


def synthetic_triples():
    gen = torch.Generator().manual_seed(1)

    def zipf(count, exponent, size):
        weight = (torch.arange(count, dtype=torch.float64) + 1) ** -exponent
        return torch.randperm(count, generator=gen)[torch.multinomial(weight, size, replacement=True, generator=gen)]

    return torch.stack([zipf(N, ENTITY_EXPONENT, T), zipf(RELS, RELATION_EXPONENT, T), zipf(N, ENTITY_EXPONENT, T)], dim=1)


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def alternate(ours, theirs, repeats, inner):
    t_new, t_ref = [], []
    for _ in range(repeats + 1):  # (the first pair of windows is the warm-up)
        t_new.append(window(ours, inner))
        t_ref.append(window(theirs, inner))
    return t_new[1:], t_ref[1:]


def cols(ts):
    return "%9.3f %19s" % (statistics.median(ts) * 1e3, "(%.3f .. %.3f)" % (min(ts) * 1e3, max(ts) * 1e3))


def reference_package():
    ref = os.path.join(ROOT, "oracle", "_ref", "pkg")
    ref = ref if os.path.isdir(os.path.join(ref, "cogdl")) else os.environ.get("COGDL_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "cogdl")):
        raise SystemExit("tools/kgsample_bench.py needs the reference package (oracle/_ref/pkg or $COGDL_REFERENCE)")
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")  # the reference writes into its own tree when imported
    shutil.copytree(os.path.join(ref, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.join(ROOT, "tests", "golden", "_stubs"), scratch]
    return scratch


class Data:
    def __init__(self, triples):
        self.triples, self._num_entities, self._num_relations = triples, N, RELS
        self.train_start_idx, self.valid_start_idx = 0, len(triples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kgsample_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--no-steps", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kgsample_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    scratch = reference_package()
    cogdl_amd.install(kg_train=True)
    import importlib

    from cogdl.datasets.kg_data import TrainDataset
    from cogdl.wrappers.data_wrapper.link_prediction.triple_link_prediction_dw import TripleDataWrapper
    from cogdl.wrappers.model_wrapper.link_prediction.triple_link_prediction_mw import TripleModelWrapper

    triples = synthetic_triples()
    as_tuples = [tuple(row) for row in triples.tolist()]
    lines = ["kgsample_bench on %s: training batches at FB15k-237 shape, N %d, %d relations, T %d, B %d, K %d" % (
                 torch.cuda.get_device_name(0), N, RELS, T, B, K),
             "synthetic triples: head, tail ~ (rank + 1)^-%.2f over a random ranking of the entities, relation ~ (rank + 1)^-%.1f, "
             "independent, seed 1" % (ENTITY_EXPONENT, RELATION_EXPONENT),
             "ms, median of %d windows of %d calls (min .. max), the two routes alternating window by window" % (args.repeats, args.inner),
             ""]
    # ---- one-off: the tables
    train_tables(triples[:4096].to(dev), N)  # (warm-up: torch loads its sort / unique kernels on first use)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tables = train_tables(triples.to(dev), N)
    torch.cuda.synchronize()
    t_tables = time.perf_counter() - t0
    t0 = time.perf_counter()
    for mode in ("head-batch", "tail-batch"):
        TrainDataset(as_tuples, N, RELS, K, mode)
    t_datasets = time.perf_counter() - t0
    lines.append("one-off  train_tables on the device (triples already there) %.1f ms | TrainDataset.__init__ x 2 %.1f ms | %.0fx" % (
        t_tables * 1e3, t_datasets * 1e3, t_datasets / t_tables))
    for mode, m in tables.modes.items():
        lens = (m.list_ptr[1:] - m.list_ptr[:-1])
        long_rows = (lens[m.group.long()] > LDS_LIST)
        perm = torch.randperm(T, device=dev)[:T // B * B].view(-1, B)
        lines.append("%s: %d groups, largest true list %d ids; %.2f%% of the positives and %.1f%% of the batches of a shuffled epoch "
                     "take the long-list path (more than %d ids)" % (mode, lens.numel(), int(lens.max()), 100 * long_rows.float().mean().item(),
                                                                     100 * long_rows[perm].any(dim=1).float().mean().item(), LDS_LIST))
    del tables
    # ---- per batch
    ours_it = TrainBatches(triples, N, K, B, seed=1, device=dev)
    ref_it = TripleDataWrapper.output_iter(Data(as_tuples), K, B)

    def ours():
        return next(ours_it)

    def theirs():
        positive, negative, weight, mode = next(ref_it)
        return positive.to(dev), negative.to(dev), weight.to(dev), mode

    a, b = ours(), theirs()
    assert a[3] == b[3] and all(x.dtype == y.dtype and x.shape == y.shape and x.device == y.device for x, y in zip(a[:3], b[:3]))
    t_new, t_ref = alternate(ours, theirs, args.repeats, args.inner)
    head = "%-34s | %9s %19s | %9s %19s | %8s" % ("", "new ms", "(min .. max)", "ref ms", "(min .. max)", "speed-up")
    lines += ["", head, "-" * len(head)]
    ratio = statistics.median(t_ref) / statistics.median(t_new)
    lines.append("%-34s | %s | %s | %7.1fx" % ("per batch (loader only)", cols(t_new), cols(t_ref), ratio))
    verdict = statistics.median(t_new) <= statistics.median(t_ref)
    print("\n".join(lines), flush=True)
    # ---- per training step
    if not args.no_steps:
        for name, cls, dbl_e, dbl_r in MODELS:
            model = getattr(importlib.import_module("cogdl.models.emb." + name), cls)(N, RELS, HIDDEN, GAMMA, dbl_e, dbl_r).to(dev)
            mw = TripleModelWrapper.__new__(TripleModelWrapper)  # (its __init__ parses the command line)
            torch.nn.Module.__init__(mw)
            mw.model = model
            mw.args = argparse.Namespace(negative_adversarial_sampling=False, adversarial_temperature=1.0, uni_weight=False,
                                         regularization=1e-9)

            def step(it):
                model.zero_grad(set_to_none=True)
                mw.train_step(it).backward()

            s_new, s_ref = alternate(lambda: step(ours_it), lambda: step(ref_it), args.repeats, args.inner)
            line = "%-34s | %s | %s | %7.1fx" % ("train_step + backward, " + name, cols(s_new), cols(s_ref),
                                                  statistics.median(s_ref) / statistics.median(s_new))
            print(line, flush=True)
            lines.append(line)
            del model, mw
            torch.cuda.empty_cache()
    lines += ["", "new: cogdl_amd.kgsample.TrainBatches on the device (one launch per batch, no read-back).  ref: the reference's",
              "  BidirectionalOneShotIterator over two CPU DataLoaders (num_workers 0, as TripleDataWrapper builds them) plus the three",
              "  host-to-device copies of train_step.  train_step rows: install(kg_train=True) in both routes, no optimizer step.",
              "the device iterator is not slower per batch than the reference's loader: %s" % ("yes" if verdict else "NO")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    shutil.rmtree(scratch, ignore_errors=True)
    print("\n".join(lines[-5:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
