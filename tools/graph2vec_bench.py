"""Graph2Vec benchmark: the two operators behind cogdl_amd.embedding.graph2vec on two synthetic batches (cogdl_amd/synth.py's
uniform pairs, one block of node ids per graph):

    dense   5000 graphs of 74 nodes, mean degree 66
    sparse  12000 graphs of 390 nodes, mean degree 2.5

  (a) wl_labels (2 rounds after round 0) on the batched CSR, on the GPU and on the host twin; per call and per round
  (b) doc2vec_dbow on the WL documents (dim 128, negative 5, min_count 5), throughput mode, on the GPU and on the host twin
      (OpenMP); per call of --epochs epochs and per epoch
  (c) a restatement of the reference's interpreted extractor (cogdl/models/emb/graph2vec.py:63-78: one md5 of a joined string
      per node and round over adjacency lists) on the host, on the first --ref-graphs graphs

GPU calls are timed with device events after a warm-up, the public calls with the flag read-back included; the median of
--reps calls is reported.  Prints one JSON document and writes it to --out.  Needs a GPU.

    python tools/graph2vec_bench.py --out profiles/graph2vec_bench.txt
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators import doc2vec_dbow, wl_labels  # noqa: E402

SHAPES = (("dense", 5000, 74, 66.0), ("sparse", 12000, 390, 2.5))


def gpu_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(times):
    times = sorted(times)
    return {"ms": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4)}


def batch(graphs, nodes, degree, seed=0):
    """-> (indptr int32, indices int32, label0 int64, graph_of int64) of the simple symmetric batch, on the CPU."""
    per_graph = int(nodes * degree / 2)
    src, dst = synth.uniform_pairs(nodes, graphs * per_graph, seed)
    block = torch.repeat_interleave(torch.arange(graphs), per_graph) * nodes
    src, dst, total = src.long() + block, dst.long() + block, graphs * nodes
    keep = src != dst
    keys = torch.unique(torch.cat([src[keep] * total + dst[keep], dst[keep] * total + src[keep]]))
    row, col = keys // total, keys % total
    indptr = torch.zeros(total + 1, dtype=torch.long)
    torch.cumsum(torch.bincount(row, minlength=total), 0, out=indptr[1:])
    return indptr.int(), col.int(), (indptr[1:] - indptr[:-1]).long(), torch.arange(total) // nodes


def documents(labels, classes, graph_of, graphs, min_count=5):
    offset = torch.cumsum(classes, 0) - classes
    tok = torch.cat([offset[r] + labels[r].long() for r in range(labels.shape[0])])
    doc = graph_of.repeat(labels.shape[0])
    order = torch.sort(doc, stable=True)[1]
    keep = torch.bincount(tok, minlength=int(classes.sum())) >= min_count
    new_id = torch.cumsum(keep, 0) - 1
    words = torch.where(keep[tok], new_id[tok], torch.full_like(tok, -1))[order].contiguous()
    doc_ptr = torch.zeros(graphs + 1, dtype=torch.long)
    torch.cumsum(torch.bincount(doc, minlength=graphs), 0, out=doc_ptr[1:])
    return doc_ptr, words, int(keep.sum())


def interpreted_extractor(indptr, indices, label0, first, last, rounds):
    """wl_iterations, restated on adjacency lists: strings, sorted, joined, md5."""
    ip, ix = indptr.tolist(), indices.tolist()
    words = 0
    features = {v: label0[v] for v in range(first, last)}
    for _ in range(rounds):
        new = {}
        for v in range(first, last):
            feats = [features[v]] + sorted(features[u] for u in ix[ip[v]:ip[v + 1]])
            new[v] = hashlib.md5("_".join(str(x) for x in feats).encode()).hexdigest()
        words += len(new)
        features = new
    return words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--ref-graphs", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "graph2vec_bench needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "epochs": args.epochs}
    for name, graphs, nodes, degree in SHAPES:
        indptr, indices, label0, graph_of = batch(graphs, nodes, degree)
        row = {"graphs": graphs, "num_nodes": int(label0.numel()), "num_edges": int(indices.numel()),
               "max_degree": int(label0.max())}
        d = (indptr.to(dev), indices.to(dev), label0.to(dev))
        for _ in range(2):
            labels, classes = wl_labels(*d, args.rounds)
        wl = stats([gpu_ms(lambda: wl_labels(*d, args.rounds)) for _ in range(args.reps)])
        wl["ms_per_round"] = round(wl["ms"] / (args.rounds + 1), 4)
        wl["classes"] = classes.tolist()
        host_labels = wl_labels(indptr, indices, label0, args.rounds)
        assert torch.equal(host_labels[0], labels.cpu()) and torch.equal(host_labels[1], classes.cpu())
        wl_host = stats([host_ms(lambda: wl_labels(indptr, indices, label0, args.rounds)) for _ in range(args.host_reps)])
        wl_host["ms_per_round"] = round(wl_host["ms"] / (args.rounds + 1), 4)
        row["wl_labels"] = {"gpu": wl, "host_twin": wl_host, "host_over_gpu": round(wl_host["ms"] / wl["ms"], 2)}

        last = args.ref_graphs * nodes
        t0 = time.perf_counter()
        n_words = interpreted_extractor(indptr, indices, label0.tolist(), 0, last, args.rounds)
        ref_s = time.perf_counter() - t0
        row["interpreted_extractor_host"] = {"graphs": args.ref_graphs, "words": n_words, "s": round(ref_s, 3),
                                             "ms_scaled_to_the_batch": round(ref_s * 1e3 * graphs / args.ref_graphs, 1)}

        doc_ptr, words, vocab = documents(host_labels[0], host_labels[1], graph_of, graphs)
        kw = dict(dim=128, negative=5, epochs=args.epochs, seed=1)
        dd = (doc_ptr.to(dev), words.to(dev))
        for _ in range(2):
            doc2vec_dbow(*dd, vocab, **kw)
        pv = stats([gpu_ms(lambda: doc2vec_dbow(*dd, vocab, **kw)) for _ in range(args.reps)])
        pv["ms_per_epoch"] = round(pv["ms"] / args.epochs, 4)
        pv_host = stats([host_ms(lambda: doc2vec_dbow(doc_ptr, words, vocab, **kw)) for _ in range(args.host_reps)])
        pv_host["ms_per_epoch"] = round(pv_host["ms"] / args.epochs, 4)
        kept = int((words >= 0).sum())
        pv["words_per_s"] = round(kept * args.epochs / (pv["ms"] * 1e-3), 1)
        row["doc2vec_dbow"] = {"words": int(words.numel()), "kept_words": kept, "vocabulary": vocab, "gpu": pv, "host_twin": pv_host,
                               "host_over_gpu": round(pv_host["ms"] / pv["ms"], 2)}
        res[name] = row
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
