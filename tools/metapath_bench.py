"""Metapath-walk benchmark (cogdl_amd.operators.walk.metapath_walk) on the arxiv-shaped uniform graph:

  (a) metapath_walk with 3 random node types, L = 80, schema "0-1-0,0-2-0,1-0-2-0-1": one walker per node and metapath whose
      first type the node has; also the one-off cost of the typed row layout (typed_rows, cache cleared each time)
  (b) the T == 1 case (all types 0, schema "0-0") against random_walk on the same graph, every node a start: both draw the
      same numbers and touch the same memory, so the ratio is what the typed indexing (seg[v * T + t], the pattern table,
      the end-of-walk test, `lengths`) costs.  The two are timed alternately.
  (c) a restatement of the reference's interpreted loop (cogdl/models/emb/metapath2vec.py:87-125: per step the neighbour
      list is filtered by comparing type strings, then random.choice) on the host, on the first --ref-nodes start nodes

Timed with device events after warm-up; the calls are the public ones (flag read-back included).  A rate is positions that
hold a node per second (walks end early where no neighbour has the wanted type).  Prints one JSON document and writes it to
--out.  Needs a GPU.

    python tools/metapath_bench.py --out profiles/metapath_bench.txt
"""
import argparse
import json
import os
import random
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cogdl_amd import synth  # noqa: E402
from cogdl_amd.operators import walk as walk_mod  # noqa: E402
from cogdl_amd.operators.walk import metapath_walk, parse_schema, random_walk, typed_rows  # noqa: E402

SCHEMA = "0-1-0,0-2-0,1-0-2-0-1"


def gpu_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def stats(times):
    times = sorted(times)
    return {"ms": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4)}


def starts_for(node_type, paths):
    start, which = [], []
    for p, items in enumerate(paths):
        nodes = torch.nonzero(node_type == items[0]).flatten()
        start.append(nodes)
        which.append(torch.full((nodes.numel(),), p, dtype=torch.int32, device=nodes.device))
    return torch.cat(start), torch.cat(which)


def reference_loop(neighbours, node_type, starts, schemas, length, rng):
    """The reference's _walk, restated: strings for types, a candidate list per step, random.choice."""
    held = 0
    for node, schema in zip(starts, schemas):
        items = schema.split("-")
        walk = [node]
        while len(walk) < length:
            candidates = []
            for x in list(neighbours[walk[-1]]):
                if node_type[x] == items[len(walk) % (len(items) - 1)]:
                    candidates.append(x)
            if not candidates:
                break
            walk.append(rng.choice(candidates))
        held += len(walk)
    return held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--length", type=int, default=80)
    ap.add_argument("--ref-nodes", type=int, default=3000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metapath_bench needs a GPU"
    dev = torch.device("cuda:0")
    g = synth.arxiv_like(seed=0, topology="uniform")
    n = g.num_nodes
    ip_h, ix_h = g.rowptr.long(), g.colind.long()
    ip, ix = ip_h.to(dev), ix_h.to(dev)
    types_h = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(0))
    types = types_h.to(dev)
    paths = parse_schema(SCHEMA)
    res = {"device": torch.cuda.get_device_name(0), "length": args.length, "reps": args.reps, "num_nodes": n,
           "num_edges": int(ix.numel()), "schema": SCHEMA}

    # (a) typed walk
    start, which = starts_for(types, paths)

    def typed():
        return metapath_walk(ip, ix, types, start, SCHEMA, args.length, walker_path=which, seed=1, return_lengths=True)

    layout = []
    for _ in range(3):
        walk_mod._TYPED.clear()
        torch.cuda.synchronize()
        layout.append(gpu_ms(lambda: typed_rows(ip, ix, types)))
    for _ in range(2):
        _, lengths = typed()
    held = int(lengths.long().sum())
    row = stats([gpu_ms(typed) for _ in range(args.reps)])
    row.update({"walkers": int(start.numel()), "positions_held": held, "mean_length": round(held / start.numel(), 2),
                "positions_per_s": round(held / (row["ms"] * 1e-3), 1), "typed_rows_build": stats(layout)})
    res["metapath_walk_3_types"] = row

    # (b) T == 1 against random_walk, alternating
    every = torch.arange(n, device=dev)
    zeros = torch.zeros(n, dtype=torch.int32, device=dev)
    one_type = lambda: metapath_walk(ip, ix, zeros, every, "0-0", args.length, seed=1)  # noqa: E731
    first_order = lambda: random_walk(ip, ix, every, args.length, seed=1)  # noqa: E731
    assert torch.equal(one_type(), first_order()) or bool((ip[1:] == ip[:-1]).any())  # (equal on a graph without dead ends)
    first_order()
    a, b = [], []
    for _ in range(args.reps):
        a.append(gpu_ms(one_type))
        b.append(gpu_ms(first_order))
    a, b = stats(a), stats(b)
    steps = n * (args.length - 1)
    a["steps_per_s"], b["steps_per_s"] = round(steps / (a["ms"] * 1e-3), 1), round(steps / (b["ms"] * 1e-3), 1)
    res["one_type"] = {"metapath_walk": a, "random_walk": b, "metapath_over_random_walk": round(a["ms"] / b["ms"], 3)}

    # (c) the interpreted loop on the host
    ip_l, ix_l = ip_h.tolist(), ix_h.tolist()
    neighbours = [ix_l[ip_l[v]:ip_l[v + 1]] for v in range(n)]
    type_str = [str(t) for t in types_h.tolist()]
    k = min(args.ref_nodes, int(start.numel()))
    sub_start, sub_schema = start[:k].tolist(), [SCHEMA.split(",")[p] for p in which[:k].tolist()]
    t0 = time.perf_counter()
    ref_held = reference_loop(neighbours, type_str, sub_start, sub_schema, args.length, random.Random(0))
    ref_s = time.perf_counter() - t0
    res["interpreted_loop_host"] = {"walkers": k, "positions_held": ref_held, "s": round(ref_s, 3),
                                    "positions_per_s": round(ref_held / ref_s, 1),
                                    "kernel_over_loop_rate": round(row["positions_per_s"] / (ref_held / ref_s), 1)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
