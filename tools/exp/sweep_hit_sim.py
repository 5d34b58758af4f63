#!/usr/bin/env python3
"""A CPU model of the L2 hit rate of the sweep's gathers (csrc/rowsweep.h) for a structure and an assignment of its rows to
groups.  numpy only.  **An estimate of a lockstep model, not a measurement** (DESIGN.md section 5 has the measured figures).

The model.  Group g is walked by wave g % n_waves (a further round of the same wave walks on where the last one ended); workgroup
b = wave // 4 runs on XCD b % 8, as the hardware deals workgroups.  The waves of an XCD advance in lockstep, one edge per step, in
wave order inside a step.  Every XCD has one LRU cache of whole gathered rows (512 bytes at F = 128 fp32: 8192 rows are 4 MiB).
Hit rate = gathers found in the cache / gathers.  The ideal for a partition of rows over XCDs is a cache that never evicts:
1 - distinct (XCD, gathered row) pairs / gathers.

A group's edges are merged the way cogdl_amd/sweepplan.py merges them: stably by the gathered row (`backward`, a structure whose
rows ascend -- the stable transpose), or by the running maximum of the column inside the row (`forward`).

Usage: python tools/exp/sweep_hit_sim.py [--nodes N --degree D --seed S] [--direction backward|forward] [--rows R] [--waves W]
       (default: the benchmark's graph, synth.arxiv_like(0), R and W of the MI355X)"""
import argparse
import collections
import os
import sys

import numpy as np

CAPACITIES = (4096, 6144, 8192)


def consecutive(n_rows, r):
    """The assignment [n_groups, r] of groups of r consecutive rows (-1 = pad)."""
    n_groups = -(-n_rows // r)
    a = np.full(n_groups * r, -1, dtype=np.int64)
    a[:n_rows] = np.arange(n_rows)
    return a.reshape(n_groups, r)


def merge_key(ptr, ind, forward=False):
    """What a group's edges are merged by: the gathered row, or (forward) the running maximum of the column inside the row."""
    ptr, ind = np.asarray(ptr, dtype=np.int64), np.asarray(ind, dtype=np.int64)
    if not forward or not len(ind):
        return ind
    row = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    stride = int(ind.max()) + 1
    return np.maximum.accumulate(ind + row * stride) - row * stride


def deal_by_degree(ptr, r, key=None):
    """sweepplan.deal_by_degree in numpy: rows sorted by edge count (descending, stable), dealt boustrophedon over the groups;
    with `key` (merge_key) rows of equal edge count in ascending order of their mean key."""
    ptr = np.asarray(ptr, dtype=np.int64)
    n_rows = len(ptr) - 1
    n_groups = -(-n_rows // r)
    deg = ptr[1:] - ptr[:-1]
    if key is None or not len(key):
        by_degree = np.argsort(-deg, kind="stable")
    else:
        total = np.concatenate([[0], np.cumsum(np.asarray(key, dtype=np.int64))])
        mean = (total[ptr[1:]] - total[ptr[:-1]]).astype(np.float64) / np.maximum(deg, 1).astype(np.float64)
        by_mean = np.argsort(mean, kind="stable")
        by_degree = by_mean[np.argsort(-deg[by_mean], kind="stable")]
    at = np.arange(n_rows)
    rnd = at // max(n_groups, 1)
    j = at - rnd * n_groups
    group = np.where(rnd % 2 == 0, j, n_groups - 1 - j)
    a = np.full(n_groups * r, -1, dtype=np.int64)
    a[group * r + rnd] = by_degree
    return a.reshape(n_groups, r)


def transpose(rowptr, colind, n_cols):
    """The stable transpose (ptr, ind) of a CSR structure: inside every row of it the gathered rows ascend."""
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(colind, kind="stable")
    ptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(colind, minlength=n_cols), out=ptr[1:])
    return ptr, row[order]


def layout(ptr, ind, assign, forward=False):
    """-> (goff [n_groups + 1], gathered [nnz]): the gathered rows in the order the groups of `assign` walk them."""
    ptr, ind = np.asarray(ptr, dtype=np.int64), np.asarray(ind, dtype=np.int64)
    n_rows = len(ptr) - 1
    n_groups, r = assign.shape
    flat = assign.reshape(-1)
    real = np.nonzero(flat >= 0)[0]
    assert len(real) == n_rows and np.array_equal(np.sort(flat[real]), np.arange(n_rows)), "not a partition of the rows"
    group_of = np.empty(n_rows, dtype=np.int64)
    group_of[flat[real]] = real // r
    row = np.repeat(np.arange(n_rows), np.diff(ptr))
    group = group_of[row]
    stride = int(ind.max()) + 1 if len(ind) else 1
    key = merge_key(ptr, ind, forward)
    order = np.argsort(group * stride + key, kind="stable")
    goff = np.zeros(n_groups + 1, dtype=np.int64)
    np.cumsum(np.bincount(group, minlength=n_groups), out=goff[1:])
    return goff, ind[order]


def simulate(goff, gathered, n_waves=4096, capacities=CAPACITIES, xcds=8, waves_per_workgroup=4):
    """-> {"gathers", "ideal", capacity: hit rate, ...} of the lockstep model above."""
    n_groups = len(goff) - 1
    length = np.diff(goff)
    g = np.arange(n_groups)
    wave = g % n_waves
    # where a group's walk starts on its wave's clock: behind the wave's earlier rounds
    start = np.zeros(n_groups, dtype=np.int64)
    for first in range(n_waves, n_groups, n_waves):
        cur = slice(first, min(first + n_waves, n_groups))
        prev = slice(first - n_waves, first - n_waves + (cur.stop - cur.start))
        start[cur] = start[prev] + length[prev]
    group_of_edge = np.repeat(g, length)
    step = np.arange(len(gathered)) - goff[group_of_edge] + start[group_of_edge]
    wave_of_edge = wave[group_of_edge]
    xcd_of_edge = (wave_of_edge // waves_per_workgroup) % xcds
    total = len(gathered)
    distinct = len(np.unique(xcd_of_edge * (int(gathered.max()) + 1 if total else 1) + gathered))
    out = {"gathers": total, "ideal": 1.0 - distinct / total if total else 0.0}
    hits = dict.fromkeys(capacities, 0)
    for x in range(xcds):
        mine = np.nonzero(xcd_of_edge == x)[0]
        seq = gathered[mine[np.lexsort((wave_of_edge[mine], step[mine]))]].tolist()
        for cap in capacities:
            lru = collections.OrderedDict()
            n = 0
            for row in seq:
                if row in lru:
                    lru.move_to_end(row)
                    n += 1
                else:
                    lru[row] = None
                    if len(lru) > cap:
                        lru.popitem(last=False)
            hits[cap] += n
    for cap in capacities:
        out[cap] = hits[cap] / total if total else 0.0
    return out


def report(name, ptr, ind, assign, forward, n_waves):
    goff, gathered = layout(ptr, ind, assign, forward)
    edges = np.diff(goff)
    res = simulate(goff, gathered, n_waves)
    print("%-12s groups %d  edges per group %.1f (sd %.2f, min %d, max %d)  ideal %.3f  " % (
        name, len(edges), edges.mean(), edges.std(), edges.min(), edges.max(), res["ideal"])
        + "  ".join("%d rows %.3f" % (c, res[c]) for c in CAPACITIES), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=0, help="0: the benchmark's graph; else synth.scaled(nodes, degree, seed)")
    ap.add_argument("--degree", type=float, default=14.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--direction", choices=("backward", "forward"), default="backward")
    ap.add_argument("--rows", type=int, default=0, help="rows per group (0: as few as one round of --waves allows, at most 48)")
    ap.add_argument("--waves", type=int, default=4096, help="waves of one round (MI355X: 256 CUs x 16)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from cogdl_amd import synth

    g = synth.scaled(args.nodes, args.degree, seed=args.seed) if args.nodes else synth.arxiv_like(seed=0, topology="uniform")
    rowptr, colind = g.rowptr.numpy().astype(np.int64), g.colind.numpy().astype(np.int64)
    if args.direction == "backward":
        ptr, ind = transpose(rowptr, colind, g.n_cols)
    else:
        ptr, ind = rowptr, colind
    n_rows = len(ptr) - 1
    r = args.rows or max(1, min(48, -(-n_rows // args.waves)))
    print("%s: %d rows, %d edges, r = %d, %d waves a round" % (args.direction, n_rows, len(ind), r, args.waves))
    forward = args.direction == "forward"
    report("consecutive", ptr, ind, consecutive(n_rows, r), forward, args.waves)
    report("degree deal", ptr, ind, deal_by_degree(ptr, r), forward, args.waves)
    report("deal by key", ptr, ind, deal_by_degree(ptr, r, merge_key(ptr, ind, forward)), forward, args.waves)


if __name__ == "__main__":
    main()
