#!/usr/bin/env python3
"""The forward launch of the headline alone (arxiv-shaped uniform graph, fp32, F = 128, weighted): the ordinary launch against
the guarded pair of the forward sweep (operators/spmm.py: csr_spmm_sweep_forward_raw), HIP events around every launch, 20 warm-up
launches, then 3 blocks of 100 launches per variant, alternating.  Variants:
  ordinary   csr_spmm_raw (what a forward call without a candidate launches)
  match      the pair with the layout's own hash: the sweep runs, the ordinary launch stands down
  mismatch   the pair with another hash: the sweep stands down, the ordinary launch runs -- the price of a wrong guess
  sweep      the unguarded sweep kernel over the same layout (what the two guards cost on top of it)
--sorted-loops: the same graph with every row's columns sorted (the self loop moved into sorted position: no out-of-order edge) --
a probe of what the out-of-order edges cost, never a default.  On a tree without the forward sweep only `ordinary` is timed.
Usage: python tools/exp/sweep_forward_ab.py [--sorted-loops] [--topology uniform|rmat]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from cogdl_amd import _lib, plan, sweepplan, synth  # noqa: E402
from cogdl_amd.operators import spmm as S  # noqa: E402

DEV = "cuda:0"
F = 128


def timed(fn, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        out.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sorted-loops", action="store_true")
    ap.add_argument("--topology", default="uniform")
    args = ap.parse_args()
    g = synth.arxiv_like(seed=0, topology=args.topology)
    rowptr, colind, w = g.rowptr, g.colind, g.weight
    if args.sorted_loops:
        row = torch.repeat_interleave(torch.arange(g.num_nodes), g.degrees())
        order = torch.sort(row * g.num_nodes + colind.long(), stable=True).indices
        colind, w = colind[order].contiguous(), w[order].contiguous()
    rowptr, colind, w = rowptr.to(DEV), colind.to(DEV), w.to(DEV)
    x = torch.randn(g.num_nodes, F, generator=torch.Generator().manual_seed(0)).to(DEV)
    variants = {"ordinary": lambda: S.csr_spmm_raw(rowptr, colind, w, x)}
    want = variants["ordinary"]()
    head = "n=%d nnz=%d sorted_loops=%s" % (g.num_nodes, g.nnz, args.sorted_loops)
    if hasattr(S, "csr_spmm_sweep_forward_raw"):
        lib = _lib.hip()
        r = sweepplan.group_rows(g.num_nodes, sweepplan.round_rows(F, torch.float32), lib.cogdl_hip_csr_spmm_sweep_group_rows())
        sp = sweepplan.build_forward(rowptr, colind, g.num_nodes, r)
        fp = plan.Fingerprint(rowptr, colind, g.num_nodes, dev_parts=True)
        sp.hash = fp.key()[4] & ((1 << 64) - 1)
        other = sweepplan.SweepPlan(sp.goff, sp.src, sp.eid, sp.r, sp.n_rows, sp.n_src, sp.out_of_order, sp.long_rows)
        other.hash = sp.hash ^ 1
        w_p = sp.permuted_values(w)
        other.permuted_values(w)
        out_sweep = torch.empty_like(want)

        def sweep():
            rc = lib.cogdl_hip_csr_spmm_sweep(_lib.ptr(sp.goff), _lib.ptr(sp.src), _lib.ptr(w_p), _lib.ptr(x), _lib.ptr(out_sweep),
                                              g.num_nodes, g.num_nodes, sp.n_groups, sp.r, F, sp.nnz, 0, _lib.stream_of(x))
            _lib.check(rc, "csr_spmm_sweep")
            return out_sweep

        variants["match"] = lambda: S.csr_spmm_sweep_forward_raw(sp, fp.dev, rowptr, colind, w, x)
        variants["mismatch"] = lambda: S.csr_spmm_sweep_forward_raw(other, fp.dev, rowptr, colind, w, x)
        variants["sweep"] = sweep
        same = all(torch.equal(fn(), want) for fn in variants.values())
        head += " r=%d groups=%d out_of_order=%.4f long_rows=%s bit-identical=%s" % (sp.r, sp.n_groups, sp.out_of_order, sp.long_rows, same)
    print(head)
    for fn in variants.values():
        timed(fn, 20)
    for _ in range(3):
        line = []
        for name, fn in variants.items():
            t = timed(fn, 100)
            line.append("%s med %.1f us (min %.1f max %.1f)" % (name, statistics.median(t), min(t), max(t)))
        print("    " + "   ".join(line))


if __name__ == "__main__":
    main()
