#!/usr/bin/env python3
"""The sweep launches alone, for an A/B of the walk (csrc/rowsweep.h: sweep_walk) between two builds: HIP events around every
launch, 20 warm-up launches, then 3 blocks of 100 launches per variant, alternating (the protocol of
tools/exp/sweep_forward_ab.py).  fp32, F = 128, weighted.  On the arxiv-shaped uniform graph:
  backward   csr_spmm_sweep_raw over the transpose's layout (what the backward of a structure seen before launches)
  match      the guarded pair of the forward with the layout's own hash: the sweep runs, the ordinary launch stands down
  mismatch   the pair with another hash: the sweep stands down, the ordinary launch runs
  sweep      the unguarded sweep kernel over the forward layout
and `backward` alone on the 85k-node and 70k-node graphs of profiles/sweep_backward.txt section 1.
--tree DIR imports cogdl_amd from DIR (a built export of another commit) instead of this tree; run once per build, alternating.
Usage: python tools/exp/sweep_pipeline_ab.py [--tree DIR]"""
import argparse
import os
import statistics
import sys

import torch

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


def blocks(variants):
    for fn in variants.values():
        timed(fn, 20)
    for _ in range(3):
        line = []
        for name, fn in variants.items():
            t = timed(fn, 100)
            line.append("%s med %.1f us (min %.1f max %.1f)" % (name, statistics.median(t), min(t), max(t)))
        print("    " + "   ".join(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from cogdl_amd import _lib, plan, sweepplan, synth
    from cogdl_amd.operators import spmm as S

    lib = _lib.hip()
    R = lib.cogdl_hip_csr_spmm_sweep_group_rows()

    def backward_of(g):
        rowptr, colind, w = g.rowptr.to(DEV), g.colind.to(DEV), g.weight.to(DEV)
        gout = torch.randn(g.num_nodes, F, generator=torch.Generator().manual_seed(1)).to(DEV)
        csc = plan.csr2csc(rowptr, colind, g.n_cols)
        want = S.csr_spmm_raw(csc.colptr, csc.rowind, csc.transposed_values(w), gout, split_long_rows=csc.has_hub_columns())
        same = torch.equal(S.csr_spmm_sweep_raw(csc, w, gout), want)
        sp = csc.sweep
        print("n=%d nnz=%d r=%d groups=%d bit-identical=%s" % (g.num_nodes, g.nnz, sp.r, sp.n_groups, same))
        return lambda: S.csr_spmm_sweep_raw(csc, w, gout)

    print("arxiv uniform")
    g = synth.arxiv_like(seed=0, topology="uniform")
    variants = {"backward": backward_of(g)}
    rowptr, colind, w = g.rowptr.to(DEV), g.colind.to(DEV), g.weight.to(DEV)
    x = torch.randn(g.num_nodes, F, generator=torch.Generator().manual_seed(0)).to(DEV)
    want = S.csr_spmm_raw(rowptr, colind, w, x)
    r = sweepplan.group_rows(g.num_nodes, sweepplan.round_rows(F, torch.float32), R)
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
    print("forward: r=%d groups=%d out_of_order=%.4f bit-identical=%s"
          % (sp.r, sp.n_groups, sp.out_of_order, all(torch.equal(variants[k](), want) for k in ("match", "mismatch", "sweep"))))
    blocks(variants)
    for name, graph in (("85k nodes uniform", synth.scaled(84672, 13.8, seed=0)), ("70k nodes uniform deg 8", synth.scaled(70000, 8, seed=4))):
        print(name)
        blocks({"backward": backward_of(graph)})


if __name__ == "__main__":
    main()
