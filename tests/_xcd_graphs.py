"""The small graphs of the XCD-plan tests (tests/test_xcd_gpu.py, tests/test_halfprec_plan_gpu.py): the smallest that reach every
kind of virtual row and every merge path of a plan -- empty rows, short rows (whole), rows around SPLIT, hubs of several pieces per
owner, a row of ~80 parts (merged by a whole workgroup), rows whose edges all have ONE owner."""
import torch

from cogdl_amd import synth

KINDS = ["hubs", "one_owner", "short", "rect"]


def graph(kind):
    if kind == "hubs":  # hubs longer than several pieces, medium rows around SPLIT, empty rows
        g = synth.hub_csr(300, 257, base_deg=6, hubs=((3, 129), (4, 1000), (17, 5000), (18, 257), (40, 65), (41, 64), (100, 20000), (299, 700)),
                           seed=5)  # (row 100: ~80 parts -- merged by a whole workgroup)
    elif kind == "one_owner":  # every long row's edges name ONE column: a single owner XCD, seven absent parts
        g = synth.hub_csr(70, 50, base_deg=2, hubs=((0, 300), (5, 66), (69, 513)), seed=2)
        g.colind[g.rowptr[0]:g.rowptr[1]] = 7
        g.colind[g.rowptr[69]:g.rowptr[70]] = 49
    elif kind == "short":  # no long row at all: every slot whole, no records
        g = synth.random_csr(1000, 333, 8, seed=3)
    else:  # rectangular, more rows than columns, R-MAT-like skew
        g = synth.hub_csr(2000, 97, base_deg=30, hubs=((1, 4000), (2, 4001), (1999, 2047)), seed=7)
    return g


def square(g):
    """The same edges as a square operand (the fused GAT operator's graphs are square): empty rows appended."""
    if g.num_nodes == g.n_cols:
        return g
    n = max(g.num_nodes, g.n_cols)
    deg = torch.zeros(n, dtype=torch.long)
    deg[:g.num_nodes] = (g.rowptr[1:] - g.rowptr[:-1]).long()
    rp = torch.zeros(n + 1, dtype=torch.long)
    torch.cumsum(deg, 0, out=rp[1:])
    return synth.CSRGraph(rp.int(), g.colind, g.weight, n, n)
