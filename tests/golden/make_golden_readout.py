"""Writes tests/golden/readout.npz: node rows of small batches of graphs and what the reference's readout computes on them.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs.

Pooling.  Segment lengths LENGTHS (empty graphs first, last and inside; the wave-boundary lengths), one input
pool_x [624, 130] = randn * 100 (the cancellation makes a wrong association show in the last bits) whose leading F columns
serve F in WIDTHS; per F the CPU results of batch_sum_pooling and batch_mean_pooling (cogdl/utils/utils.py:192-203) as
pool_sum_F / pool_mean_F.  The mean is taken over the batch without its empty graphs (the reference returns one row per id
that occurs): its rows are those of the non-empty graphs, in order.  pool1_sum_F / pool1_mean_F: the first 300 rows as ONE
graph (B = 1).

Sort-pool.  Graph sizes SORT_SIZES, input sort_x [422, 33]; a reference SortPool with num_layers=0 and hidden_dim = F has no
GNN in front, and a forward pre-hook on its conv1d captures the pooled [B, F, k] tensor: sort_F_k.  torch's descending sort
promises no tie order, so the script asserts that the keys (the last channel after the row sort) are distinct inside every
graph."""
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "/root/reference")
LENGTHS = [0, 1, 2, 63, 64, 65, 129, 300, 0]
WIDTHS = (1, 7, 64, 65, 130)
SORT_SIZES = [1, 2, 29, 30, 31, 64, 65, 200]
SORT_K = (1, 5, 30, 65)
SORT_WIDTHS = (8, 33)
MAX_BYTES = 700_000


def main():
    import torch

    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.join(HERE, "_stubs"), scratch]
    from cogdl.models.nn.sortpool import SortPool
    from cogdl.utils.utils import batch_mean_pooling, batch_sum_pooling

    torch.manual_seed(20250)
    out = {"lengths": np.asarray(LENGTHS, dtype=np.int64), "sort_sizes": np.asarray(SORT_SIZES, dtype=np.int64)}
    x = torch.randn(sum(LENGTHS), max(WIDTHS)) * 100
    batch = torch.repeat_interleave(torch.arange(len(LENGTHS)), torch.tensor(LENGTHS))
    dense = torch.unique(batch, return_inverse=True)[1]  # the same rows without the empty graphs
    out["pool_x"] = x.numpy()
    for f in WIDTHS:
        xf = x[:, :f].contiguous()
        got = batch_sum_pooling(xf, batch)  # (max id + 1 rows: the trailing empty graph is not among them)
        assert got.shape == (len(LENGTHS) - 1, f)
        out["pool_sum_%d" % f] = got.numpy()
        out["pool_mean_%d" % f] = batch_mean_pooling(xf, dense).numpy()
        one = torch.zeros(300, dtype=torch.long)
        out["pool1_sum_%d" % f] = batch_sum_pooling(xf[:300].contiguous(), one).numpy()
        out["pool1_mean_%d" % f] = batch_mean_pooling(xf[:300].contiguous(), one).numpy()

    xs = torch.randn(sum(SORT_SIZES), max(SORT_WIDTHS)) * 100
    sbatch = torch.repeat_interleave(torch.arange(len(SORT_SIZES)), torch.tensor(SORT_SIZES))
    out["sort_x"] = xs.numpy()
    for f in SORT_WIDTHS:
        xf = xs[:, :f].contiguous()
        keys = xf.sort(dim=-1)[0][:, -1]
        for g in range(len(SORT_SIZES)):
            mine = keys[sbatch == g]
            assert torch.unique(mine).numel() == mine.numel(), "repeated keys in graph %d" % g
        for k in SORT_K:
            model = SortPool(f, f, 2, 0, 4, 1, k=k).eval()
            seen = []
            model.conv1d.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
            with torch.no_grad():
                model(types.SimpleNamespace(x=xf, batch=sbatch))
            assert len(seen) == 1 and seen[0].shape == (len(SORT_SIZES), f, k)
            out["sort_%d_%d" % (f, k)] = seen[0].numpy()
    path = os.path.join(HERE, "readout.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < MAX_BYTES, size
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
