"""Writes tests/golden/kg_sample.npz: the small knowledge graph of tests/_kgsample_cases.py (small_kg) with what the reference's
own TrainDataset (cogdl/datasets/kg_data.py:83-179) derives from its training triples: the true-head list of every
(relation, tail) and the true-tail list of every (head, relation), and the subsampling weight its __getitem__ returns for every
training triple in both modes.

Run in the build container only, where the reference package is checked out ($COGDL_REFERENCE, as for make_golden.py); the
package is imported from a scratch copy (it writes into its own tree when imported) with the stubs of tests/golden/_stubs.
CPU only.

Recorded: triples int16 [360, 3] with train_start / valid_start / test_start, num_entities, num_relations; per mode the keys
int16 [G, 2] in ascending order ((relation, tail) for head, (head, relation) for tail), list_ptr int32 [G + 1] and the ids of
every list in ascending order (the reference keeps them as arrays of a set: the order is not part of its contract);
weight_head / weight_tail float32 [300].  Only arrays are stored."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get("COGDL_REFERENCE", "/root/reference")
MAX_BYTES = 100_000


def main():
    scratch = tempfile.mkdtemp(prefix="cogdl_refcopy_")
    shutil.copytree(os.path.join(REFERENCE_ROOT, "cogdl"), os.path.join(scratch, "cogdl"))
    sys.dont_write_bytecode = True
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(HERE, "_stubs"), scratch]
    from cogdl.datasets.kg_data import TrainDataset

    import _kgsample_cases as C

    triples, train_start, valid_start, test_start, n, rels = C.small_kg()
    train = triples[train_start:valid_start]
    out = {"triples": np.array(triples, dtype=np.int16), "train_start": np.asarray(train_start), "valid_start": np.asarray(valid_start),
           "test_start": np.asarray(test_start), "num_entities": np.asarray(n), "num_relations": np.asarray(rels)}
    np.random.seed(0)
    for mode in C.MODES:
        side = mode.split("-")[0]
        ds = TrainDataset(train, n, rels, 4, mode)
        lists = ds.true_head if mode == "head-batch" else ds.true_tail
        keys = sorted(lists)
        ptr, ids = [0], []
        for key in keys:
            ids += sorted(int(v) for v in lists[key])
            ptr.append(len(ids))
        out["keys_" + side] = np.array(keys, dtype=np.int16)
        out["list_ptr_" + side] = np.array(ptr, dtype=np.int32)
        out["list_idx_" + side] = np.array(ids, dtype=np.int16)
        weights = []
        for i in range(len(ds)):
            positive, negative, weight, got_mode = ds[i]
            assert got_mode == mode and tuple(positive.tolist()) == tuple(train[i]) and weight.dtype.is_floating_point
            true = set(int(v) for v in lists[C.list_key(train[i], mode)])
            assert not true & set(negative.tolist())
            weights.append(weight.numpy())
        out["weight_" + side] = np.concatenate(weights).astype(np.float32)
        print(mode, len(keys), "groups, longest list", int(np.diff(ptr).max()))
    path = os.path.join(HERE, "kg_sample.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < MAX_BYTES, size
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
