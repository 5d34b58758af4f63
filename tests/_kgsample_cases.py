"""Shared cases of the knowledge-graph training-batch tests (tests/test_kgsample_host.py, tests/test_kgsample_gpu.py,
tests/test_kgsample_install_cpu.py, tests/golden/make_golden_kgsample.py).

    law_row(a, n, seed, mode, sid, k)      the law of csrc/kgsample_law.h restated in numpy on oracle.philox4x32_10 and Python's
                                           exact integers: the k negatives of positive `sid` whose sorted true list is `a`
    sweep_kg(mode) / CASES / make(name)    a graph with one group per list length around the kernel's LDS threshold, and the
                                           batches cut from it
    true_lists(triples, mode)              the reference's get_true_head_and_tail as Python sets
    frequency(triples)                     the reference's count_frequency as a Python dict
    small_kg()                             the fixture's graph (tests/golden/kg_sample.npz)
"""
import os

import numpy as np
import torch

from cogdl_amd.operators import kgsample as KS
from oracle.oracle import philox4x32_10

MODES = ("head-batch", "tail-batch")
TAGS = {"head-batch": 0x4B474E48, "tail-batch": 0x4B474E54}
THRESHOLD = KS.LDS_LIST
N = THRESHOLD + 37
LENGTHS = (1, 2, 63, 64, 65, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1, N - 1)
SEED = 0x1234_5678_9ABC_DEF1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kg_sample.npz")


def law_words(seed, mode, sids, k):
    """[len(sids), k] Python-int words: the 64-bit draw of every (sid, j)."""
    sids = [int(s) % 2 ** 64 for s in sids]
    pairs = (k + 1) // 2
    ctr = np.zeros((len(sids), pairs, 4), dtype=np.uint32)
    ctr[:, :, 0] = np.arange(pairs, dtype=np.uint32)[None, :]
    ctr[:, :, 1] = np.array([s & 0xFFFFFFFF for s in sids], dtype=np.uint32)[:, None]
    ctr[:, :, 2] = np.array([s >> 32 for s in sids], dtype=np.uint32)[:, None]
    ctr[:, :, 3] = TAGS[mode]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    out = philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:2] + (2,))).astype(object)
    words = np.empty((len(sids), 2 * pairs), dtype=object)
    words[:, 0::2] = out[:, :, 0] * 2 ** 32 + out[:, :, 1]
    words[:, 1::2] = out[:, :, 2] * 2 ** 32 + out[:, :, 3]
    return words[:, :k]


def law_from_words(words, a, n):
    """One row: words [k] -> negatives int64 [k] for the sorted, distinct true list a over n entities."""
    a = np.asarray(a, dtype=np.int64)
    m = n - len(a)
    assert m > 0
    r = np.array([(int(w) * m) >> 64 for w in words], dtype=np.int64)
    gaps = a - np.arange(len(a), dtype=np.int64)
    assert np.all(np.diff(gaps) >= 0)
    return r + np.searchsorted(gaps, r, side="right")


def law_row(a, n, seed, mode, sid, k):
    return law_from_words(law_words(seed, mode, [sid], k)[0], a, n)


def true_lists(triples, mode):
    """{(relation, tail): set of heads} for head-batch, {(head, relation): set of tails} for tail-batch
    (TrainDataset.get_true_head_and_tail, cogdl/datasets/kg_data.py:156-179)."""
    out = {}
    for h, r, t in triples:
        if mode == "head-batch":
            out.setdefault((r, t), set()).add(h)
        else:
            out.setdefault((h, r), set()).add(t)
    return out


def list_key(triple, mode):
    h, r, t = triple
    return (r, t) if mode == "head-batch" else (h, r)


def frequency(triples, start=4):
    """TrainDataset.count_frequency (kg_data.py:137-154)."""
    count = {}
    for h, r, t in triples:
        for key in ((h, r), (t, -r - 1)):
            count[key] = count[key] + 1 if key in count else start
    return count


def reference_weight(count, triple):
    h, r, t = triple
    return torch.sqrt(1 / torch.Tensor([count[(h, r)] + count[(t, -r - 1)]]))


_SWEEP = {}


def sweep_kg(mode):
    """-> (triples list of (h, r, t), first: {L: the id of the first triple whose `mode` list has L ids}).  Relation i's group
    has LENGTHS[i] ids, drawn without replacement from [0, N); the group of length 64 holds 0 and N - 1."""
    if mode not in _SWEEP:
        rng = np.random.RandomState(77 + MODES.index(mode))
        triples, first = [], {}
        for i, length in enumerate(LENGTHS):
            ids = np.sort(rng.choice(N, size=length, replace=False))
            if length == 64:
                ids[0], ids[-1] = 0, N - 1
                assert len(set(ids.tolist())) == 64
            first[length] = len(triples)
            fixed = int(rng.randint(N))
            for e in ids.tolist():
                triples.append((e, i, fixed) if mode == "head-batch" else (fixed, i, e))
        _SWEEP[mode] = (triples, first)
    return _SWEEP[mode]


#          name            mode          B     K    first_sid    index dtype   lists the first rows name
CASES = {
    "k1":                ("tail-batch", 1027, 1, 0, torch.int64, LENGTHS),
    "k2":                ("head-batch", 1027, 2, 0, torch.int64, LENGTHS),
    "k63":               ("tail-batch", 1027, 63, 0, torch.int32, LENGTHS),
    "k64":               ("head-batch", 1027, 64, 0, torch.int64, LENGTHS),
    "k65_sid_hi":        ("tail-batch", 1027, 65, 2 ** 32 - 3, torch.int64, LENGTHS),
    "k128":              ("head-batch", 1027, 128, 0, torch.int32, LENGTHS),
    "k257":              ("tail-batch", 1027, 257, 0, torch.int64, LENGTHS),
    "b1_long":           ("head-batch", 1, 65, 0, torch.int64, (THRESHOLD + 1,)),
    "b1_one_free":       ("tail-batch", 1, 128, 2 ** 32 - 3, torch.int32, (N - 1,)),
    "b5_sid_hi":         ("head-batch", 5, 65, 2 ** 32 - 3, torch.int64, (1, 64, THRESHOLD, THRESHOLD + 1, N - 1)),
    "b5_i32":            ("tail-batch", 5, 63, 0, torch.int32, (THRESHOLD - 1, THRESHOLD, THRESHOLD + 1, 2, 65)),
}


def make(name):
    """-> dict(mode, triples, order int32 [B], K, first_sid, index_dtype): the first rows name one triple of each listed
    length, the rest are drawn over all triples."""
    mode, b, k, first_sid, dtype, lengths = CASES[name]
    triples, first = sweep_kg(mode)
    rng = np.random.RandomState(sum(map(ord, name)))
    order = rng.randint(len(triples), size=b).astype(np.int32)
    for i, length in enumerate(lengths[:b]):
        order[i] = first[length] + rng.randint(length)
    return dict(mode=mode, triples=triples, order=order, K=k, first_sid=first_sid, index_dtype=dtype)


_RESTATED = {}


def restated(name):
    """(positive int64 [B, 3], negative int64 [B, K], weight float32 [B]) of a case from the numpy restatement, Python sets and
    the Python frequency dict: nothing of the library is involved."""
    if name not in _RESTATED:
        c = make(name)
        triples, mode, order = c["triples"], c["mode"], c["order"]
        lists = {key: np.array(sorted(v), dtype=np.int64) for key, v in true_lists(triples, mode).items()}
        count = frequency(triples)
        words = law_words(SEED, mode, [c["first_sid"] + b for b in range(len(order))], c["K"])
        neg = np.stack([law_from_words(words[b], lists[list_key(triples[t], mode)], N) for b, t in enumerate(order)])
        pos = np.array([triples[t] for t in order], dtype=np.int64).reshape(len(order), 3)
        weight = torch.cat([reference_weight(count, triples[t]) for t in order]).numpy()
        _RESTATED[name] = (pos, neg.reshape(len(order), c["K"]), weight)
    return _RESTATED[name]


def small_kg():
    """The fixture's graph: 40 entities, 5 relations, 300 training triples followed by 30 validation and 30 test triples.
    (relation 0, tail 7) is a hub with 30 distinct heads; triples of multiplicity 2 and 3 are present.
    -> (triples list of (h, r, t), train_start, valid_start, test_start, num_entities, num_relations)"""
    rng = np.random.RandomState(20266)
    n, rels = 40, 5
    train = [(int(h), 0, 7) for h in rng.choice(n, size=30, replace=False)]
    while len(train) < 291:
        train.append((int(rng.randint(n)), int(rng.randint(rels)), int(rng.randint(n))))
    train += [train[40]] + [train[50]] * 2 + [train[0]] + [train[60]] * 2 + [train[70]] * 2 + [train[80]]
    assert len(train) == 300
    order = rng.permutation(300)
    train = [train[i] for i in order]
    rest = [(int(rng.randint(n)), int(rng.randint(rels)), int(rng.randint(n))) for _ in range(60)]
    return train + rest, 0, 300, 330, n, rels
