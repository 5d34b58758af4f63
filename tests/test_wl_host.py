"""WL subtree relabelling on the host twin (csrc/host_wl.cpp, the law of csrc/wl_law.h), no GPU: the twin against an
independent Python oracle over rows of every length class, multi-edges, self-loops, both label dtypes and N = 0; what WL can
and cannot tell apart; flags for malformed input; the truncated-hash emulation."""
from collections import Counter

import numpy as np
import pytest
import torch

from cogdl_amd import _lib
from cogdl_amd.operators import wl_labels

from _wl_cases import GRID, cases, expected, isomorphic_pair_case


@pytest.mark.parametrize("name,rounds", GRID, ids=["%s-r%d" % c for c in GRID])
def test_host_twin_equals_the_oracle(name, rounds):
    indptr, indices, label0 = cases()[name]
    labels, classes = wl_labels(indptr, indices, label0, rounds)
    want_labels, want_classes = expected(name, rounds)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (rounds + 1, label0.numel())
    assert classes.dtype == torch.long and tuple(classes.shape) == (rounds + 1,)
    assert np.array_equal(labels.numpy(), want_labels) and np.array_equal(classes.numpy(), want_classes)


def test_isomorphic_graphs_in_one_batch_get_equal_label_multisets():
    indptr, indices, label0, n = isomorphic_pair_case()
    labels, classes = wl_labels(indptr, indices, label0, 3)
    for r in range(4):
        assert Counter(labels[r, :n].tolist()) == Counter(labels[r, n:].tolist())
    assert int(classes[3]) > int(classes[0])


def test_c6_and_two_c3_are_not_told_apart():
    indptr, indices, label0 = cases()["cycles"]
    labels, classes = wl_labels(indptr, indices, label0, 3)
    for r in range(4):
        assert Counter(labels[r, :6].tolist()) == Counter(labels[r, 6:].tolist())
    assert classes.tolist() == [1, 1, 1, 1]


def test_a_round_that_adds_no_class_leaves_classes_put():
    indptr, indices, label0 = cases()["stable"]
    labels, classes = wl_labels(indptr, indices, label0, 3)
    assert classes.tolist() == [2, 2, 2, 2] and labels.tolist() == [[0, 1, 0]] * 4


def test_malformed_input_raises_and_arguments_are_checked():
    indptr, indices, label0 = cases()["cycles"]
    back = indptr.clone()
    back[3] = back[2] - 1
    with pytest.raises(_lib.BackendError, match="indptr"):
        wl_labels(back, indices, label0, 1)
    short = indptr.clone()
    short[-1] -= 1
    with pytest.raises(_lib.BackendError, match="indptr"):
        wl_labels(short, indices, label0, 1)
    bad = indices.clone()
    bad[4] = 12
    with pytest.raises(_lib.BackendError, match="outside"):
        wl_labels(indptr, bad, label0, 1)
    star = torch.tensor([0, 32769] + [32769] * 32769, dtype=torch.int32)
    with pytest.raises(_lib.BackendError, match="row too long"):
        wl_labels(star, torch.arange(1, 32770, dtype=torch.int32), torch.zeros(32770, dtype=torch.long), 1)
    for args in ((indptr.long(), indices, label0, 1), (indptr, indices, label0.float(), 1), (indptr, indices, label0, -1),
                 (indptr, indices, label0[:-1], 1)):
        with pytest.raises(ValueError):
            wl_labels(*args)
    with pytest.raises(ValueError):
        wl_labels(indptr, indices, label0, 1, hash_bits=0)


def test_truncated_hash_emulation_raises_exactly_where_classes_would_merge():
    indptr, indices, label0 = cases()["many_classes"]
    full = wl_labels(indptr, indices, label0, 2)
    assert int(full[1].min()) > 16
    with pytest.raises(_lib.BackendError, match="collision"):  # more than 16 classes on 16 hash values: pigeonhole
        wl_labels(indptr, indices, label0, 2, hash_bits=4)
    wide = wl_labels(indptr, indices, label0, 2, hash_bits=100)
    assert torch.equal(wide[0], full[0]) and torch.equal(wide[1], full[1])
