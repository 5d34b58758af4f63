"""WL subtree relabelling on the GPU (csrc/wl.hip): labels and classes equal the host twin's bit for bit on every case of
_wl_cases.py (rows of every length class: the wave path, both workgroup paths and their thresholds); the degree cap;
malformed input raises instead of faulting; a truncated hash is caught by the verification, never a wrong label; two runs
give equal bytes."""
import numpy as np
import pytest
import torch

from cogdl_amd import _lib
from cogdl_amd.operators import wl_labels
from cogdl_amd.operators import wl as wl_mod

from _wl_cases import GRID, cases, expected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_gpu(name):
    return tuple(t.to(DEV) for t in cases()[name])


@pytest.mark.parametrize("name,rounds", GRID, ids=["%s-r%d" % c for c in GRID])
def test_labels_and_classes_equal_the_host_twin_bit_for_bit(name, rounds):
    host = wl_labels(*cases()[name], rounds)
    labels, classes = wl_labels(*on_gpu(name), rounds)
    assert labels.is_cuda and labels.dtype == torch.int32 and classes.is_cuda and classes.dtype == torch.long
    assert torch.equal(labels.cpu(), host[0]) and torch.equal(classes.cpu(), host[1])
    want_labels, want_classes = expected(name, rounds)  # and the oracle's
    assert np.array_equal(labels.cpu().numpy(), want_labels) and np.array_equal(classes.cpu().numpy(), want_classes)


def test_a_row_over_the_degree_cap_raises():
    assert _lib.hip().cogdl_hip_wl_max_degree() == wl_mod.MAX_DEGREE == 32768
    n = 32770
    indptr = torch.tensor([0, 32769] + [32769] * 32769, dtype=torch.int32, device=DEV)
    indices = torch.arange(1, n, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.BackendError, match="row too long"):
        wl_labels(indptr, indices, torch.zeros(n, dtype=torch.long, device=DEV), 1)
    # a row of exactly the cap is served
    indptr = torch.tensor([0, 32768] + [32768] * 32768, dtype=torch.int32)
    indices = torch.arange(1, 32769, dtype=torch.int32) % 7
    label0 = torch.arange(32769) % 5
    host = wl_labels(indptr, indices, label0, 1)
    gpu = wl_labels(indptr.to(DEV), indices.to(DEV), label0.to(DEV), 1)
    assert torch.equal(gpu[0].cpu(), host[0]) and torch.equal(gpu[1].cpu(), host[1])


def test_malformed_input_raises_and_the_device_is_fine_afterwards():
    indptr, indices, label0 = on_gpu("many_classes")
    back = indptr.clone()
    back[3] = back[2] - 1
    with pytest.raises(_lib.BackendError, match="indptr"):
        wl_labels(back, indices, label0, 2)
    bad = indices.clone()
    bad[4] = label0.numel()  # an index equal to N
    with pytest.raises(_lib.BackendError, match="outside"):
        wl_labels(indptr, bad, label0, 2)
    bad[4] = -1
    with pytest.raises(_lib.BackendError, match="outside"):
        wl_labels(indptr, bad, label0, 2)
    torch.cuda.synchronize()
    host = wl_labels(*cases()["many_classes"], 2)
    assert torch.equal(wl_labels(indptr, indices, label0, 2)[0].cpu(), host[0])


@pytest.mark.parametrize("name", ["many_classes", "cycles", "stable", "row_lengths"])
def test_a_truncated_hash_is_caught_never_a_wrong_label(name, monkeypatch):
    """hash_bits=4 leaves 16 hash values.  Whether two different signatures of a round share one is decided on the CPU, by
    the host twin's emulation of the truncation (the hash is the law's, csrc/wl_law.h): `many_classes` has more than 16
    classes in every round, so a collision is certain and the error branch is the one taken; `cycles` has one class, so the
    result must be the twin's."""
    monkeypatch.setattr(wl_mod, "SALT", 0x5eed)
    exact = wl_labels(*cases()[name], 2)
    try:
        wl_labels(*cases()[name], 2, hash_bits=4)
        collides = False
    except _lib.BackendError as e:
        assert "collision" in str(e)
        collides = True
    assert collides == {"many_classes": True, "cycles": False, "stable": collides, "row_lengths": collides}[name]
    if collides:
        with pytest.raises(_lib.BackendError, match="collision"):
            wl_labels(*on_gpu(name), 2, hash_bits=4)
    else:
        got = wl_labels(*on_gpu(name), 2, hash_bits=4)
        assert torch.equal(got[0].cpu(), exact[0]) and torch.equal(got[1].cpu(), exact[1])


def test_two_runs_give_equal_bytes():
    args = on_gpu("row_lengths")
    a, b = wl_labels(*args, 3), wl_labels(*args, 3)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and torch.equal(a[1], b[1])
