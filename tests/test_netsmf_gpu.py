"""NetSMF on the GPU: the HIP kernel (csrc/netsmf.hip) returns the host twin's pairs bit for bit, path_counts is the same
matrix on both devices and for every batch, and the checks of tests/test_netsmf_host.py (law, golden, randomized SVD, end to
end) hold on the device path (coalesce, csr2csc, csrspmm).  Cases and checks: tests/_netsmf_cases.py."""
import pytest
import torch

import _netsmf_cases as cases
from cogdl_amd import _lib
from cogdl_amd.operators import path_counts, path_pairs
from test_netsmf_host import SVD_GRAM_RECORDED, SVD_S_RECORDED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gd_dev():
    indptr, indices, n = cases.gd()
    return indptr.to(DEV), indices.to(DEV), n


@pytest.fixture(scope="module")
def full_pairs(gd_dev):
    """(GPU pairs, host pairs) of GD, T = 10, samples 0 .. 2 E + 36: computed once, read by several tests."""
    indptr, indices, _ = cases.gd()
    count = 2 * indices.numel() + 37
    return path_pairs(gd_dev[0], gd_dev[1], 10, 0, count, seed=9), path_pairs(indptr, indices, 10, 0, count, seed=9), count


def test_pairs_equal_the_host_twin(full_pairs):
    gpu, host, count = full_pairs
    for g, h in zip(gpu, host):
        assert g.is_cuda and g.dtype == torch.int32 and g.numel() == 10 * count
        assert torch.equal(g.cpu(), h)


def test_a_slice_equals_the_same_positions_of_the_full_call(gd_dev, full_pairs):
    gpu, _, count = full_pairs
    e = gd_dev[1].numel()
    part = path_pairs(gd_dev[0], gd_dev[1], 10, e + 5, 100, seed=9)
    for f, p in zip(gpu, part):
        assert torch.equal(p.view(10, 100), f.view(10, count)[:, e + 5:e + 105])


def test_window_one_is_the_entry_list_and_count_zero_is_empty(gd_dev):
    indptr, indices, n = gd_dev
    row, col = path_pairs(indptr, indices, 1, 0, indices.numel(), seed=9)
    assert torch.equal(row.long(), torch.repeat_interleave(torch.arange(n, device=DEV), indptr[1:] - indptr[:-1]))
    assert torch.equal(col.long(), indices)
    row, col = path_pairs(indptr, indices, 10, 5, 0, seed=9)
    assert row.numel() == 0 and col.numel() == 0 and row.is_cuda and row.dtype == torch.int32


def test_counts_equal_the_cpu_result_for_every_batch(gd_dev):
    indptr, indices, n = cases.gd()
    want = path_counts(indptr, indices, 10, 2, seed=3)
    for batch in (None, 1000, 64):
        got = path_counts(gd_dev[0], gd_dev[1], 10, 2, seed=3, batch=batch)
        assert got[0].is_cuda and got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.int64
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want)), "batch %r" % batch


def test_a_bad_neighbour_id_raises_on_the_device_too(gd_dev):
    indptr, indices, n = gd_dev
    bad = indices.clone()
    bad[17] = n
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        path_pairs(indptr, bad, 4, 0, indices.numel(), seed=0)


def test_counts_follow_the_exact_expectation():
    cases.check_law(DEV)


def test_sparsifier_reproduces_the_reference_transform():
    cases.check_sparsifier_reproduces_golden(DEV)


def test_own_estimate_agrees_with_the_reference_matrix():
    cases.check_own_estimate_agrees_with_golden(DEV)


def test_randomized_svd_on_a_rank_five_matrix():
    dev_s, dev_gram = cases.svd_deviations(DEV)
    print("S: largest relative deviation %.3e; rows: largest deviation of |<row_i, row_j>| from 0 / 1 %.3e" % (dev_s, dev_gram))
    assert dev_s <= 10 * SVD_S_RECORDED and dev_gram <= 10 * SVD_GRAM_RECORDED


def test_embedding_end_to_end_on_the_block_model():
    cases.check_end_to_end(DEV)
