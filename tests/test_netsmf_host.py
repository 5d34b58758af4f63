"""NetSMF without a GPU: the host twin (libcogdl_host.so) behind cogdl_amd.operators.netsmf, the torch composition of the
sparsifier, the randomized SVD on spmm_cpu and cogdl_amd.embedding.netsmf.  The GPU kernel returns the same pairs bit for bit
(tests/test_netsmf_gpu.py), so the law tests here cover both.  Cases and checks: tests/_netsmf_cases.py."""
import numpy as np
import pytest
import torch

import _netsmf_cases as cases
from cogdl_amd import _lib, embedding
from cogdl_amd.operators import netsmf as ns
from cogdl_amd.operators import path_counts, path_pairs, randomized_svd, sparsifier

# randomized_svd on the block-diagonal case, CPU path, against numpy.linalg.svd in float64 (recorded from this test's own
# print on the CPU): the largest relative deviation of S is 1.13e-7, the largest deviation of |<row_i, row_j>| from 0 / 1 is
# 7.1e-8.  The assertion, on the CPU and on the GPU, is ten times that: float32 rounding, other reduction orders on the device.
SVD_S_RECORDED, SVD_GRAM_RECORDED = 1.13e-7, 7.1e-8


def test_counts_follow_the_exact_expectation():
    cases.check_law("cpu")


def test_split_k_is_uniform():
    """k of 20,000 samples with r = 5 is uniform on 1 .. 5 within 6 sigma (the first draw, restated in Python; the
    restatement test below ties the restatement to the library)."""
    ks = np.asarray([cases.split_k(77, s, 5) for s in range(20_000)])
    counts = np.bincount(ks, minlength=6)
    assert counts[0] == 0 and counts.sum() == 20_000 and ks.max() == 5
    sigma = np.sqrt(20_000 * 0.2 * 0.8)
    print("k counts:", counts[1:], "sigma %.1f" % sigma)
    assert (np.abs(counts[1:] - 4000) <= 6 * sigma).all()


def test_python_restatement_equals_the_host_twin():
    indptr, indices, _ = cases.gd()
    row, col = path_pairs(indptr, indices, 10, 37, 200, seed=0x1234567890ABCDEF)
    assert row.dtype == torch.int32 and col.dtype == torch.int32 and row.numel() == 2000 and col.numel() == 2000
    want_row, want_col = cases.restated_pairs(indptr, indices, 10, 37, 200, 0x1234567890ABCDEF)
    assert np.array_equal(row.numpy(), want_row) and np.array_equal(col.numpy(), want_col)


def test_slices_window_one_and_empty():
    indptr, indices, n = cases.gd()
    e = indices.numel()
    full = path_pairs(indptr, indices, 10, 0, 2 * e + 37, seed=9)
    part = path_pairs(indptr, indices, 10, e + 5, 100, seed=9)
    for f, p in zip(full, part):
        assert torch.equal(p.view(10, 100), f.view(10, 2 * e + 37)[:, e + 5:e + 105])
    assert not torch.equal(full[0], path_pairs(indptr, indices, 10, 0, 2 * e + 37, seed=10)[0])
    row, col = path_pairs(indptr, indices, 1, 0, e, seed=9)  # no steps: the entry list itself
    assert torch.equal(row.long(), torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1]))
    assert torch.equal(col.long(), indices)
    row, col = path_pairs(indptr, indices, 10, 5, 0, seed=9)
    assert row.numel() == 0 and col.numel() == 0 and row.dtype == torch.int32


def test_counts_do_not_depend_on_the_batch():
    indptr, indices, n = cases.gd()
    want = path_counts(indptr, indices, 10, 2, seed=3)
    cases.assert_canonical(want[0], want[1], n)
    assert int(want[2].sum()) == 10 * 2 * indices.numel()
    for batch in (1000, 64):
        got = path_counts(indptr, indices, 10, 2, seed=3, batch=batch)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    again = path_counts(indptr, indices, 10, 2, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(again, want))
    empty = path_counts(indptr, indices, 10, 0, seed=3)
    assert empty[0].tolist() == [0] * (n + 1) and empty[1].numel() == 0 and empty[2].dtype == torch.int64


def test_invalid_graphs_raise():
    indptr, indices, n = cases.gd()
    bad = indices.clone()
    bad[17] = n
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        path_pairs(indptr, bad, 4, 0, indices.numel(), seed=0)
    bad[17] = -1
    with pytest.raises(_lib.BackendError, match="neighbour id"):
        path_counts(indptr, bad, 4, 1, seed=0)
    backwards = indptr.clone()
    backwards[40:60] = backwards[40:60].flip(0)
    assert bool((backwards[1:] < backwards[:-1]).any())
    with pytest.raises(_lib.BackendError, match="indptr"):
        path_pairs(backwards, indices, 4, 0, indices.numel(), seed=0)
    beyond = indptr.clone()
    beyond[-1] += 5
    with pytest.raises(_lib.BackendError, match="indptr"):
        path_pairs(beyond, indices, 4, 0, indices.numel(), seed=0)
    # the C entry point refuses bad sizes / pointers itself
    host = _lib.host().cogdl_host_netsmf_sample
    flags = torch.zeros(1, dtype=torch.int32)
    assert host(None, None, 4, 4, 0, 3, 5, 1, None, None, _lib.ptr(flags)) == 1
    assert host(None, None, 4, 0, 0, 3, 5, 1, None, None, None) == 1
    out = torch.zeros(8, dtype=torch.int32)
    args = (_lib.ptr(indptr), _lib.ptr(indices), n, indices.numel(), 0, 1)
    assert host(*args, 0, 1, _lib.ptr(out), _lib.ptr(out), _lib.ptr(flags)) == 1
    assert host(*args, 257, 1, _lib.ptr(out), _lib.ptr(out), _lib.ptr(flags)) == 1
    assert host(_lib.ptr(indptr), _lib.ptr(indices), 2 ** 31, indices.numel(), 0, 1, 4, 1, _lib.ptr(out), _lib.ptr(out),
                _lib.ptr(flags)) == 2
    assert host(_lib.ptr(indptr), _lib.ptr(indices), n, 0, 0, 1, 4, 1, _lib.ptr(out), _lib.ptr(out), _lib.ptr(flags)) == 1


def test_argument_errors_raise_before_anything_runs():
    indptr, indices, n = cases.gd()
    for window in (0, 257):
        with pytest.raises(ValueError):
            path_pairs(indptr, indices, window, 0, 4)
        with pytest.raises(ValueError):
            path_counts(indptr, indices, window, 1)
    with pytest.raises(ValueError):
        path_pairs(indptr, indices, 4, -1, 4)
    with pytest.raises(ValueError):
        path_pairs(indptr, indices, 4, 0, -4)
    with pytest.raises(ValueError):
        path_pairs(indptr[:3] * 0, indices[:0], 4, 0, 4)  # nothing to sample from
    with pytest.raises(ValueError):
        path_counts(indptr, indices, 4, -1)
    with pytest.raises(ValueError):
        path_counts(indptr, indices, 4, 1, batch=0)
    with pytest.raises(_lib.BackendError):
        path_pairs(indptr.int(), indices, 4, 0, 4)
    with pytest.raises(_lib.BackendError):
        path_pairs(indptr, indices.int(), 4, 0, 4)
    with pytest.raises(_lib.BackendError):
        path_pairs(indptr, indices.to("meta"), 4, 0, 4)  # mixed devices
    rowptr, col, count = path_counts(indptr, indices, 2, 1, seed=0)
    with pytest.raises(_lib.BackendError):
        sparsifier(indptr, rowptr.long(), col, count, 2, 1)
    with pytest.raises(_lib.BackendError):
        sparsifier(indptr, rowptr[:-1], col, count, 2, 1)
    with pytest.raises(_lib.BackendError):
        sparsifier(indptr, rowptr, col, count.float(), 2, 1)
    with pytest.raises(ValueError):
        sparsifier(indptr, rowptr, col, count, 2, 0)
    with pytest.raises(ValueError):
        sparsifier(indptr, rowptr, col, count, 2, 1, negative=0)
    m = sparsifier(indptr, rowptr, col, count, 2, 1)
    with pytest.raises(ValueError):
        randomized_svd(*m, n, 0)
    with pytest.raises(ValueError):
        randomized_svd(*m, n, n + 1)
    with pytest.raises(_lib.BackendError):
        randomized_svd(m[0], m[1], m[2].double(), n, 4)
    with pytest.raises(ValueError):
        embedding.netsmf((indptr, indices), dim=8, rounds=0)
    with pytest.raises(ValueError):
        embedding.netsmf((indptr, indices), dim=n + 1)


def test_sparsifier_reproduces_the_reference_transform():
    cases.check_sparsifier_reproduces_golden("cpu")


def test_own_estimate_agrees_with_the_reference_matrix():
    cases.check_own_estimate_agrees_with_golden("cpu")


def test_sparsifier_leaves_nodes_without_edges_empty():
    """A directed graph: the rows AND columns of nodes without out-neighbours are empty, every value is finite and > 0."""
    indptr, indices, n = cases.gd()
    rowptr, col, count = path_counts(indptr, indices, 4, 8, seed=1)
    m_rowptr, m_col, m_val = sparsifier(indptr, rowptr, col, count, 4, 8)
    cases.assert_canonical(m_rowptr, m_col, n)
    deg = (indptr[1:] - indptr[:-1])
    assert bool(((m_rowptr[1:] - m_rowptr[:-1])[deg == 0] == 0).all())
    assert bool((deg[m_col.long()] > 0).all()) and bool(torch.isfinite(m_val).all()) and bool((m_val > 0).all())
    assert m_val.numel() > 0


def test_randomized_svd_on_a_rank_five_matrix():
    dev_s, dev_gram = cases.svd_deviations("cpu")
    print("S: largest relative deviation %.3e; rows: largest deviation of |<row_i, row_j>| from 0 / 1 %.3e" % (dev_s, dev_gram))
    assert dev_s <= 10 * SVD_S_RECORDED and dev_gram <= 10 * SVD_GRAM_RECORDED


def test_randomized_svd_of_a_general_matrix_and_seeds():
    """A full-rank sparse matrix with a decaying spectrum: S against numpy's within 1e-4 relative; seeded runs are equal."""
    rng = np.random.default_rng(0)
    n = 90
    q1, q2 = np.linalg.qr(rng.normal(size=(n, n)))[0], np.linalg.qr(rng.normal(size=(n, n)))[0]
    dense = ((q1 * (0.7 ** np.arange(n))) @ q2.T).astype(np.float32)
    r, c = np.nonzero(dense)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    args = (torch.from_numpy(rowptr).int(), torch.from_numpy(c.astype(np.int32)), torch.from_numpy(dense[r, c]), n, 6)
    u, s = randomized_svd(*args, seed=1)
    exact_u, exact_s, _ = np.linalg.svd(dense.astype(np.float64))
    assert np.allclose(s.numpy(), exact_s[:6], rtol=1e-4)
    assert np.allclose(np.abs(u.numpy().T @ exact_u[:, :6]), np.eye(6), atol=1e-3)
    u2, s2 = randomized_svd(*args, seed=1)
    assert torch.equal(u, u2) and torch.equal(s, s2)
    zero = randomized_svd(torch.zeros(n + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0), n, 3, seed=1)
    assert not zero[0].any() and not zero[1].any()


def test_embedding_end_to_end_on_the_block_model():
    cases.check_end_to_end("cpu")


def test_embedding_gives_isolated_nodes_a_zero_row_and_is_seeded():
    indptr, indices, a = cases.g15()
    ip = torch.cat([indptr, indptr[-1:].repeat(2)])  # nodes 15 and 16 without edges
    emb = embedding.netsmf((ip, indices), dim=4, window=3, rounds=7, seed=2)
    assert tuple(emb.shape) == (17, 4) and not emb[15:].any()
    assert np.allclose(emb[:15].norm(dim=1).numpy(), 1.0, atol=1e-5)
    assert torch.equal(emb, embedding.netsmf((ip, indices), dim=4, window=3, rounds=8, seed=2))  # 7 rounds = 4 passes = 8 rounds
    torch.manual_seed(5)
    e1 = embedding.netsmf((ip, indices), dim=4, window=3, rounds=8)
    torch.manual_seed(5)
    assert torch.equal(e1, embedding.netsmf((ip, indices), dim=4, window=3, rounds=8))


def test_cpu_path_does_not_load_the_hip_library():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import _netsmf_cases as cases\n"
            "from cogdl_amd import _lib, embedding\n"
            "ip, ix, _ = cases.g15()\n"
            "embedding.netsmf((ip, ix), dim=4, window=3, rounds=4, seed=1)\n"
            "assert _lib._hip is None and _lib._host is not None\n"
            "assert not any('libcogdl_hip' in line for line in open('/proc/self/maps'))\n"
            "print('ok')\n" % (root, os.path.join(root, "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
