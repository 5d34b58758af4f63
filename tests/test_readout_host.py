"""The host twin of the batched graph readout (libcogdl_host.so, csrc/host_readout.cpp) through cogdl_amd.operators.readout on
CPU tensors: sum / mean bit for bit the reference's recorded CPU results and a sequential float32 loop, max / argmax numpy's
with first occurrence on ties, sort-pool the stable descending order, every backward against the plain torch composition,
segment_ptr's gaps and refusals.  No GPU."""
import numpy as np
import pytest
import torch

import _readout_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators import readout as R


@pytest.fixture(scope="module")
def gold(golden):
    return golden("readout")


@pytest.fixture(scope="module")
def cases():
    return C.grid()


def test_recorded_inputs_are_the_grids(gold):
    assert gold["lengths"].tolist() == C.LENGTHS and gold["sort_sizes"].tolist() == C.SORT_SIZES


@pytest.mark.parametrize("f", C.WIDTHS)
def test_sum_and_mean_equal_the_reference_bit_for_bit(gold, f):
    x, ptr = C.cols(torch.from_numpy(gold["pool_x"]), f), C.ptr_of(C.LENGTHS)
    got = R.segment_pool(x, ptr, "sum").numpy()
    assert got[:-1].tobytes() == gold["pool_sum_%d" % f].tobytes() and not got[-1].any()
    mean = R.segment_pool(x, ptr, "mean").numpy()
    filled = np.asarray(C.LENGTHS) > 0  # (the reference's mean has one row per graph id that occurs)
    assert mean[filled].tobytes() == gold["pool_mean_%d" % f].tobytes() and not mean[~filled].any()
    one = C.ptr_of([300])
    assert R.segment_pool(x[:300].contiguous(), one, "sum").numpy().tobytes() == gold["pool1_sum_%d" % f].tobytes()
    assert R.segment_pool(x[:300].contiguous(), one, "mean").numpy().tobytes() == gold["pool1_mean_%d" % f].tobytes()


@pytest.mark.parametrize("f", C.WIDTHS)
def test_sum_is_the_sequential_float32_loop(cases, f):
    lengths, ptr, x = cases
    x = C.cols(x, f)
    assert R.segment_pool(x, ptr, "sum").numpy().tobytes() == C.sequential_sum(x, ptr).tobytes()
    n = R.exact_nodes()
    xs = x.repeat((n + x.shape[0] - 1) // x.shape[0], 1)[:n].contiguous()  # one graph (B = 1) of exactly the bound
    assert R.segment_pool(xs, C.ptr_of([n]), "sum").numpy().tobytes() == C.sequential_sum(xs, C.ptr_of([n])).tobytes()


def test_above_the_exact_bound_the_sum_is_within_the_summation_bound_and_repeatable():
    n = R.exact_nodes() + 1
    assert n - 1 >= 4096
    lengths, ptr, x = C.grid(extra=n)
    for f in (7, 64, 130):
        xf = C.cols(x, f)
        got = R.segment_pool(xf, ptr, "sum").numpy()
        assert got.tobytes() == R.segment_pool(xf, ptr, "sum").numpy().tobytes()
        assert got[:-1].tobytes() == C.sequential_sum(xf[:-n], C.ptr_of(C.LENGTHS)).tobytes()
        seg = xf[-n:].double().numpy()
        bound = n * 2.0 ** -24 * np.abs(seg).sum(0)
        assert (np.abs(got[-1].astype(np.float64) - seg.sum(0)) <= bound).all()
        mean = R.segment_pool(xf, ptr, "mean").numpy()
        assert mean[-1].tobytes() == (got[-1] / np.float32(n)).tobytes()


@pytest.mark.parametrize("f", C.WIDTHS)
def test_max_and_argmax_equal_numpy(cases, f):
    lengths, ptr, x = cases
    x = C.cols(x, f)
    xg = x.clone().requires_grad_()   # (argmax is what the operator saves for its backward)
    out = R.segment_pool(xg, ptr, "max")
    argmax = out.grad_fn.saved_tensors[1].numpy()
    p = ptr.tolist()
    for g, n in enumerate(lengths):
        if n == 0:
            assert not out[g].detach().numpy().any() and (argmax[g] == -1).all()
            continue
        seg = x[p[g]:p[g + 1]].numpy()
        assert out[g].detach().numpy().tobytes() == seg.max(0).tobytes()
        assert (argmax[g] == seg.argmax(0) + p[g]).all()


def test_max_ties_go_to_the_smallest_row():
    lengths = [5, 0, 4200]
    x = torch.randn(sum(lengths), 9, generator=torch.Generator().manual_seed(3))
    x[1], x[3] = 50.0, 50.0                       # duplicates of the maximum inside one graph
    x[5 + 1500], x[5 + 1024], x[5 + 4199] = 60.0, 60.0, 60.0   # ... and across the chunks of a long segment
    xg = x.clone().requires_grad_()
    out = R.segment_pool(xg, C.ptr_of(lengths), "max")
    argmax = out.grad_fn.saved_tensors[1].numpy()
    assert (argmax[0] == 1).all() and (argmax[1] == -1).all() and (argmax[2] == 5 + 1024).all()
    assert (out[0] == 50).all() and (out[2] == 60).all()


def _sorted_rows(x):
    return torch.from_numpy(np.sort(x.numpy(), axis=-1))


@pytest.mark.parametrize("f", C.SORT_WIDTHS)
@pytest.mark.parametrize("k", C.SORT_K)
def test_sort_pool_equals_the_reference(gold, f, k):
    h = _sorted_rows(C.cols(torch.from_numpy(gold["sort_x"]), f))
    ptr = C.ptr_of(C.SORT_SIZES)
    out, idx = R.sort_pool(h, ptr, k)
    assert out.permute(0, 2, 1).contiguous().numpy().tobytes() == gold["sort_%d_%d" % (f, k)].tobytes()
    sizes = np.asarray(C.SORT_SIZES)[:, None]
    assert ((idx.numpy() == -1) == (np.arange(k)[None, :] >= sizes)).all()
    assert (idx.numpy() == C.stable_topk(h[:, -1].numpy(), ptr, k)).all()


def test_sort_pool_is_the_stable_descending_sort_on_planted_ties():
    lengths = [0, 40, 3, 2100, 1]               # (2100: above the kernels' in-LDS bound, the same law here)
    x = torch.randn(sum(lengths), 5, generator=torch.Generator().manual_seed(5))
    x[:, 2] = torch.randint(0, 7, (sum(lengths),)).float()   # seven distinct keys: ties everywhere
    x[10, 2], x[11, 2] = 0.0, -0.0                           # -0 equals +0
    ptr = C.ptr_of(lengths)
    for k in (1, 6, 64):
        out, idx = R.sort_pool(x, ptr, k, key_col=2)
        want = C.stable_topk(x[:, 2].numpy(), ptr, k)
        assert (idx.numpy() == want).all()
        assert torch.equal(out, C.gather_rows(x, want))


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_segment_pool_backward_equals_the_torch_composition(mode):
    n = R.exact_nodes() + 1
    lengths, ptr, x = C.grid(extra=n)
    for f in (7, 64):
        xf = C.cols(x, f)
        go = torch.randn(len(lengths), f, generator=torch.Generator().manual_seed(11))
        xg = xf.clone().requires_grad_()
        R.segment_pool(xg, ptr, mode).backward(go)
        x64 = xf.double().requires_grad_()
        C.torch_pool(x64, ptr, mode).backward(go.double())
        if mode == "sum":
            assert torch.equal(xg.grad, x64.grad.float())
        else:
            torch.testing.assert_close(xg.grad.double(), x64.grad, rtol=1e-6, atol=0)


def test_sort_pool_backward_is_an_exact_copy():
    ptr = C.ptr_of(C.SORT_SIZES)
    x = torch.randn(sum(C.SORT_SIZES), 33, generator=torch.Generator().manual_seed(13))
    for k in (5, 65):
        go = torch.randn(len(C.SORT_SIZES), k, 33, generator=torch.Generator().manual_seed(k))
        xg = x.clone().requires_grad_()
        out, idx = R.sort_pool(xg, ptr, k)
        out.backward(go)
        xr = x.clone().requires_grad_()
        C.gather_rows(xr, idx).backward(go)
        assert torch.equal(xg.grad, xr.grad)


def test_segment_ptr_gaps_give_empty_segments():
    batch = torch.tensor([1, 1, 4, 4, 4, 6])
    ptr, b = R.segment_ptr(batch)
    assert b == 7 and ptr.tolist() == [0, 0, 2, 2, 2, 5, 5, 6] and ptr.dtype == torch.int32
    ptr, b = R.segment_ptr(batch, num_graphs=9)
    assert b == 9 and ptr.tolist() == [0, 0, 2, 2, 2, 5, 5, 6, 6, 6]
    lengths, want, _ = C.grid()
    got, b = R.segment_ptr(torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths)), num_graphs=len(lengths))
    assert torch.equal(got, want)


def test_segment_ptr_refuses_unsorted_and_out_of_range_batches():
    with pytest.raises(_lib.BackendError):
        R.segment_ptr(torch.tensor([0, 2, 1, 2]))
    with pytest.raises(_lib.BackendError):
        R.segment_ptr(torch.tensor([0, 1, 5]), num_graphs=5)   # a value >= B
    with pytest.raises(_lib.BackendError):
        R.segment_ptr(torch.tensor([-1, 0, 1]))


def test_operators_refuse_what_they_do_not_cover():
    ptr = C.ptr_of([3])
    with pytest.raises(_lib.BackendError):
        R.segment_pool(torch.zeros(3, 4, dtype=torch.float64), ptr, "sum")
    with pytest.raises(_lib.BackendError):
        R.sort_pool(torch.zeros(3, 4, dtype=torch.float16), ptr, 2)
    with pytest.raises(_lib.BackendError):
        R.segment_pool(torch.zeros(3, 4), ptr.long(), "sum")
    with pytest.raises(ValueError):
        R.segment_pool(torch.zeros(3, 4), ptr, "median")
    assert _lib.host().cogdl_host_segment_pool_fwd(None, None, 1, 1, 2 ** 31, 0, None, None) == 2   # COGDL_HOST_ERANGE
    assert _lib.host().cogdl_host_sort_pool_fwd(None, None, 2 ** 31, 1, 4, 2, 0, None, None) == 2


def test_empty_inputs():
    ptr = C.ptr_of([0, 0])
    x = torch.zeros(0, 6)
    assert torch.equal(R.segment_pool(x, ptr, "mean"), torch.zeros(2, 6))
    out, idx = R.sort_pool(x, ptr, 3)
    assert torch.equal(out, torch.zeros(2, 3, 6)) and (idx == -1).all()
