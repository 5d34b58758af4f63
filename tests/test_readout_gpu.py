"""The readout kernels (csrc/readout.hip) against their host twin, bit for bit: every mode, forward and backward, the grid
with an over-bound segment, B = 1, the slow sort path; the reference's recorded sums; repeatability; a side stream; graph
capture; the row clamp (last in the file)."""
import pytest
import torch

import _readout_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators import readout as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pool_all(x, ptr, mode, go):
    xg = x.clone().requires_grad_()
    out = R.segment_pool(xg, ptr, mode)
    out.backward(go)
    return out.detach(), xg.grad


def _sort_all(x, ptr, k, go, key_col=-1):
    xg = x.clone().requires_grad_()
    out, idx = R.sort_pool(xg, ptr, k, key_col)
    out.backward(go)
    return out.detach(), idx, xg.grad


def _same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def over():
    return C.grid(extra=R.exact_nodes() + 1)


@pytest.mark.parametrize("f", C.WIDTHS)
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_segment_pool_equals_the_host_twin(over, mode, f):
    lengths, ptr, x = over
    x = C.cols(x, f)
    go = torch.randn(len(lengths), f, generator=torch.Generator().manual_seed(1))
    want = _pool_all(x, ptr, mode, go)
    got = _pool_all(x.to(DEV), ptr.to(DEV), mode, go.to(DEV))
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    again = _pool_all(x.to(DEV), ptr.to(DEV), mode, go.to(DEV))
    assert _same(again[0], got[0]) and _same(again[1], got[1])
    one = C.ptr_of([x.shape[0]])  # B = 1: the whole grid as one (long) graph
    want = _pool_all(x, one, mode, go[:1])
    got = _pool_all(x.to(DEV), one.to(DEV), mode, go[:1].to(DEV))
    assert _same(got[0], want[0]) and _same(got[1], want[1])


@pytest.mark.parametrize("f", C.WIDTHS)
def test_sum_and_mean_equal_the_reference_bit_for_bit(golden, f):
    gold = golden("readout")
    x, ptr = C.cols(torch.from_numpy(gold["pool_x"]), f).to(DEV), C.ptr_of(C.LENGTHS).to(DEV)
    filled = torch.tensor(C.LENGTHS) > 0
    assert R.segment_pool(x, ptr, "sum").cpu().numpy()[:-1].tobytes() == gold["pool_sum_%d" % f].tobytes()
    assert R.segment_pool(x, ptr, "mean").cpu()[filled].numpy().tobytes() == gold["pool_mean_%d" % f].tobytes()
    one = C.ptr_of([300]).to(DEV)
    assert R.segment_pool(x[:300].contiguous(), one, "sum").cpu().numpy().tobytes() == gold["pool1_sum_%d" % f].tobytes()
    assert R.segment_pool(x[:300].contiguous(), one, "mean").cpu().numpy().tobytes() == gold["pool1_mean_%d" % f].tobytes()


@pytest.mark.parametrize("f", C.SORT_WIDTHS)
def test_sort_pool_equals_the_host_twin(f):
    lds = _lib.hip().cogdl_hip_sort_pool_lds_nodes()
    sizes = [0] + C.SORT_SIZES + [lds + 1, lds]  # the slow path, and the largest graph of the LDS path
    ptr = C.ptr_of(sizes)
    x = torch.randn(sum(sizes), f, generator=torch.Generator().manual_seed(2)) * 100
    x[:, 0] = torch.randint(0, 9, (sum(sizes),)).float()  # a key column full of ties
    for k, key_col in ((1, -1), (5, 0), (30, -1), (65, 0)):
        go = torch.randn(len(sizes), k, f, generator=torch.Generator().manual_seed(k))
        want = _sort_all(x, ptr, k, go, key_col)
        got = _sort_all(x.to(DEV), ptr.to(DEV), k, go.to(DEV), key_col)
        assert all(_same(a, b) for a, b in zip(got, want)), (k, key_col)
        again = _sort_all(x.to(DEV), ptr.to(DEV), k, go.to(DEV), key_col)
        assert all(_same(a, b) for a, b in zip(again, got))


def test_segment_ptr_equals_the_host_twin():
    lengths, want, _ = C.grid()
    batch = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))
    got, b = R.segment_ptr(batch.to(DEV))
    assert b == len(lengths) - 1 and torch.equal(got.cpu(), want[:-1])
    got, b = R.segment_ptr(batch.to(DEV), num_graphs=len(lengths))
    assert torch.equal(got.cpu(), want)
    with pytest.raises(_lib.BackendError):
        R.segment_ptr(torch.tensor([0, 2, 1, 2], device=DEV))
    with pytest.raises(_lib.BackendError):
        R.segment_ptr(torch.tensor([0, 1, 5], device=DEV), num_graphs=5)


def test_operators_run_on_a_side_stream(over):
    lengths, ptr, x = over
    x, go = C.cols(x, 65), torch.randn(len(lengths), 65, generator=torch.Generator().manual_seed(1))
    gs = torch.randn(len(lengths), 5, 65, generator=torch.Generator().manual_seed(4))
    want, want_s = _pool_all(x, ptr, "mean", go), _sort_all(x, ptr, 5, gs)
    xd, pd, god, gsd = x.to(DEV), ptr.to(DEV), go.to(DEV), gs.to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, got_s = _pool_all(xd, pd, "mean", god), _sort_all(xd, pd, 5, gsd)
    side.synchronize()
    assert all(_same(a, b) for a, b in zip(got + got_s, want + want_s))


def test_captured_forward_and_backward_replay_to_the_same_bytes(over):
    lengths, ptr, x = over
    f, k = 64, 30
    xd = C.cols(x, f).to(DEV).requires_grad_()
    pd = ptr.to(DEV)
    go = torch.randn(len(lengths), f, generator=torch.Generator().manual_seed(1)).to(DEV)
    gs = torch.randn(len(lengths), k, f, generator=torch.Generator().manual_seed(4)).to(DEV)

    def step():
        out = R.segment_pool(xd, pd, "sum")
        top, idx = R.sort_pool(xd, pd, k)
        (gx,) = torch.autograd.grad([out, top], [xd], [go, gs])
        return out.detach(), top.detach(), idx, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        want = [t.clone() for t in step()]  # (warm-up outside the capture: libraries and workspaces load here)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(got, want))


def test_mixed_devices_raise():
    x, ptr = torch.zeros(4, 8), C.ptr_of([4])
    with pytest.raises(_lib.BackendError):
        R.segment_pool(x.to(DEV), ptr, "sum")
    with pytest.raises(_lib.BackendError):
        R.sort_pool(x, ptr.to(DEV), 2)


def test_a_ptr_past_the_last_row_is_clamped():
    """Rows are clamped into [0, N]: a ptr that runs past x gives wrong numbers, not an access outside x (kept last)."""
    x = torch.randn(100, 64, device=DEV).requires_grad_()
    ptr = torch.tensor([0, 40, 250], dtype=torch.int32, device=DEV)
    out = R.segment_pool(x, ptr, "sum")
    top, idx = R.sort_pool(x, ptr, 70)
    torch.autograd.grad([out, top], [x], [torch.ones_like(out), torch.ones_like(top)])
    torch.cuda.synchronize()
    assert torch.equal(out[1], R.segment_pool(x.detach(), torch.tensor([0, 40, 100], dtype=torch.int32, device=DEV), "sum")[1])
    assert int(idx.max()) < 100
