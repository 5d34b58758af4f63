"""cogdl_amd.operators.genaggr.gen_aggregate on the GPU (cogdl_hip_gen_aggr_fwd / cogdl_hip_gen_aggr_bwd, csrc/genaggr.hip) on
the cases of tests/_gen_cases.py:
  * sum and mean: rows of at most `exact_row_edges` edges are the CPU composition's bytes (torch's deterministic mode = the
    sequential edge order), output, grad of x and grad of eterm; a one-edge row of the softmax is its message bit for bit;
  * softmax: output and the three gradients against the float64 oracle under the rule err_new <= 4 err_ref + 8 eps32 max|oracle|,
    every width, hub rows included; beta * m up to ~1000 stays finite and inside the rule (the maximum is carried); the
    gradient is exactly 0 where x + eterm == 0; two runs give the same bytes;
  * x and eterm at a storage offset: the vector-width 1 and 2 paths chosen by pointer alignment;
  * errors and torch routes; a second call on the same index tensors is captured and replayed on one stream."""
import warnings

import pytest
import torch

import _gen_cases as C
from cogdl_amd import _lib
from cogdl_amd.operators import genaggr as GA
from cogdl_amd.operators.ops import TorchRouteWarning

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dev_graph():
    """The same index tensors for every case: the plans are built once."""
    return tuple(t.to(DEV) for t in C.graph())


def _ours(dev_graph, aggr):
    row, col = dev_graph
    return lambda x, t, b: GA.gen_aggregate(x, row, col, t, aggr, b, C.EPS, num_nodes=C.N)


def _same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _short():
    row, col = C.graph()
    thresh = _lib.hip().cogdl_hip_exact_row_edges(row.numel())
    assert thresh == 128
    return torch.bincount(row, minlength=C.N) <= thresh, torch.bincount(col, minlength=C.N) <= thresh


@pytest.mark.parametrize("width", C.WIDTHS)
@pytest.mark.parametrize("with_eterm", [False, True])
def test_sum_and_mean_are_the_cpu_bytes_on_short_rows(dev_graph, width, with_eterm):
    x, eterm, G = C.inputs(width, with_eterm)
    dst_short, src_short = _short()
    assert int((~dst_short).sum()) == 2 and not bool(src_short[C.HUB_SOURCE])
    for aggr in ("sum", "mean"):
        oracle, ref32 = C.reference(width, with_eterm, aggr)
        got = C.run(_ours(dev_graph, aggr), x, eterm, None, G, False, device=DEV)
        assert _same(got["out"][dst_short], ref32["out"][dst_short]), aggr
        assert _same(got["g_x"][src_short], ref32["g_x"][src_short]), aggr
        if with_eterm:
            assert _same(got["g_eterm"], ref32["g_eterm"]), aggr
        C.check("gpu F=%d eterm=%d %s" % (width, with_eterm, aggr), got, oracle, ref32)  # (the two long rows, the hub source)
        again = C.run(_ours(dev_graph, aggr), x, eterm, None, G, False, device=DEV)
        assert all(_same(again[k], got[k]) for k in got), aggr  # no atomics


@pytest.mark.parametrize("width", C.WIDTHS)
@pytest.mark.parametrize("with_eterm", [False, True])
def test_softmax_against_the_oracle(dev_graph, width, with_eterm):
    row, col = C.graph()
    x, eterm, G = C.inputs(width, with_eterm)
    one = int((row == 1).nonzero()[0])
    for beta, learn in ((0.75, True), (None, False), (3.0, False)):
        oracle, ref32 = C.reference(width, with_eterm, "softmax", beta, learn)
        got = C.run(_ours(dev_graph, "softmax"), x, eterm, beta, G, learn, device=DEV)
        assert got.keys() == oracle.keys() and ("g_beta" in got) == learn
        C.check("gpu F=%d eterm=%d softmax beta=%s" % (width, with_eterm, beta), got, oracle, ref32)
        m = torch.relu(x[col[one]] + (eterm[one] if with_eterm else 0)) + C.EPS
        assert _same(got["out"][1], m)  # a one-edge row: its message, bit for bit
        assert _same(got["out"][0], torch.zeros(width)) and not got["out"][260:].any()  # empty rows
        assert not got["g_x"][280:].any()  # sources without out-edges
        if with_eterm:  # torch's relu: no gradient at exactly 0
            at = (x[col] + eterm) == 0
            assert int(at.sum()) >= 40 and not got["g_eterm"][at].any()
        again = C.run(_ours(dev_graph, "softmax"), x, eterm, beta, G, learn, device=DEV)
        assert all(_same(again[k], got[k]) for k in got)  # no atomics, fixed merge order


@pytest.mark.parametrize("width", [7, 128])
def test_large_logits_carry_the_maximum(dev_graph, width):
    """beta * m up to about 1000: exp(beta * m) alone overflows float32 from 88.7 on."""
    row, col = C.graph()
    scale, beta = 10.0, 25.0
    x, eterm, G = C.inputs(width, True, scale)
    top = float(beta * (torch.relu(x[col] + eterm) + C.EPS).max())
    assert 600 < top < 2000, top
    oracle, ref32 = C.reference(width, True, "softmax", beta, True, scale)
    got = C.run(_ours(dev_graph, "softmax"), x, eterm, beta, G, True, device=DEV)
    C.check("gpu F=%d large logits (max beta * m = %.0f)" % (width, top), got, oracle, ref32)


@pytest.mark.parametrize("offset", [1, 2])
def test_misaligned_tables_take_the_narrow_vector_paths(dev_graph, offset):
    """x and eterm that start 4 (8) bytes into their storage: vector width 1 (2) by pointer alignment, with the workspace that
    was sized for the 16-byte geometry.  Per column the arithmetic of a short row does not depend on the width: the same bytes as
    the aligned call there; everything, long rows included, inside the rule.  (The pieces of a long row are cut by the number of
    lane groups, which follows the width: its `out` and `lse` may differ in the last bits, and with them the softmax gradient of
    every source that sends into a long row -- those sources are compared under the rule only.)"""
    width = 64
    x, eterm, G = C.inputs(width, True)
    row, col = C.graph()
    dst_short, src_short = _short()
    feeds_long = torch.zeros(C.N, dtype=torch.bool)
    feeds_long[col[~dst_short[row]]] = True
    src_exact = {"softmax": src_short & ~feeds_long, "mean": src_short}  # (sum / mean: the gradient does not read `out`)
    assert int((torch.bincount(col, minlength=C.N)[src_exact["softmax"]] > 0).sum()) >= 5 and int(feeds_long.sum()) > 100

    def shifted(t):
        store = torch.zeros(t.numel() + offset, device=DEV)
        view = store[offset:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
        return view.requires_grad_()

    for aggr, beta in (("softmax", 0.75), ("mean", None)):
        oracle, ref32 = C.reference(width, True, aggr, beta, False)
        aligned = C.run(_ours(dev_graph, aggr), x, eterm, beta, G, False, device=DEV)
        xs, ts = shifted(x), shifted(eterm)
        out = _ours(dev_graph, aggr)(xs, ts, beta)
        out.backward(G.to(DEV))
        got = {"out": out.detach().cpu(), "g_x": xs.grad.cpu(), "g_eterm": ts.grad.cpu()}
        C.check("gpu F=%d offset %d %s" % (width, offset, aggr), got, oracle, ref32)
        assert _same(got["out"][dst_short], aligned["out"][dst_short]), aggr
        assert _same(got["g_x"][src_exact[aggr]], aligned["g_x"][src_exact[aggr]]), aggr


def test_errors_and_routes(dev_graph):
    row, col = C.graph()
    x, eterm, _ = C.inputs(7, True)
    xd, td = x.to(DEV), eterm.to(DEV)
    for which, bad in ((0, C.N), (0, -1), (1, C.N), (1, -1)):  # refused by the plan of that view: no kernel gathers
        idx = [row.clone(), col.clone()]
        idx[which][17] = bad
        with pytest.raises(_lib.BackendError):
            GA.gen_aggregate(xd, idx[0].to(DEV), idx[1].to(DEV), td, num_nodes=C.N)
    with pytest.raises(ValueError):
        GA.gen_aggregate(xd, *dev_graph, aggr="max")
    with pytest.raises(ValueError):
        GA.gen_aggregate(xd, *dev_graph, eterm=td[:, :6])
    GA._ROUTE_NOTED.clear()
    want = C.composition(x.double(), row, col, eterm.double(), "softmax", 0.75, C.EPS, C.N)
    with pytest.warns(TorchRouteWarning):  # another dtype
        got = GA.gen_aggregate(xd.double(), *dev_graph, td.double(), "softmax", 0.75, C.EPS)
    assert got.dtype == torch.float64 and torch.allclose(got.cpu(), want, rtol=1e-12, atol=1e-12)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the second call of the same kind is silent
        GA.gen_aggregate(xd.double(), *dev_graph, td.double(), "softmax", 0.75, C.EPS)
    with pytest.warns(TorchRouteWarning):  # tensors on two devices: beta on the CPU
        got = GA.gen_aggregate(xd, *dev_graph, td, "softmax", torch.tensor(0.75), C.EPS)
    assert torch.allclose(got.cpu().double(), want, rtol=1e-4, atol=1e-5)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    with pytest.warns(TorchRouteWarning):  # E == 0: zeros
        out = GA.gen_aggregate(xd, empty, empty)
    assert out.shape == (C.N, 7) and not out.any()
    with pytest.warns(TorchRouteWarning):  # F == 0
        assert GA.gen_aggregate(xd[:, :0], *dev_graph).shape == (C.N, 0)
    with pytest.warns(TorchRouteWarning):  # an empty x
        assert GA.gen_aggregate(xd[:0], empty[:0].clone(), empty[:0].clone(), num_nodes=0).shape == (0, 7)


def test_capture_on_one_stream(dev_graph):
    width = 64
    x, eterm, G = C.inputs(width, True)
    xd, td = x.to(DEV).requires_grad_(), eterm.to(DEV).requires_grad_()
    beta = torch.tensor([0.75], device=DEV, requires_grad=True)
    Gd = G.to(DEV)

    def step():
        out = GA.gen_aggregate(xd, *dev_graph, td, "softmax", beta, C.EPS, num_nodes=C.N)
        out2 = GA.gen_aggregate(xd, *dev_graph, None, "mean", None, C.EPS, num_nodes=C.N)
        gx, gt, gb = torch.autograd.grad([out, out2], [xd, td, beta], [Gd, Gd])
        return out.detach(), out2.detach(), gx, gt, gb

    want = [t.clone() for t in step()]  # (the plans, the int32 copies and the workspaces exist after this)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(got, want))
    with torch.no_grad():  # beta is read by the kernel through its address: a replay sees the new value
        beta.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        fresh = GA.gen_aggregate(xd, *dev_graph, td, "softmax", beta, C.EPS, num_nodes=C.N)
    assert _same(got[0], fresh) and not _same(got[0], want[0])
