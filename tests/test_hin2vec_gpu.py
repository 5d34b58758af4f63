"""hin_pairs and hin_scores on the GPU (csrc/hin2vec.hip): the pair kernels against the host twin, element for element, and
against the Python loop; the scorer against the float64 composition under the project's acceptance rule; determinism, the
torch route, and embedding.hin2vec end to end."""
import warnings

import pytest
import torch

import _hin2vec_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("W,L,hop,negative,T", cases.PAIR_CASES)
def test_pairs_equal_the_host_twin_and_the_loop(W, L, hop, negative, T):
    from cogdl_amd.operators.hin2vec import hin_pairs

    walks, node_type = cases.pair_inputs(W, L, hop, T)
    host = hin_pairs(walks, node_type, hop, negative, seed=11)
    gpu = hin_pairs(walks.to(DEV), node_type.to(DEV), hop, negative, seed=11)
    for name, a, b in zip("x y key label".split(), gpu, host):
        assert a.device.type == "cuda" and a.dtype == torch.int64 and torch.equal(a.cpu(), b), name
    positives = [row[::1 + negative].tolist() for row in (t.cpu() for t in gpu[:3])]
    assert list(zip(*positives)) == cases.loop_positives(walks, node_type, hop)


@pytest.mark.parametrize("B,N,R,d", cases.SCORE_CASES)
def test_scores_and_gradients_against_float64(B, N, R, d):
    from cogdl_amd.operators.hin2vec import hin_scores

    (Wx, Wr, x, y, r, G), oracle, err_ref = cases.score_case(B, N, R, d)

    def run():
        a, b = Wx.to(DEV).requires_grad_(), Wr.to(DEV).requires_grad_()
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # the HIP route: no TorchRouteWarning
            p = hin_scores(a, b, x.to(DEV), y.to(DEV), r.to(DEV))
        p.backward(G.to(DEV))
        return p.detach(), a.grad, b.grad

    first, second = run(), run()
    for name, got, again, want, ref in zip(("p", "grad_Wx", "grad_Wr"), first, second, oracle, err_ref):
        assert got.dtype == torch.float32 and torch.equal(got, again), "%s differs between two runs" % name
        cases.accept(name, got, want, ref)
    assert not first[1][N - 1].any(), "a node that never occurs has a gradient"
    assert R == 1 or not first[2][R - 1].any(), "a relation that never occurs has a gradient"


def test_float64_takes_the_torch_route_with_one_warning():
    from cogdl_amd.operators import hin2vec, ops

    (Wx, Wr, x, y, r, _), oracle, _ = cases.score_case(70, 9, 3, 6)
    ops._ROUTE_NOTED.discard(("hin_scores", "dtype torch.float64"))
    args = [t.to(DEV) for t in (Wx.double(), Wr.double(), x, y, r)]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        p = hin2vec.hin_scores(*args)
        hin2vec.hin_scores(*args)
    assert [w.category for w in seen] == [ops.TorchRouteWarning]
    assert p.dtype == torch.float64 and torch.allclose(p.cpu(), oracle[0], rtol=0, atol=1e-12)


def test_embedding_hin2vec_end_to_end():
    from cogdl_amd import embedding

    n = 40
    src = torch.arange(n)
    row = torch.cat([src, src, src])
    col = torch.cat([(src + 1) % n, (src + 7) % n, (src * 3 + 2) % n])
    order = torch.argsort(row, stable=True)
    indptr = torch.zeros(n + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    graph = (indptr.to(DEV), col[order].to(DEV))
    node_type = (src % 3).to(DEV)
    runs = [embedding.hin2vec(graph, node_type, dim=16, walk_length=6, walk_num=2, batch_size=100, epochs=1, seed=5)
            for _ in range(2)]
    assert runs[0].is_cuda and runs[0].dtype == torch.float32 and tuple(runs[0].shape) == (n, 16)
    assert bool(torch.isfinite(runs[0]).all()) and torch.equal(runs[0], runs[1])
