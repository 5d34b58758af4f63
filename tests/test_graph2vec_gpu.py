"""cogdl_amd.embedding.graph2vec on the GPU: the WL documents equal the CPU's, and the throughput mode of the PV-DBOW kernel
reaches the sequential CPU twin's 1-NN family purity on 80 small graphs of two families."""
import pytest
import torch

from cogdl_amd import embedding

from test_graph2vec_cpu import QUALITY, golden_graphs, purity, twin_purity, two_families

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_documents_on_the_gpu_equal_the_cpus():
    for graphs in (golden_graphs()[1], two_families()[0]):
        cpu = embedding.graph2vec_documents(graphs, 2, device="cpu")
        gpu = embedding.graph2vec_documents(graphs, 2, device=DEV)
        assert all(g.is_cuda and torch.equal(g.cpu(), c) for g, c in zip(gpu, cpu))


def test_graph2vec_separates_two_families_like_the_cpu_twin():
    graphs, family = two_families()
    host = twin_purity()
    emb = embedding.graph2vec(graphs, device=DEV, **QUALITY)
    assert emb.is_cuda and emb.dtype == torch.float32 and tuple(emb.shape) == (len(graphs), QUALITY["dim"])
    assert torch.isfinite(emb).all()
    got = purity(emb, family)
    print("1-NN family purity of graph2vec: GPU %.4f, sequential CPU twin %.4f" % (got, host))
    assert host >= 0.9
    assert got >= host - 0.05
