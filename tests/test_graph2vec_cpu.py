"""cogdl_amd.embedding.graph2vec on the CPU (host twins only): its WL documents against the golden record of the reference's
own feature_extractor (tests/golden/graph2vec_wl.npz, written by make_golden_graph2vec.py); the vocabulary cut; the Doc2Vec
shim; embedding quality of the sequential twin on two graph families."""
import functools
import os

import numpy as np
import pytest
import torch

from cogdl_amd import embedding

HERE = os.path.dirname(os.path.abspath(__file__))


def golden_graphs():
    z = np.load(os.path.join(HERE, "golden", "graph2vec_wl.npz"))
    graphs = []
    for g in range(len(z["has_x"])):
        ei = torch.from_numpy(z["edges"][:, z["edge_ptr"][g]:z["edge_ptr"][g + 1]])
        x = torch.from_numpy(z["x"][z["x_ptr"][g]:z["x_ptr"][g + 1]]) if z["has_x"][g] else None
        graphs.append((ei, x))
    return z, graphs


def test_documents_map_onto_the_references_words_by_a_bijection_position_for_position():
    z, graphs = golden_graphs()
    doc_ptr, tok, rnd, node, classes = embedding.graph2vec_documents(graphs, int(z["rounds"]))
    assert doc_ptr.tolist() == z["doc_ptr"].tolist()
    there, back = {}, {}
    for g in range(len(graphs)):
        lo, hi = int(doc_ptr[g]), int(doc_ptr[g + 1])
        # the reference walks the nodes in networkx insertion order, this library in id order: align by (round, node)
        order = np.lexsort((z["node"][lo:hi], z["round"][lo:hi]))
        assert rnd[lo:hi].tolist() == z["round"][lo:hi][order].tolist()
        assert node[lo:hi].tolist() == z["node"][lo:hi][order].tolist()
        for mine, theirs in zip(tok[lo:hi].tolist(), z["word"][lo:hi][order].tolist()):
            assert there.setdefault(mine, theirs) == theirs and back.setdefault(theirs, mine) == mine
    assert len(there) == len(back) == len(set(z["word"].tolist()))
    # words are shared across graphs (0 and 1 are one structure) and distinct across rounds
    assert sorted(tok[doc_ptr[0]:doc_ptr[1]].tolist()) == sorted(tok[doc_ptr[1]:doc_ptr[2]].tolist())
    for r in range(int(z["rounds"])):
        assert int(tok[rnd == r].max()) < int(tok[rnd == r + 1].min())
    assert int(classes.sum()) >= len(there)


def test_graph_inputs_and_errors():
    z, graphs = golden_graphs()
    tuples = [((ei[0], ei[1]), x) for ei, x in graphs]  # a Graph's edge_index is a (row, col) pair
    a = embedding.graph2vec_documents(graphs, 2)
    b = embedding.graph2vec_documents(tuples, 2)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    with pytest.raises(ValueError):
        embedding.graph2vec_documents([], 2)
    with pytest.raises(ValueError):
        embedding.graph2vec_documents([(torch.tensor([[0], [3]]), torch.zeros(2, 2))], 1)  # node 3 has no row of x
    star = torch.stack([torch.zeros(32769, dtype=torch.long), torch.arange(1, 32770)])
    with pytest.raises(embedding.DegreeCapError):
        embedding.graph2vec_documents([(star, None)], 1)


def test_vocabulary_cut_and_shapes():
    _, graphs = golden_graphs()
    emb = embedding.graph2vec(graphs, dim=8, rounds=2, min_count=1, epochs=2, seed=3, workers=1)
    again = embedding.graph2vec(graphs, dim=8, rounds=2, min_count=1, epochs=2, seed=3, workers=1)
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (len(graphs), 8) and torch.isfinite(emb).all()
    assert torch.equal(emb, again)
    from cogdl_amd.operators.pvdbow import init_tables

    untouched = embedding.graph2vec(graphs, dim=8, rounds=2, min_count=10 ** 6, epochs=2, seed=3, workers=1)  # no word is kept
    assert torch.equal(untouched, init_tables(len(graphs), 1, 8, 3, "cpu")[0])
    assert not torch.equal(emb, untouched)


def test_doc2vec_shim_serves_dbow_where_gensim_selects_it():
    from cogdl_amd import gensim_compat
    from cogdl_amd.gensim_compat import Doc2Vec, KeyedVectors, TaggedDocument

    rng = np.random.default_rng(0)
    docs = [TaggedDocument(words=[str(int(t)) for t in rng.integers(0, 20, rng.integers(3, 30))], tags=["g_%d" % k]) for k in range(12)]
    assert docs[0].words is docs[0][0] and docs[0].tags == ["g_0"]
    for dm in (0, 1e-4):
        model = Doc2Vec(docs, vector_size=10, window=0, min_count=1, dm=dm, sample=0.0, workers=1, epochs=3, alpha=0.025, seed=5, device="cpu")
        assert model["g_3"].shape == (10,) and model["g_3"].dtype == np.float32
        assert np.array_equal(model["g_3"], model.dv["g_3"]) and np.array_equal(model["g_3"], model.docvecs["g_3"])
        assert isinstance(model.wv, KeyedVectors) and model.wv.vectors.shape == (len(model.wv), 10) and "g_3" in model.dv
        assert np.isfinite(model.dv.vectors).all() and model.dv.vectors.shape == (12, 10)
    again = Doc2Vec(docs, vector_size=10, window=0, min_count=1, dm=1e-4, sample=0.0, workers=1, epochs=3, alpha=0.025, seed=5, device="cpu")
    assert np.array_equal(model.dv.vectors, again.dv.vectors)
    for kw in (dict(dm=1), dict(hs=1), dict(negative=0), dict(dbow_words=1)):
        with pytest.raises(NotImplementedError):
            Doc2Vec(docs, vector_size=10, device="cpu", **dict(dict(dm=0), **kw))
    assert gensim_compat.models.doc2vec.Doc2Vec is Doc2Vec and gensim_compat.models.doc2vec.TaggedDocument is TaggedDocument
    assert gensim_compat.SUBMODULES["gensim.models.doc2vec"] is gensim_compat.models.doc2vec


# ---------------------------------------------------------------------------------------------------------- quality
QUALITY = dict(dim=32, rounds=2, min_count=2, epochs=20, seed=4)


@functools.lru_cache(maxsize=None)
def two_families(count=80, seed=1):
    """80 small graphs under random node orders: cycles with chords against caterpillar-like paths whose ends are closed into
    triangles and whose legs are triangles on a stalk.  Both families have nodes of degree 2 and 3 only, so the round-0
    vocabulary is common; the neighbourhoods differ from round 1 on.  -> (graphs, family)."""
    rng = np.random.default_rng(seed)
    graphs, family = [], []
    for k in range(count):
        n = int(rng.integers(10, 16))
        if k % 2 == 0:  # a cycle with two or three chords: degrees 2 and 3
            edges = [(i, (i + 1) % n) for i in range(n)]
            starts = rng.choice(n // 2 - 1, int(rng.integers(2, 4)), replace=False)
            edges += [(int(s), int(s) + n // 2) for s in starts]
        else:  # a path closed into triangles at both ends; one or two inner nodes carry a triangle on a stalk
            edges = [(i, i + 1) for i in range(n - 1)] + [(0, 2), (n - 3, n - 1)]
            legs = rng.choice(np.arange(3, n - 3), int(rng.integers(1, 3)), replace=False)
            extra = n
            for v in legs:
                edges += [(int(v), extra), (extra, extra + 1), (extra + 1, extra + 2), (extra + 2, extra)]
                extra += 3
        perm = rng.permutation(max(max(e) for e in edges) + 1)
        ei = torch.tensor([[int(perm[a]), int(perm[b])] for a, b in edges], dtype=torch.long).t().contiguous()
        graphs.append((ei, None))
        family.append(k % 2)
    return graphs, np.asarray(family)


def purity(x, family):
    x = torch.as_tensor(x).detach().cpu().double()
    x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-30)
    sim = x @ x.T
    sim.fill_diagonal_(-np.inf)
    family = torch.as_tensor(family)
    return float((family[sim.argmax(1)] == family).double().mean())


@functools.lru_cache(maxsize=None)
def twin_purity():
    graphs, family = two_families()
    return purity(embedding.graph2vec(graphs, workers=1, device="cpu", **QUALITY), family)


def test_sequential_twin_separates_the_two_families_and_round_0_does_not():
    graphs, family = two_families()
    doc_ptr, tok, rnd, _, classes = embedding.graph2vec_documents(graphs, 2)
    # the families share their degree vocabulary: every round-0 word occurs in both
    doc = torch.repeat_interleave(torch.arange(len(graphs)), doc_ptr[1:] - doc_ptr[:-1])
    fam = torch.as_tensor(family)[doc]
    r0 = rnd == 0
    assert set(tok[r0 & (fam == 0)].tolist()) == set(tok[r0 & (fam == 1)].tolist())
    assert int(classes[1]) > int(classes[0])
    got = twin_purity()
    print("1-NN family purity of graph2vec: sequential twin %.4f" % got)
    assert got >= 0.9
