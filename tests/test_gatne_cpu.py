"""embedding.gatne without a GPU: the pieces of the trainer on hand-made inputs (pair count, neighbour table, vocabulary order)
and the whole run on the two-layer block network of tests/_gatne_cases.py."""
import torch

import _gatne_cases as G
from cogdl_amd import embedding


def test_pair_count_is_what_the_window_rule_gives():
    # the reference's loops (gatne.py:338-349) on the same walks
    walks = [torch.tensor([[0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0]]), torch.tensor([[2, 3, 2], [1, 0, 1], [4, 4, 4]])]
    for window, skip in ((5, 2), (2, 1), (7, 3), (1, 0)):
        want = []
        for layer, ws in enumerate(walks):
            for w in ws.tolist():
                for i in range(len(w)):
                    for j in range(1, skip + 1):
                        if i - j >= 0:
                            want.append((w[i], w[i - j], layer))
                        if i + j < len(w):
                            want.append((w[i], w[i + j], layer))
        c, x, t = embedding.gatne_pairs(walks, window)
        assert c.numel() == len(want) == sum(ws.shape[0] * sum(2 * (ws.shape[1] - j) for j in range(1, skip + 1)) for ws in walks)
        assert sorted(zip(c.tolist(), x.tolist(), t.tolist())) == sorted(want)
    # a walk that ended early (-1) pairs only what it holds
    c, x, t = embedding.gatne_pairs([torch.tensor([[3, 4, -1, -1]])], 5)
    assert sorted(zip(c.tolist(), x.tolist())) == [(3, 4), (4, 3)]


def test_neighbour_table_obeys_its_three_rules():
    # six nodes, S = 3.  layer 0: node 0 has five neighbours (1, 2, 3, 4 and 1 again: multiplicity), node 5 none;
    # layer 1: node 5 has one neighbour, node 2 exactly three, nodes 0 and 1 none
    layer0 = torch.tensor([[0, 1], [0, 2], [3, 0], [0, 4], [1, 0]])
    layer1 = torch.tensor([[5, 4], [2, 3], [2, 4], [5, 2]])
    s = 3
    a = embedding.gatne_neighbors([layer0, layer1], 6, s, torch.Generator().manual_seed(0))
    b = embedding.gatne_neighbors([layer0, layer1], 6, s, torch.Generator().manual_seed(1))
    assert tuple(a.shape) == (6, 2, s) and a.dtype == torch.int64
    lists = [[[] for _ in range(2)] for _ in range(6)]
    for t, e in enumerate((layer0, layer1)):
        for x, y in e.tolist():
            lists[x][t].append(y)
            lists[y][t].append(x)
    seen_more = set()
    for table in (a, b):
        for node in range(6):
            for t in range(2):
                have, got = lists[node][t], table[node, t].tolist()
                if not have:
                    assert got == [node] * s
                elif len(have) <= s:
                    assert sorted(got[:len(have)]) == sorted(have) and set(got[len(have):]) <= set(have)
                else:
                    assert set(got) <= set(have)
                    seen_more.update(got)
    assert lists[0][0].count(1) == 2 and len(lists[0][0]) == 5 and lists[5][0] == [] and len(lists[2][1]) == 3
    assert len(seen_more) > 1  # (draws, not a fixed slot)
    assert torch.equal(a, embedding.gatne_neighbors([layer0, layer1], 6, s, torch.Generator().manual_seed(0)))


def test_vocabulary_is_in_descending_count_order_with_ties_by_id():
    walks = [torch.tensor([[7, 3, 7], [3, 9, 7]]), torch.tensor([[2, 9, 2], [5, 5, 0]])]
    nodes, index_of = embedding.gatne_vocabulary(walks, 12)
    assert nodes.tolist() == [7, 2, 3, 5, 9, 0]  # counts 3, 2, 2, 2, 2, 1
    assert index_of[nodes].tolist() == list(range(6)) and int((index_of < 0).sum()) == 6


def test_layer_graph_is_undirected_and_simple():
    indptr, indices = embedding.gatne_layer_csr(torch.tensor([[0, 1], [1, 0], [0, 1], [2, 2], [3, 1]]), 5)
    assert indptr.tolist() == [0, 1, 3, 4, 5, 5] and indices.tolist() == [1, 0, 3, 2, 1]


def test_the_run_on_the_block_network():
    G.check_run("cpu")


def test_nodes_of_the_run_are_in_descending_count_order_and_t1_trains():
    layers, _ = G.network()
    emb, nodes = embedding.gatne([layers[1]], dim=8, edge_dim=3, att_dim=4, neighbor_samples=3, walk_num=2, walk_length=6, epochs=1,
                                 batch_size=1000, lr=0.01, seed=3, device="cpu")
    assert tuple(emb.shape) == (1, nodes.numel(), 8) and bool(torch.isfinite(emb).all())
    assert nodes.numel() == torch.unique(layers[1]).numel()
