"""Unsupervised node embeddings without leaving the device: walks from the library's walk operators, trained by the
library's skip-gram operator -- what the reference's DeepWalk / Node2vec do through networkx and gensim
(cogdl/models/emb/deepwalk.py:54-110, node2vec.py:72-140).

    deepwalk(graph_or_csr, dim, walk_length, walk_num, window, epochs)      -> float32 [N, dim]
    node2vec(graph_or_csr, dim, walk_length, walk_num, window, epochs, p, q) -> float32 [N, dim]
    netsmf(graph_or_csr, dim, window, negative, rounds)                     -> float32 [N, dim]
    metapath2vec(graph_or_csr, node_type, schema, dim, walk_length, walk_num, window, epochs) -> float32 [N, dim]
    prone(graph_or_csr, dim, step, mu, theta)                               -> float32 [N, dim]
    graph2vec(graphs, dim, rounds, min_count, epochs)                       -> float32 [G, dim]  (one row per graph)
    line(graph_or_csr, dim, walk_length, walk_num, negative, alpha, order)  -> float32 [N, dim]
    gatne(layers, dim, walk_length, walk_num, window, epochs, batch_size, ...) -> (float32 [T, N, dim], nodes int64 [N])

`graph_or_csr` is a cogdl Graph (its row_indptr / col_indices are used on the device they live on) or an
(indptr, indices) pair of int64 tensors.  Each of the walk_num passes starts one walk at every node, in an order shuffled
per pass (as the reference does); the passes' rows follow each other, which is the order the trainer consumes them in.
Differences from the reference: the draws come from Philox, not from numpy's / gensim's generators; at a node without
out-neighbours the walker stays (the reference ends the walk); node2vec ignores edge weights.  metapath2vec (the walk of
cogdl/models/emb/metapath2vec.py:87-125) ends a walk where no neighbour has the wanted type, as the reference does.

netsmf is the matrix-factorisation member of the family (cogdl/models/emb/netsmf.py): path samples counted into a sparse
matrix, the sparsifier's log transform, a randomized SVD -- all three from cogdl_amd/operators/netsmf.py, nothing trained.

prone is the other one (cogdl/models/emb/prone.py): an elementwise transform of the adjacency's entries, the same randomized
SVD, the spectral propagation of cogdl_amd/operators/spectral.py (one fused filter step per sparse product) and a dense
embedding from the [dim, dim] Gram matrix.

line is the edge-sampling member (cogdl/models/emb/line.py): no walks, walk_length * walk_num * N edge samples trained by
cogdl_amd/operators/line.py, orders 1 and 2 side by side for order 3.
"""
import math

import torch

from .operators.sgns import skipgram
from .operators.walk import _seed, metapath_walk, node2vec_walk, parse_schema, random_walk


def _csr(graph_or_csr):
    if isinstance(graph_or_csr, (tuple, list)):
        indptr, indices = graph_or_csr
    else:
        indptr, indices = graph_or_csr.row_indptr, graph_or_csr.col_indices
    indptr, indices = torch.as_tensor(indptr), torch.as_tensor(indices)
    return indptr.long().contiguous(), indices.to(indptr.device).long().contiguous()


def _starts(n, walk_num, seed, device):
    gen = torch.Generator().manual_seed(seed % (2 ** 63))
    return torch.cat([torch.randperm(n, generator=gen) for _ in range(walk_num)]).to(device)


def _embed(walk, graph_or_csr, dim, walk_length, walk_num, window, epochs, seed, negative, alpha, min_alpha, sample, workers):
    walk_num = int(walk_num)
    if walk_num < 1:
        raise ValueError("walk_num must be >= 1 (got %d)" % walk_num)
    indptr, indices = _csr(graph_or_csr)
    n = indptr.numel() - 1
    seed = _seed(seed)
    start = _starts(n, walk_num, seed, indptr.device)
    walks = walk(indptr, indices, start, (seed + 1) & (2 ** 64 - 1))
    syn0, _ = skipgram(walks, n, dim=dim, window=window, negative=negative, epochs=epochs, alpha=alpha, min_alpha=min_alpha,
                       sample=sample, seed=(seed + 2) & (2 ** 64 - 1), workers=workers)
    return syn0


def deepwalk(graph_or_csr, dim=128, walk_length=80, walk_num=40, window=5, epochs=5, seed=None, negative=5, alpha=0.025,
             min_alpha=1e-4, sample=1e-3, workers=0):
    """DeepWalk: uniform walks, then skip-gram with negative sampling.  -> float32 [N, dim] on the graph's device."""
    return _embed(lambda ip, ix, st, sd: random_walk(ip, ix, st, walk_length, seed=sd), graph_or_csr, dim, walk_length, walk_num,
                  window, epochs, seed, negative, alpha, min_alpha, sample, workers)


def node2vec(graph_or_csr, dim=128, walk_length=80, walk_num=40, window=5, epochs=5, p=1.0, q=1.0, seed=None, negative=5,
             alpha=0.025, min_alpha=1e-4, sample=1e-3, workers=0):
    """node2vec: second-order walks with return parameter p and in-out parameter q, then skip-gram."""
    return _embed(lambda ip, ix, st, sd: node2vec_walk(ip, ix, st, walk_length, p=p, q=q, seed=sd), graph_or_csr, dim, walk_length,
                  walk_num, window, epochs, seed, negative, alpha, min_alpha, sample, workers)


def metapath2vec(graph_or_csr, node_type, schema, dim=128, walk_length=80, walk_num=20, window=5, epochs=10, seed=None,
                 negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, workers=0, nodes=None, return_walks=False):
    """metapath2vec: walks that follow a node-type schema ("0-1-0,0-2-0,1-0-2-0-1", or a list of integer lists), then
    skip-gram.  -> float32 [N, dim] on the graph's device.  For every metapath, each of the walk_num passes starts one walker
    at every node of the metapath's first type, in an order shuffled per pass; a walk that meets a node without a neighbour of
    the wanted type ends there (the rest of its row is -1, which skipgram skips).  schema="No" is the reference's
    type-agnostic walk: one metapath over a single type.  `nodes` (int64 ids) restricts the start nodes (the reference starts
    at the nodes that occur in an edge); return_walks=True also returns the int64 [W, walk_length] walks.  A node that no
    walk visits keeps its initial row."""
    walk_num = int(walk_num)
    if walk_num < 1:
        raise ValueError("walk_num must be >= 1 (got %d)" % walk_num)
    indptr, indices = _csr(graph_or_csr)
    dev, n = indptr.device, indptr.numel() - 1
    if isinstance(schema, str) and schema == "No":
        node_type, paths = torch.zeros(n, dtype=torch.int32, device=dev), [[0, 0]]
    else:
        node_type, paths = torch.as_tensor(node_type).to(dev).contiguous(), parse_schema(schema)
        if node_type.dtype not in (torch.int32, torch.long):
            raise ValueError("node_type must be an integer tensor (got %s)" % node_type.dtype)
    if node_type.dim() != 1 or node_type.numel() != n:
        raise ValueError("node_type must have one entry per node (%d)" % n)
    seed = _seed(seed)
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    if nodes is not None:
        mask = torch.zeros(n, dtype=torch.bool, device=dev)
        mask[torch.as_tensor(nodes, dtype=torch.long, device=dev)] = True
    firsts = [torch.nonzero(mask & (node_type == items[0])).flatten().cpu() for items in paths]
    gen = torch.Generator().manual_seed(seed % (2 ** 63))
    start, which = [], []
    for _ in range(walk_num):
        for p, first in enumerate(firsts):
            start.append(first[torch.randperm(first.numel(), generator=gen)])
            which.append(torch.full((first.numel(),), p, dtype=torch.int32))
    start, which = torch.cat(start).to(dev), torch.cat(which).to(dev)
    if start.numel() == 0:
        raise ValueError("metapath2vec: no node has the first type of a metapath of %r" % (schema,))
    walks = metapath_walk(indptr, indices, node_type, start, paths, walk_length, walker_path=which, seed=(seed + 1) & (2 ** 64 - 1))
    syn0, _ = skipgram(walks, n, dim=dim, window=window, negative=negative, epochs=epochs, alpha=alpha, min_alpha=min_alpha,
                       sample=sample, seed=(seed + 2) & (2 ** 64 - 1), workers=workers)
    return (syn0, walks) if return_walks else syn0


class DegreeCapError(ValueError):
    """A node of the batch has more neighbours than wl_labels sorts in one workgroup."""


def _edge_pair(edge_index):
    row, col = (edge_index[0], edge_index[1])
    return torch.as_tensor(row).long().flatten(), torch.as_tensor(col).long().flatten()


def graph2vec_documents(graphs, rounds=2, device=None):
    """The WL documents of a list of graphs (cogdl Graphs, or (edge_index, x_or_None) pairs) on `device` (default: the
    device of the first graph's edges) -> (doc_ptr int64 [G + 1], token int64 [T], round int64 [T], node int64 [T], classes
    int64 [rounds + 1]): graph g owns the positions [doc_ptr[g], doc_ptr[g + 1]), ordered by (round, node id); node ids are
    the graph's own; token = classes[0] + .. + classes[round - 1] + labels[round][node] over the whole batch.

    Per graph the edges are symmetrised and duplicates dropped (networkx's from_edgelist: undirected and simple, a
    self-loop kept once); one batched CSR is built with the library's COO to CSR route.  Round-0 labels: with x the id of
    the node's feature row (rows equal as float32 arrays share a label, across graphs), without x the networkx degree (a
    self-loop counts 2).  In rounds 1..R the nodes that occur in an edge contribute; in round 0 every row of x does when x
    is given, otherwise the same nodes -- as the reference's feature_extractor / wl_iterations do."""
    from .graph_build import coo2csr_index
    from .operators.wl import MAX_DEGREE, wl_labels

    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("graph2vec: rounds must be >= 0 (got %d)" % rounds)
    pairs = []
    for g in graphs:
        if isinstance(g, (tuple, list)) and len(g) == 2:
            pairs.append((g[0], g[1]))
        else:
            pairs.append((g.edge_index, getattr(g, "x", None)))
    if not pairs:
        raise ValueError("graph2vec: an empty list of graphs")
    edges = [_edge_pair(ei) for ei, _ in pairs]
    dev = torch.device(device) if device is not None else edges[0][0].device
    n_graphs = len(pairs)
    x_rows = torch.tensor([0 if x is None else int(x.shape[0]) for _, x in pairs], dtype=torch.long, device=dev)
    has_x = torch.tensor([x is not None for _, x in pairs], dtype=torch.bool, device=dev)
    n_edges = torch.tensor([r.numel() for r, _ in edges], dtype=torch.long, device=dev)
    row = torch.cat([r for r, _ in edges]).to(dev)
    col = torch.cat([c for _, c in edges]).to(dev)
    if row.numel() and int(torch.minimum(row.min(), col.min())) < 0:
        raise ValueError("graph2vec: a negative node id")
    gid = torch.repeat_interleave(torch.arange(n_graphs, device=dev), n_edges)
    top = torch.full((n_graphs,), -1, dtype=torch.long, device=dev)
    top.scatter_reduce_(0, gid, torch.maximum(row, col), "amax")
    if bool((has_x & (top >= x_rows)).any()):
        raise ValueError("graph2vec: an edge names a node without a row of x")
    n_nodes = torch.maximum(top + 1, x_rows)
    first = torch.zeros(n_graphs + 1, dtype=torch.long, device=dev)
    torch.cumsum(n_nodes, 0, out=first[1:])
    total = int(first[-1])
    graph_of = torch.repeat_interleave(torch.arange(n_graphs, device=dev), n_nodes)
    # the simple undirected structure of the batch
    a, b = row + first[gid], col + first[gid]
    keys = torch.unique(torch.cat([a * total + b, b * total + a]))
    src, dst = keys // max(total, 1), keys % max(total, 1)
    indptr, perm = coo2csr_index(src, dst, total)
    indices = dst[perm]
    deg = indptr[1:] - indptr[:-1]
    if total and int(deg.max()) > MAX_DEGREE:
        raise DegreeCapError("graph2vec: a node has %d neighbours, more than %d" % (int(deg.max()), MAX_DEGREE))
    in_edge = deg > 0
    loops = torch.zeros(total, dtype=torch.long, device=dev)
    loops[src[src == dst]] = 1
    label0 = (deg + loops) * 2  # the networkx degree; even, feature-row ids are odd
    if bool(has_x.any()):
        widths = set(int(x.shape[1]) if x.dim() == 2 else -1 for _, x in pairs if x is not None)
        if len(widths) != 1 or -1 in widths:
            raise ValueError("graph2vec: x must be 2-D with one width over the batch")
        feats = torch.cat([x.to(dev).float() for _, x in pairs if x is not None])
        row_id = torch.unique(feats, dim=0, return_inverse=True)[1]
        node_has_x = has_x[graph_of]
        # (a graph with x has exactly x_rows nodes, so its rows are its nodes in order)
        label0 = label0.clone()
        label0[node_has_x] = row_id * 2 + 1
    else:
        node_has_x = torch.zeros(total, dtype=torch.bool, device=dev)
    labels, classes = wl_labels(indptr.int().contiguous(), indices.int().contiguous(), label0, rounds)
    offset = torch.cumsum(classes, 0) - classes
    local = torch.arange(total, device=dev) - first[graph_of]
    tok, rnd, node, doc = [], [], [], []
    for r in range(rounds + 1):
        mask = in_edge | node_has_x if r == 0 else in_edge
        tok.append(offset[r] + labels[r][mask].long())
        rnd.append(torch.full((int(mask.sum()),), r, dtype=torch.long, device=dev))
        node.append(local[mask])
        doc.append(graph_of[mask])
    tok, rnd, node, doc = torch.cat(tok), torch.cat(rnd), torch.cat(node), torch.cat(doc)
    order = torch.sort(doc, stable=True)[1]  # (rounds follow each other, nodes ascend inside one: (graph, round, node))
    doc_ptr = torch.zeros(n_graphs + 1, dtype=torch.long, device=dev)
    torch.cumsum(torch.bincount(doc, minlength=n_graphs), 0, out=doc_ptr[1:])
    return doc_ptr, tok[order].contiguous(), rnd[order], node[order], classes


def graph2vec(graphs, dim=128, rounds=2, min_count=5, epochs=10, alpha=0.025, sample=0.0, negative=5, seed=None, workers=0,
              device=None):
    """Graph2Vec: WL subtree words per graph (graph2vec_documents), a vocabulary of the words seen at least min_count times
    (ids compacted by a prefix sum; a dropped word becomes padding), then PV-DBOW.  -> float32 [G, dim] on `device`.  A graph
    none of whose words is kept keeps its initial vector."""
    from .operators.pvdbow import doc2vec_dbow, init_tables

    doc_ptr, tok, _, _, classes = graph2vec_documents(graphs, rounds, device)
    n_tokens = int(classes.sum())
    keep = torch.bincount(tok, minlength=max(n_tokens, 1)) >= max(int(min_count), 1)
    if not bool(keep.any()):  # nothing to train on
        return init_tables(doc_ptr.numel() - 1, 1, int(dim), _seed(seed), doc_ptr.device)[0]
    new_id = torch.cumsum(keep, 0) - 1
    words = torch.where(keep[tok], new_id[tok], torch.full_like(tok, -1)) if tok.numel() else tok
    dv, _ = doc2vec_dbow(doc_ptr, words.contiguous(), max(int(keep.sum()), 1), dim=dim, negative=negative, epochs=epochs, alpha=alpha,
                         sample=sample, seed=seed, workers=workers)
    return dv


def netsmf(graph_or_csr, dim=128, window=10, negative=1, rounds=100, seed=None):
    """NetSMF on a simple symmetric graph with unit weights -> float32 [N, dim] on the graph's device: U sqrt(S) of the
    sparsifier's randomized SVD with the rows L2-normalised (netsmf.py:122-132).  `rounds` is the reference's num_round: a
    round takes every undirected edge once in a random orientation, which is half a pass over the CSR entries, so
    passes = ceil(rounds / 2).  A node without edges gets a zero row (as does any row whose U sqrt(S) is zero)."""
    from .operators.netsmf import path_counts, randomized_svd, sparsifier

    rounds, dim = int(rounds), int(dim)
    if rounds < 1:
        raise ValueError("rounds must be >= 1 (got %d)" % rounds)
    indptr, indices = _csr(graph_or_csr)
    n = indptr.numel() - 1
    if not 1 <= dim <= n:
        raise ValueError("dim must be in [1, N = %d] (got %d)" % (n, dim))
    passes = math.ceil(rounds / 2)
    seed = _seed(seed)
    rowptr, col, count = path_counts(indptr, indices, window, passes, seed=seed)
    m_rowptr, m_col, m_val = sparsifier(indptr, rowptr, col, count, window, passes, negative)
    u, s = randomized_svd(m_rowptr, m_col, m_val, n, dim, seed=(seed + 1) & (2 ** 64 - 1))
    emb = u * s.sqrt()
    norm = emb.norm(dim=1, keepdim=True)
    return torch.where(norm > 0, emb / norm.clamp_min(1e-30), torch.zeros_like(emb))


def prone_prefactorization(indptr, indices):
    """The matrix ProNE factorises (prone.py:74-92) for a simple graph with unit weights -> CSR (rowptr int32, col int32, val
    float32) with the graph's own pattern, on its device: C1 = the l1 row-normalised adjacency, neg_j = colsum_j(C1)^0.75 /
    sum_k colsum_k(C1)^0.75, entry (i, j) = log(C1_ij) - log(neg_j), with the reference's `<= 0 -> 1` replacement in front
    of each log.  The column sums are float32 sums in increasing row order: the library's transpose (csr2csc; a stable sort
    on the CPU) and its segment sum, no float atomics; the rest is elementwise float64 on the device, rounded to float32
    once.  Rows and columns of nodes of degree 0 are empty."""
    from .operators.netsmf import _transpose
    from .operators.readout import segment_pool

    n = indptr.numel() - 1
    rowptr, col = indptr.int().contiguous(), indices.int().contiguous()
    deg = (indptr[1:] - indptr[:-1])
    rows = torch.repeat_interleave(torch.arange(n, device=indptr.device), deg)
    c1 = (1.0 / deg.float())[rows].contiguous()  # (a row with an entry has deg >= 1)
    colptr, _, c1_t = _transpose(rowptr, col, c1, n)
    colsum = segment_pool(c1_t.reshape(-1, 1).contiguous(), colptr.int().contiguous(), "sum").reshape(-1).double()
    neg = colsum.pow(0.75)
    neg = neg / neg.sum()
    c1d, negd = c1.double(), neg[indices]
    c1d = torch.where(c1d <= 0, torch.ones_like(c1d), c1d)
    negd = torch.where(negd <= 0, torch.ones_like(negd), negd)
    return rowptr, col, (c1d.log() - negd.log()).float().contiguous()


def dense_embedding(x):
    """get_embedding_dense (cogdl/utils/prone_utils.py:232-241) of a tall [N, dim] matrix without a device solver: the
    [dim, dim] Gram matrix X^T X in float64 on x's device, its eigen-decomposition V diag(lam) V^T on the host in float64,
    then U sqrt(S) = X V S^(-1/2) with S = sqrt(lam) (descending) and l2-normalised rows -> float32 [N, dim].  Directions
    whose eigenvalue is below 1e-12 of the largest come out as zero columns; a zero row stays zero.  Columns are determined
    up to sign, as singular vectors are."""
    xd = x.double()
    gram = (xd.t() @ xd).cpu()
    lam, v = torch.linalg.eigh((gram + gram.t()) / 2)
    lam, v = lam.flip(0), v.flip(1)
    top = float(lam[0]) if lam.numel() else 0.0
    good = lam > 1e-12 * top if top > 0.0 else torch.zeros_like(lam, dtype=torch.bool)
    w = torch.zeros_like(v)
    w[:, good] = v[:, good] * lam[good].pow(-0.25)
    emb = xd @ w.to(x.device)
    norm = emb.norm(dim=1, keepdim=True)  # (float64 up to here: the result is rounded to float32 once)
    return torch.where(norm > 0, emb / norm.clamp_min(1e-300), torch.zeros_like(emb)).float()


def prone(graph_or_csr, dim=128, step=5, mu=0.2, theta=0.5, seed=None):
    """ProNE on a simple symmetric graph with unit weights, without self loops -> float32 [N, dim] on the graph's device:
    the pre-factorisation matrix, U sqrt(S) of its randomized SVD (n_iter = 5) with l2-normalised rows, the spectral
    propagation spectral_filter("prone", order=step, mu=mu, s=theta) -- ProNE.forward hands (step, mu, theta) to
    _chebyshev_gaussian's positional (order, mu, s), whose defaults carry the two names' values the other way round; what it
    does is followed, not the defaults -- and the dense embedding of the result.  step == 1 returns the factorisation's
    embedding as it is, as the reference does."""
    from .operators.netsmf import randomized_svd
    from .operators.spectral import spectral_filter

    dim, step = int(dim), int(step)
    if step < 1:
        raise ValueError("step must be >= 1 (got %d)" % step)
    indptr, indices = _csr(graph_or_csr)
    n = indptr.numel() - 1
    if not 1 <= dim <= n:
        raise ValueError("dim must be in [1, N = %d] (got %d)" % (n, dim))
    rowptr, col, val = prone_prefactorization(indptr, indices)
    u, s = randomized_svd(rowptr, col, val, n, dim, n_iter=5, seed=_seed(seed))
    feat = u * s.sqrt()
    norm = feat.norm(dim=1, keepdim=True)
    feat = torch.where(norm > 0, feat / norm.clamp_min(1e-30), torch.zeros_like(feat)).contiguous()
    if step == 1:
        return feat
    return dense_embedding(spectral_filter("prone", rowptr, col, feat, order=step, mu=mu, s=theta))


def gatne_layer_csr(edges, num_ids):
    """The undirected simple graph of one layer's raw edge list (int64 [E, 2]) over the ids [0, num_ids), as nx.Graph builds it:
    both directions, parallel edges collapsed, a self-loop kept once -> (indptr int64 [num_ids + 1], indices int64, ascending per
    row)."""
    a, b = edges[:, 0], edges[:, 1]
    keys = torch.unique(torch.cat([a * num_ids + b, b * num_ids + a]))
    src, dst = keys // num_ids, keys % num_ids
    indptr = torch.zeros(num_ids + 1, dtype=torch.long, device=edges.device)
    torch.cumsum(torch.bincount(src, minlength=num_ids), 0, out=indptr[1:])
    return indptr, dst.contiguous()


def gatne_vocabulary(walks, num_ids):
    """The nodes that occur in a walk, by descending count, ties in ascending id -> (nodes int64 [N], index_of int64 [num_ids]
    with -1 for an id that is in no walk)."""
    count = torch.zeros(num_ids, dtype=torch.long, device=walks[0].device)
    for w in walks:
        count += torch.bincount(w[w >= 0].reshape(-1), minlength=num_ids)
    present = torch.nonzero(count > 0).flatten()  # ascending ids
    order = torch.sort(count[present], descending=True, stable=True)[1]
    nodes = present[order].contiguous()
    index_of = torch.full((num_ids,), -1, dtype=torch.long, device=nodes.device)
    index_of[nodes] = torch.arange(nodes.numel(), device=nodes.device)
    return nodes, index_of


def gatne_pairs(walks, window=5):
    """The training pairs of a list of index walks (one int64 [W_t, L] tensor per layer, -1 = past the walk's end), by slicing:
    every position with its window // 2 predecessors and successors (generate_pairs, gatne.py:338-349)
    -> (center, context, layer), int64 [P] each, in no particular order."""
    skip = int(window) // 2
    center, context, layer = [], [], []
    for t, w in enumerate(walks):
        for j in range(1, min(skip, w.shape[1] - 1) + 1):
            for c, x in ((w[:, j:], w[:, :-j]), (w[:, :-j], w[:, j:])):
                ok = (c >= 0) & (x >= 0)
                center.append(c[ok])
                context.append(x[ok])
                layer.append(torch.full((center[-1].numel(),), t, dtype=torch.long, device=w.device))
    if not center:
        empty = torch.zeros(0, dtype=torch.long, device=walks[0].device if walks else None)
        return empty, empty.clone(), empty.clone()
    return torch.cat(center), torch.cat(context), torch.cat(layer)


def gatne_neighbors(layers, num_nodes, samples, generator=None):
    """The [N, T, S] neighbour table of GATNE (gatne.py:130-146) from the layers' raw edge lists in index space (int64 [E_t, 2]):
    both directions, with multiplicity, in edge order (forward entries before backward ones).  A node without a neighbour of a
    type gets itself S times; one with fewer than S gets all of them, then uniform draws with replacement from them; one with
    more gets S uniform draws with replacement; one with exactly S gets them as they are.  -> int64 [N, T, S]."""
    n, s = int(num_nodes), int(samples)
    dev = layers[0].device
    slot = torch.arange(s, device=dev).view(1, s)
    me = torch.arange(n, device=dev).view(n, 1).expand(n, s)
    out = []
    for e in layers:
        src, dst = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
        order = torch.sort(src, stable=True)[1]
        dst = dst[order]
        deg = torch.bincount(src, minlength=n)
        ptr = torch.cumsum(deg, 0) - deg
        deg = deg.view(n, 1)
        r = torch.rand((n, s), generator=generator, device=dev, dtype=torch.float64)
        drawn = torch.minimum((r * deg).long(), (deg - 1).clamp_min(0))
        pick = torch.where((deg > s) | (slot >= deg), drawn, slot.expand(n, s))
        if dst.numel():
            got = dst[(ptr.view(n, 1) + pick).clamp(0, dst.numel() - 1)]
        else:
            got = me
        out.append(torch.where(deg > 0, got, me))
    return torch.stack(out, dim=1).contiguous()


def gatne(layers, dim=200, walk_length=10, walk_num=10, window=5, epochs=20, batch_size=256, edge_dim=10, att_dim=20, negative=5,
          neighbor_samples=10, lr=1e-4, seed=None, device=None, return_loss=False):
    """GATNE-T (cogdl/models/emb/gatne.py:111-194) on a multiplex network: `layers` is a list of int64 [E_t, 2] edge lists, one
    per edge type, over non-negative node ids -> (emb float32 [T, N, dim], nodes int64 [N]); emb[t, k] is the embedding of node
    nodes[k] under edge type t, rows of unit norm.  With return_loss=True also the list of the mean loss of each epoch.

    Per layer the undirected simple graph (gatne_layer_csr) is walked walk_num times from every node in shuffled order
    (random_walk); the vocabulary is the nodes that occur in a walk, by descending count (ties: ascending id, where the reference
    keeps first appearance); the pairs come from gatne_pairs with the given window (the reference's forward always uses 5), the
    [N, T, S] neighbour table from gatne_neighbors.  A step takes a shuffled slice of the pairs, embeds the centres with
    operators.multiplex.multiplex_embed, scores them against the context table with operators.kgscore.sampled_scores on
    [context | negatives] (negatives from torch.multinomial over the rank weights log(k + 2) - log(k + 1)), takes
    -mean(logsigmoid(pos) + SUM logsigmoid(-neg)) and applies torch.optim.Adam(lr).  Initial values follow the reference:
    uniform(-1, 1) for the two tables, normal with std 1 / sqrt(dim) for the rest.  The final embeddings are one batched call of
    N T samples.  Everything after the edge lists stays on `device` (default: the GPU where there is one).  lr defaults to the
    reference's 1e-4, with which a small network barely moves in a few epochs.  `seed` makes a run reproducible on one device."""
    from .operators.kgscore import sampled_scores
    from .operators.multiplex import multiplex_embed

    dev = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    layers = [torch.as_tensor(e).long().reshape(-1, 2).to(dev) for e in layers]
    if not layers or any(e.numel() == 0 for e in layers):
        raise ValueError("gatne: needs at least one layer, and every layer at least one edge")
    walk_num, walk_length, epochs, batch_size = int(walk_num), int(walk_length), int(epochs), int(batch_size)
    dim, edge_dim, att_dim, negative, samples = int(dim), int(edge_dim), int(att_dim), int(negative), int(neighbor_samples)
    if min(walk_num, walk_length, batch_size, dim, edge_dim, att_dim, negative, samples) < 1 or epochs < 0:
        raise ValueError("gatne: walk_num, walk_length, batch_size, dim, edge_dim, att_dim, negative and neighbor_samples must be "
                         "at least 1, epochs at least 0")
    if int(min(int(e.min()) for e in layers)) < 0:
        raise ValueError("gatne: a negative node id")
    num_ids = max(int(e.max()) for e in layers) + 1
    seed = _seed(seed)
    t_count = len(layers)
    cpu_gen = torch.Generator().manual_seed(seed % (2 ** 63))
    walks = []
    for t, e in enumerate(layers):
        indptr, indices = gatne_layer_csr(e, num_ids)
        members = torch.nonzero(indptr[1:] > indptr[:-1]).flatten().cpu()
        start = torch.cat([members[torch.randperm(members.numel(), generator=cpu_gen)] for _ in range(walk_num)]).to(dev)
        walks.append(random_walk(indptr, indices, start, walk_length, seed=(seed + 1 + t) & (2 ** 64 - 1)))
    nodes, index_of = gatne_vocabulary(walks, num_ids)
    n = nodes.numel()
    center, context, layer = gatne_pairs([index_of[w] for w in walks], window)
    gen = torch.Generator(device=dev).manual_seed((seed + 1 + t_count) % (2 ** 63))
    neigh = gatne_neighbors([index_of[e] for e in layers], n, samples, gen)
    neigh32 = neigh.to(torch.int32)

    std = 1.0 / math.sqrt(dim)
    f32 = dict(dtype=torch.float32, device=dev)
    node_emb = (torch.rand((n, dim), generator=gen, **f32) * 2 - 1).requires_grad_()
    type_emb = (torch.rand((n, t_count, edge_dim), generator=gen, **f32) * 2 - 1).requires_grad_()
    trans_w = (torch.randn((t_count, edge_dim, dim), generator=gen, **f32) * std).requires_grad_()
    att_w1 = (torch.randn((t_count, edge_dim, att_dim), generator=gen, **f32) * std).requires_grad_()
    att_w2 = (torch.randn((t_count, att_dim), generator=gen, **f32) * std).requires_grad_()
    ctx_w = (torch.randn((n, dim), generator=gen, **f32) * std).requires_grad_()
    params = [node_emb, type_emb, trans_w, att_w1, att_w2]
    rank = torch.arange(n, dtype=torch.float64, device=dev)
    noise = (torch.log(rank + 2) - torch.log(rank + 1)).float()
    opt = torch.optim.Adam(params + [ctx_w], lr=lr)
    n_pairs = center.numel()
    losses = []
    for _ in range(epochs):
        perm = torch.randperm(n_pairs, generator=gen, device=dev)
        total = torch.zeros((), dtype=torch.float64, device=dev)
        for lo in range(0, n_pairs, batch_size):
            pick = perm[lo:lo + batch_size]
            x, y, t = center[pick], context[pick], layer[pick]
            negs = torch.multinomial(noise, negative * x.numel(), replacement=True, generator=gen).view(-1, negative)
            opt.zero_grad(set_to_none=True)
            embs = multiplex_embed(*params, neigh32, x, t, check=False)  # (every id comes from this function's own tables)
            scores = sampled_scores(embs, ctx_w, torch.cat([y.unsqueeze(1), negs], dim=1), "dot", check=False)
            logsig = torch.nn.functional.logsigmoid
            loss = -(logsig(scores[:, 0]) + logsig(-scores[:, 1:]).sum(1)).mean()
            loss.backward()
            opt.step()
            total += loss.detach().double() * x.numel()
        losses.append(float(total / max(n_pairs, 1)))
    with torch.no_grad():
        every = torch.arange(n, device=dev).repeat(t_count)
        kinds = torch.repeat_interleave(torch.arange(t_count, device=dev), n)
        emb = multiplex_embed(*params, neigh32, every, kinds, check=False).view(t_count, n, dim)
    return (emb, nodes, losses) if return_loss else (emb, nodes)


def undirected_edges(row, col, num_nodes, weight=None):
    """The undirected edge table of (row, col) on their device -> (edges int64 [M, 2] with edges[:, 0] <= edges[:, 1], weight
    float64 [M] or None): one entry per unordered pair, pairs ascending.  Where a pair repeats, the weight of its last
    occurrence wins, as networkx's add_weighted_edges_from overwrites (Graph.to_networkx, cogdl/data/data.py:424-437)."""
    row, col = torch.as_tensor(row).long().flatten(), torch.as_tensor(col).long().flatten()
    lo, hi = torch.minimum(row, col), torch.maximum(row, col)
    pairs, inverse = torch.unique(lo * num_nodes + hi, return_inverse=True)
    edges = torch.stack([pairs // num_nodes, pairs % num_nodes], dim=1).contiguous()
    if weight is None:
        return edges, None
    last = torch.zeros(pairs.numel(), dtype=torch.long, device=pairs.device)
    last.scatter_reduce_(0, inverse, torch.arange(row.numel(), device=pairs.device), "amax", include_self=False)
    return edges, torch.as_tensor(weight).to(pairs.device).double().flatten()[last]


def _unit_rows(x):
    norm = x.norm(dim=1, keepdim=True)
    return torch.where(norm > 0, x / norm.clamp_min(1e-30), torch.zeros_like(x))


def line_from_edges(edges, num_nodes, edge_weight=None, dim=128, samples=0, negative=5, alpha=0.025, order=3, seed=None, workers=0):
    """LINE on an undirected edge table (int64 [M, 2], optional weights [M]) -> float32 [num_nodes, width], rows
    L2-normalised (a zero row stays zero, as sklearn.preprocessing.normalize leaves it): width = dim for orders 1 and 2; order
    3 trains order 1 and then order 2 at dim // 2 each and puts the two normalised halves side by side, width 2 * (dim // 2)."""
    from .operators.line import line_train

    order, dim = int(order), int(dim)
    if order not in (1, 2, 3):
        raise ValueError("line: order must be 1, 2 or 3 (got %d)" % order)
    if order == 3 and dim < 2:
        raise ValueError("line: order 3 needs dim >= 2 (got %d)" % dim)
    seed = _seed(seed)
    width = dim // 2 if order == 3 else dim
    halves = []
    for k, o in enumerate((1, 2) if order == 3 else (order,)):
        out = line_train(edges, num_nodes, width, o, samples, negative=negative, alpha=alpha, edge_weight=edge_weight,
                         seed=(seed + k) & (2 ** 64 - 1), workers=workers)
        halves.append(_unit_rows(out if o == 1 else out[0]))
    return halves[0] if len(halves) == 1 else torch.cat(halves, dim=1)


def line(graph_or_csr, dim=128, walk_length=80, walk_num=20, negative=5, alpha=0.025, order=3, seed=None, edge_weight=None,
         workers=0):
    """LINE: walk_length * walk_num * N edge samples per order, each an edge drawn in proportion to its weight, oriented by a
    fair coin, with `negative` negatives drawn in proportion to (weighted degree)^0.75 (cogdl_amd/operators/line.py).  The
    graph is taken as undirected: one edge per unordered pair of the structure; `edge_weight` ([E], in the order of the CSR's
    entries) gives a pair the weight of its last entry.  -> float32 [N, dim] on the graph's device, [N, 2 * (dim // 2)] for
    order 3."""
    indptr, indices = _csr(graph_or_csr)
    n = indptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
    edges, weight = undirected_edges(row, indices, n, edge_weight)
    return line_from_edges(edges, n, weight, dim=dim, samples=int(walk_length) * int(walk_num) * n, negative=negative, alpha=alpha,
                           order=order, seed=seed, workers=workers)
