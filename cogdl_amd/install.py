"""Hook the HIP operators underneath an unmodified CogDL.

CogDL resolves its native operators by importing `cogdl.operators.<op>` lazily
(cogdl/utils/spmm_utils.py:21-40,137-146,241-248; cogdl/layers/sage_layer.py:22-25;
cogdl/data/data.py:18; cogdl/utils/graph_utils.py:7).  `install()` registers a meta-path finder
that serves those module names from `cogdl_amd.operators.<op>`, so GCNLayer / GATLayer /
SAGELayer and Graph pick the new path up without any source change.  Call it before
`import cogdl` (modules CogDL already imported are also rebound, and the dispatcher's CONFIGS
registry is reset so that it re-reads the names).

The alternative, equivalent integration is to replace each cogdl/operators/<op>.py by a
one-line shim (`from cogdl_amd.operators.<op> import *`) -- see INTEGRATION.md.
"""
import importlib
import importlib.abc
import importlib.util
import sys

from . import _rebind

REPLACED = ("spmm", "edge_softmax", "mhspmm", "scatter_max", "fused_gat", "sample", "ops")
_PREFIX = "cogdl.operators."


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path=None, target=None):
        if fullname.startswith(_PREFIX) and fullname[len(_PREFIX):] in REPLACED:
            return importlib.util.spec_from_loader(fullname, self)
        return None

    def create_module(self, spec):
        return importlib.import_module("cogdl_amd.operators." + spec.name[len(_PREFIX):])

    def exec_module(self, module):
        pass


_finder = None


def install(linear=False, fused_gat=True, fused_norm=False, narrow_side=False, fused_gat_dropout=False, structure_memo=False,
            metis=False, big_graphs=False, torch_sparse=False, random_walk=False, ppr=False, skipgram=False, readout=False,
            relational=False, genconv=False, disengcn=False, contrast=False, netsmf=False, metapath=False, prone=False,
            kg_eval=False, kg_train=False, graph2vec=False, kg_sample=False, gatne=False, actnn=False, line=False):
    """Idempotent.  Returns the list of cogdl module names that are now served by cogdl_amd.
    fused_norm=True rebinds the dispatcher function `cogdl.utils.spmm_utils.spmm` itself (opt-in: that is no longer the
    unchanged dispatcher) to cogdl_amd.fused.spmm, which folds `out_norm * x` / `in_norm * x` into the kernel.
    fused_gat=True (default) also runs the dispatcher's own `initialize_fused_gat()` (utils/spmm_utils.py:241-248)
    once cogdl is imported and a GPU is present: nothing in the reference ever calls it, so GATLayer's fused branch
    (`check_fused_gat()`, layers/gat_layer.py:68) would otherwise stay dead even with a working fused operator.
    narrow_side=True rebinds GCNLayer.forward (opt-in, like fused_norm: no longer the unchanged layer) to
    cogdl_amd.fused's version, which aggregates at the input width where a layer widens ((A X) W instead of A (X W)).
    fused_gat_dropout=True rebinds GATLayer.forward (opt-in, same caveat) so that the branch the gat model takes by
    default -- attn_drop 0.5: leaky_relu(h_l[row] + h_r[col]) -> edge_softmax -> nn.Dropout -> mhspmm,
    layers/gat_layer.py:72-77 -- is one fused operator with the dropout mask regenerated from a seed (cogdl_amd/fused.py).
    `import cogdl` (or cogdl.layers) must have happened before; call install() again afterwards otherwise.
    structure_memo=True rebinds the two properties Graph.row_indptr / Graph.col_indices (opt-in, same caveat) so that the
    `.int()` copies the dispatcher makes on every call, and the content hash this library takes of them, happen once per
    structure (cogdl_amd/structure_memo.py).
    big_graphs=True rebinds the dispatcher function `spmm` (opt-in, like fused_norm) to cogdl_amd.big_dispatch's front: GPU
    graphs of 2^31 edges and more keep their int64 row pointer on the way to csrspmm (the reference's `.int()` wraps there).
    metis=True registers cogdl_amd.metis_compat as the module `metis` when the real package cannot be imported, so that
    ClusteredDataset / ClusteredLoader (cogdl/data/sampler.py:188-262) partition on the GPU instead of exiting.
    torch_sparse=True registers cogdl_amd.torch_sparse_compat as the module `torch_sparse` when the real package cannot be
    imported, so that the models that call torch_sparse.spspmm / spmm (srgcn, graph_unet, gtn) import and run: the sparse x
    sparse product on the HIP SpGEMM (cogdl_amd.operators.spgemm), spmm on the COO message operator.
    random_walk=True rebinds the name `RandomWalker` in cogdl.utils.sampling, cogdl.utils, cogdl.data.data and
    cogdl.data.sampler (opt-in: the walks then come from a different generator than the reference's) to
    cogdl_amd.random_walk_compat.RandomWalker: Graph.random_walk / random_walk_with_restart and the unsupervised sampler's
    positive pairs run on the library's walk operators (HIP kernels for a graph on the GPU, the OpenMP host twin otherwise)
    instead of the reference's numba / interpreted Python loop.
    ppr=True rebinds `ppr_topk`, `topk_ppr_matrix` and `build_topk_ppr_matrix_from_data` in cogdl.utils.ppr_utils and the
    by-name copies in cogdl.wrappers.data_wrapper.node_classification.pprgo_dw and cogdl.models.nn.mvgrl (opt-in: the scores
    are those of a deterministic push order, within eps * deg of the reference's) to cogdl_amd.ppr_compat: the top-k PPR
    matrix of pprgo and mvgrl comes from the library's PPR operator (HIP kernel when a GPU is visible, the OpenMP host twin
    otherwise).  Where cogdl.utils.ppr_utils cannot be imported (numba missing), cogdl_amd.ppr_compat is registered under
    that name, so the two models import at all.
    skipgram=True registers cogdl_amd.gensim_compat as the module `gensim` (with gensim.models, gensim.models.word2vec and
    gensim.models.keyedvectors) when the real package cannot be imported, so that the embedding models that train through
    gensim.models.Word2Vec (deepwalk, node2vec, metapath2vec, dgk) import and train on the library's skip-gram operator, and
    rebinds DeepWalk.forward and Node2vec.forward (opt-in: the draws are Philox's, not numpy's and gensim's generators, and
    at a node without out-neighbours the walker stays instead of ending the walk) to versions that walk and train on the
    graph's device through cogdl_amd.embedding, with the same return value (features_matrix as numpy [N, dim], or the dict
    with return_dict=True).
    readout=True rebinds `batch_sum_pooling`, `batch_mean_pooling` and `batch_max_pooling` in cogdl.utils.utils and the by-name
    copies in cogdl.utils, cogdl.models.nn.gcc_model, cogdl.models.nn.infograph, cogdl.layers.deepergcn_layer and
    cogdl.layers.set2set, and rebinds GIN.forward and SortPool.forward (opt-in: no longer the unchanged models) to
    cogdl_amd.readout_compat: the graph readout runs on the library's segment reduction and top-k operators (HIP kernels for
    CUDA tensors, the OpenMP host twin otherwise) instead of zeros + scatter_add_, a CSR built per call, or SortPool's dense
    pad + sort + gather.  No float atomics: sums are equal from run to run, and equal to the reference's CPU sums bit for bit;
    max pooling also runs on the CPU without torch_scatter; equal SortPool keys go in row order.  A batch vector that is
    unsorted or empty, an x that is not 2-D float32, and a mean over absent graph ids go to the reference's own functions.
    relational=True rebinds CompGCNLayer.message_passing in cogdl.models.nn.compgcn (opt-in: no longer the unchanged layer, and
    the sums are re-associated -- float32 rounding apart, the same numbers) to cogdl_amd.relational_compat: the typed message
    passing of the compgcn link-prediction model is one relational aggregation to [N, in] on the library's rel_gspmm operator
    (HIP kernels for CUDA tensors: no [E, in] / [E, out] message tensors, no float atomics, equal from run to run; the torch
    composition on the CPU) followed by one [N, in] x [in, out] matmul, instead of a matmul per edge and scatter_add_.  `opn`
    "sub" and "mult" are served, any other reaches the reference's method.  The reference's RGCNLayer is not served
    (INTEGRATION.md).
    genconv=True rebinds GENConv.forward in cogdl.layers.deepergcn_layer (opt-in: no longer the unchanged layer, and the softmax
    sums are re-associated -- float32 rounding apart, the same numbers) to cogdl_amd.genconv_compat: the aggregation of the
    deepergcn and revgcn models (gather, edge encoder term, relu + eps, beta, per-column edge softmax, multiply, scatter_add_)
    is one call of the library's gen_aggregate operator (HIP kernels for CUDA tensors: no [E, F] message tensors, no float
    atomics, equal from run to run; the torch composition on the CPU).  `softmax_sg`, `softmax`, `mean` and the plain sum are
    served; `powermean`, `max`, a graph without a CSR and a graph whose CSR does not describe its edge_index reach the
    reference's forward.
    disengcn=True rebinds DisenGCNLayer.forward in cogdl.layers.disengcn_layer (opt-in: no longer the unchanged layer, and the
    softmax sums are re-associated -- float32 rounding apart, the same numbers) to cogdl_amd.disengcn_compat: the channel
    normalisation and the routing loop of the disengcn model (per iteration three [E, K, d] gathers, a K-head edge softmax, an
    int64 [K, E, d] index and scatter_add_) are one call of the library's neighbor_routing (per iteration one disen_route
    operator; HIP kernels for CUDA tensors with d in {2, .., 64}: nothing of size [E, .] is written, no float atomics, equal
    from run to run; the torch composition on the CPU).  A graph without a CSR, a graph whose CSR does not describe its
    edge_index, an x that is not 2-D and an out_feats that K does not divide reach the reference's forward.
    contrast=True rebinds GRACEModelWrapper.contrastive_loss in cogdl.wrappers.model_wrapper.node_classification.grace_mw (opt-in:
    no longer the unchanged wrapper, and the row sums are re-associated -- float32 rounding apart, the same numbers) to
    cogdl_amd.contrast_compat: the loss of the grace model is one call of the library's grace_loss (normalisation, then the
    pair_lse operator: a torch composition in row blocks of the queries whose backward recomputes the scores, so neither of
    the two [N, N] score matrices is kept; there is no HIP kernel behind it, GPU tensors run torch's kernels and say so once
    with a TorchRouteWarning).  batched_loss calls the rebound method and is served as it stands.  Inputs that are not 2-D
    float tensors of one width reach the reference's method.
    netsmf=True rebinds NetSMF.forward in cogdl.models.emb.netsmf (opt-in: the draws are Philox's, not numpy's; num_round rounds
    become ceil(num_round / 2) passes over the CSR entries, so an odd num_round is rounded up; a node without edges gets a zero
    row where the reference divides by its degree) to cogdl_amd.netsmf_compat: the simple symmetric structure of edge_index is
    built on the graph's device, the num_round * num_edge * window_size path samples come from the library's path sampler (HIP
    kernel for a graph on the GPU, the OpenMP host twin otherwise) instead of an interpreted loop into a scipy lil_matrix, the
    sparsifier and the randomized SVD run there too (cogdl_amd/operators/netsmf.py), with the same return value
    (features_matrix as numpy [N, dim], or the dict with return_dict=True).  A graph whose edge weights are not all equal and
    a graph without edges reach the reference's forward.
    metapath=True rebinds Metapath2vec.forward in cogdl.models.emb.metapath2vec (opt-in: the draws are Philox's, not `random`'s
    and gensim's; the start order differs; `worker` is ignored) to cogdl_amd.metapath_compat: the DiGraph's CSR is built on the
    device of edge_index, the walk_num x nodes x metapaths walks come from the library's metapath walk (typed row layout, HIP
    kernel for a graph on the GPU, the OpenMP host twin otherwise) instead of an interpreted loop over networkx neighbour
    lists, and the skip-gram operator trains on them; the return value is the reference's (float32 numpy, one row per node
    that occurs in an edge, in networkx insertion order; KeyError for a node that no walk visits).  The reference module
    imports gensim, so where gensim is absent cogdl_amd.gensim_compat is registered first, as skipgram=True does.  A schema
    item that is not an integer, a metapath whose first item differs from its last and a data.pos that is not an integer
    tensor reach the reference's forward.
    prone=True rebinds ProNE.forward in cogdl.models.emb.prone, and `propagate` in cogdl.utils.prone_utils with its by-name copy
    in cogdl.models.emb.pronepp (opt-in: float32 where the reference runs scipy in float64, the library's randomized SVD where
    it runs sklearn's, a zero row of the factorisation for a node without edges) to cogdl_amd.prone_compat: the simple
    symmetric structure of edge_index is built on the graph's device and cogdl_amd.embedding.prone runs there -- the
    pre-factorisation matrix, the randomized SVD, the spectral propagation as one fused filter step per sparse product
    (cogdl_amd/operators/spectral.py: HIP kernel for a graph on the GPU, the OpenMP host twin otherwise) and the dense embedding
    -- with the same return value (features_matrix as numpy [N, dim], or the dict with return_dict=True).  `propagate` keeps
    its signature and runs the heat / ppr / gaussian / prone filters on the GPU when one is visible (the host twin otherwise),
    returning float64 numpy: ProNE++'s search and the `--enhance prone` / `prone++` post-processing inherit it.  A graph whose
    edge weights are not all equal, a graph with self loops, a graph without edges and step == 1 reach the reference's
    forward; the "sc" filter, any other name and a matrix that is not square with unit entries and an empty diagonal reach the
    reference's propagate.
    kg_eval=True rebinds TripleModelWrapper.eval_step in cogdl.wrappers.model_wrapper.link_prediction.triple_link_prediction_mw,
    and `cal_mrr` in cogdl.utils.link_prediction_utils with its by-name copy in
    cogdl.wrappers.model_wrapper.link_prediction.gnn_kg_link_prediction_mw (opt-in: the loaders are read, not iterated; the rank
    of a target that ties with other candidates is 1 + greater + equal_before where the reference's is whatever its sort does)
    to cogdl_amd.kgrank_compat: the filtered evaluation of transe, distmult, complex and rotate and the raw evaluation of compgcn
    and rgcn are counts from the library's rank_all operator (HIP kernels for CUDA tensors -- dot on the fp32 MFMA, the two
    distances on the VALU -- the OpenMP host twin otherwise): no [B, N, D] gather, no [B, N] sort, no read-back per triple; the
    filter lists are built once per dataset with torch sort / unique.  cal_mrr also serves protocol="filtered" when its new
    optional `seen_triples` argument is given.  Any other model class reaches the reference's eval_step, ConvELayer scoring
    the reference's cal_mrr.
    kg_train=True rebinds KGEModel.forward in cogdl.models.emb.knowledge_base (opt-in: no longer the unchanged model, and the sums
    over the embedding width are re-associated -- float32 rounding apart, the same numbers) to cogdl_amd.kgtrain_compat: the two
    forward calls of TripleModelWrapper.train_step for transe, distmult, complex and rotate -- the negative scores [B, K] of a
    head-batch or tail-batch and the positive scores [B, 1] -- are the [B, D] query of cogdl_amd.kgrank.prepare_query in torch
    and one call of the library's sampled_scores operator against the entity table (HIP kernels for CUDA tensors, the OpenMP
    host twin otherwise): no [B, K, D] gather, no elementwise kernels of that size kept for backward, and the gradient of the
    entity table is a sum in a fixed order instead of an atomic scatter, equal from run to run.  The loss, the self-adversarial
    softmax and the regulariser stay the reference's.  Any other model class, a subclass with its own `score` and an unknown
    mode reach the reference's forward.  Not for use under torch.cuda.graph capture.
    graph2vec=True rebinds Graph2Vec.forward in cogdl.models.emb.graph2vec (opt-in: the draws are Philox's, the vocabulary is not
    gensim's, and feature rows are compared as float32 arrays, not as numpy's printed strings) to cogdl_amd.graph2vec_compat: one
    batched CSR of all graphs is built on their device (or on the GPU when one is visible), the WL subtree words come from the
    library's wl_labels operator (HIP kernels for a CSR on the GPU, the host twin otherwise) instead of an md5 per node and round
    over networkx adjacency, and the library's doc2vec_dbow operator trains PV-DBOW on them; the return value is the
    reference's (a numpy array with one row per graph).  The reference module imports gensim.models.doc2vec, so where gensim is
    absent cogdl_amd.gensim_compat is registered first, as metapath=True does.  A dm that selects PV-DM, an x that is not a
    numeric tensor, an empty list and a node over wl_labels' degree cap reach the reference's forward.
    kg_sample=True rebinds TripleDataWrapper.train_wrapper in
    cogdl.wrappers.data_wrapper.link_prediction.triple_link_prediction_dw (opt-in: the negatives are drawn by this library's
    Philox law, csrc/kgsample_law.h, seeded with torch.initial_seed(), not by numpy's global generator -- the distribution is the
    same, uniform with repetition over the entities that are not true for the positive, and the numbers are not) to
    cogdl_amd.kgsample_compat: the iterator the trainer hands to TripleModelWrapper.train_step is cogdl_amd.kgsample.TrainBatches
    instead of BidirectionalOneShotIterator over two DataLoaders.  The true-head and true-tail lists and the subsampling weights
    (bit-equal to the reference's) are flat tables built once with torch sort / unique on the triples' device, and every batch --
    positive int64 [b, 3], negative int64 [b, K], subsampling_weight float32 [b], mode, "tail-batch" first -- is one launch of
    the library's negative_batch operator on the training device (HIP kernel for tables on the GPU, the OpenMP host twin
    otherwise) without a rejection loop, a collate or a host-to-device copy.  A dataset without `triples`, `train_start_idx`,
    `valid_start_idx` and `_num_entities` reaches the reference's method.
    line=True rebinds LINE.forward in cogdl.models.emb.line (opt-in: the update is the original LINE program's, not the
    reference's -- the reference's `_update` changes fancy-indexed copies, so it never updates a target or context row and its
    orders 1 and 2 are one computation; here target rows are updated and the order-2 context table starts at zero -- the draws
    are Philox's by inverse CDF, not numpy's through alias tables, the learning rate changes with every sample, a negative
    equal to either endpoint is skipped, `batch_size` is ignored, `self.dimension` is not halved by a call with order 3, and
    weighted degrees stay float64) to cogdl_amd.line_compat: the undirected edge table networkx would hold is built on the
    graph's device with torch sort / unique, and the walk_length * walk_num * N samples per order run on the library's
    line_train operator (HIP kernel for a graph on the GPU, the OpenMP host twin otherwise) instead of an interpreted
    alias_draw per edge and per negative; the return value is the reference's (float64 numpy [N, width] with L2-normalised
    rows, or the dict with return_dict=True).  Edge weights that are not all finite and positive, a graph without edges, an
    order outside {1, 2, 3} and dimension < 2 with order 3 reach the reference's forward.
    gatne=True rebinds GATNE.forward in cogdl.models.emb.gatne (opt-in: the draws are Philox's and torch's, not `random`'s and
    numpy's; ties in the vocabulary order go in ascending node id where the reference keeps first appearance; a trailing batch
    of one pair and a network of one edge type train here, where the reference's module raises; `worker` is ignored) to
    cogdl_amd.gatne_compat: cogdl_amd.embedding.gatne builds the layers' graphs, walks them with the library's random_walk,
    slices the pairs, draws the [N, T, S] neighbour table once and trains with one multiplex_embed and one sampled_scores call
    per step (HIP kernels for CUDA tensors: the model step is one forward launch without the reference's [B, T, S, T, U] gather,
    and no gradient uses a float atomic; the torch composition and the host twins on the CPU) under torch.optim.Adam(lr=1e-4);
    the final embeddings are one batched call.  The return value is the reference's ({edge type: {node id: float32 numpy
    [dimension]}}).  The reference module imports gensim.models.keyedvectors.Vocab, so where gensim is absent
    cogdl_amd.gensim_compat is registered first, as metapath=True does.  A schema other than None, an empty network_data, a
    layer without edges and node ids that are not non-negative integers reach the reference's forward.
    actnn=True registers cogdl_amd.actnn_compat as `actnn` (with actnn.ops, actnn.conf, actnn.qscheme, actnn.layers and
    actnn.utils) where the real package cannot be imported, as metis=True does for metis: the reference's `--actnn` family --
    the actgcn model, graphsage / gcnii with actnn=True, cogdl/operators/linear.py with its random projection,
    cogdl/layers/act*_layer.py and Trainer(actnn=True) -- imports and trains.  What a layer saves for its backward pass is
    held by the library's activation-compression operators (cogdl_amd/operators/actq.py; HIP kernels for CUDA tensors, the
    OpenMP host twin otherwise): the input of a QLinear, of a QBatchNorm1d and of csrspmm(actnn=True) in 2 bits per element
    (config.activation_compression_bits), the state of a QReLU in one bit per element, and a QDropout saves nothing -- its
    mask is regenerated from a counter.  This is not ActNN's arithmetic (INTEGRATION.md lists every deviation): groups of
    the flattened tensor, float32 (min, step) pairs, Philox draws keyed by torch.initial_seed(), float32 compute only, and
    the optimisation levels L3 and above are served as L2 with one warning.  A training step that uses it must not be
    captured in a graph (a replay would repeat one noise draw).
    linear=True additionally routes torch.nn.functional.linear -- i.e. the unchanged nn.Linear inside every CogDL
    layer -- through cogdl_amd.linear (hand-written MFMA weight gradient for full-graph shapes)."""
    global _finder
    if _finder is None:
        _finder = _Finder()
        sys.meta_path.insert(0, _finder)
    for op in REPLACED:
        name = _PREFIX + op
        if name in sys.modules and not getattr(sys.modules[name], "__name__", "").startswith("cogdl_amd."):
            mod = importlib.import_module("cogdl_amd.operators." + op)
            _rebind.put("operators", sys.modules, name, mod)
            pkg = sys.modules.get("cogdl.operators")
            if pkg is not None:
                _rebind.put("operators", pkg, op, mod)
                if op == "ops":  # cogdl/operators/__init__.py:1-16 re-exports the s_* names from .ops
                    for attr in dir(mod):
                        if attr.startswith("s_") and hasattr(pkg, attr):
                            _rebind.put("operators", pkg, attr, getattr(mod, attr))
    _rebind_graph_build()
    if linear:
        from . import linear as _linear

        _linear.install()
    if fused_norm:
        from . import fused as _fused

        _fused.install()
    if narrow_side:
        from . import fused as _fused

        _fused.install_narrow_side()
    if fused_gat_dropout:
        from . import fused as _fused

        _import_target("cogdl.layers.gat_layer", "fused_gat_dropout")  # (the finder above already serves cogdl.operators.*)
        if not _fused.install_gat_dropout():
            raise _lib_error("install(fused_gat_dropout=True): GATLayer.forward could not be rebound")
    if big_graphs:
        from . import big_dispatch as _big

        _import_target("cogdl.utils.spmm_utils", "big_graphs")
        if not _big.install():
            raise _lib_error("install(big_graphs=True): cogdl.utils.spmm_utils.spmm could not be rebound")
    if structure_memo:
        from . import structure_memo as _memo

        _import_target("cogdl.data.data", "structure_memo")
        if not _memo.install():
            raise _lib_error("install(structure_memo=True): Graph.row_indptr / col_indices could not be rebound")
    if metis:
        _serve_where_absent("metis")
    if torch_sparse:
        _serve_where_absent("torch_sparse")
    if actnn:
        from . import actnn_compat

        _serve_where_absent("actnn")
        actnn_compat.register(_rebind)
    if random_walk:
        _rebind_random_walker()
    if ppr:
        _rebind_ppr()
    if skipgram:
        _install_skipgram()
    if readout:
        _rebind_readout()
    if relational:
        from . import relational_compat

        _import_target("cogdl.models.nn.compgcn", "relational")
        if not relational_compat.install():
            raise _lib_error("install(relational=True): CompGCNLayer.message_passing could not be rebound")
    if genconv:
        from . import genconv_compat

        _import_target("cogdl.layers.deepergcn_layer", "genconv")
        if not genconv_compat.install():
            raise _lib_error("install(genconv=True): GENConv.forward could not be rebound")
    if disengcn:
        from . import disengcn_compat

        _import_target("cogdl.layers.disengcn_layer", "disengcn")
        if not disengcn_compat.install():
            raise _lib_error("install(disengcn=True): DisenGCNLayer.forward could not be rebound")
    if contrast:
        from . import contrast_compat

        _import_target(contrast_compat._MODULE, "contrast")
        if not contrast_compat.install():
            raise _lib_error("install(contrast=True): GRACEModelWrapper.contrastive_loss could not be rebound")
    if netsmf:
        from . import netsmf_compat

        _import_target(netsmf_compat._MODULE, "netsmf")
        if not netsmf_compat.install():
            raise _lib_error("install(netsmf=True): NetSMF.forward could not be rebound")
    if metapath:
        from . import metapath_compat

        _serve_gensim_where_absent()  # (cogdl.models.emb.metapath2vec imports gensim)
        _import_target(metapath_compat._MODULE, "metapath")
        if not metapath_compat.install():
            raise _lib_error("install(metapath=True): Metapath2vec.forward could not be rebound")
    if prone:
        from . import prone_compat

        _import_target(prone_compat._MODULE, "prone")
        _import_target(prone_compat._UTILS, "prone")
        try:  # (the module that copied `propagate` by name; it needs optuna, and is rebound where it imports)
            importlib.import_module(prone_compat._HOLDER)
        except ImportError:
            pass
        if not prone_compat.install():
            raise _lib_error("install(prone=True): ProNE.forward / propagate could not be rebound")
    if kg_eval:
        from . import kgrank_compat

        for name in (kgrank_compat._UTILS, kgrank_compat._WRAPPER, kgrank_compat._HOLDER) + tuple(m for _, m, _ in kgrank_compat._MODELS):
            _import_target(name, "kg_eval")  # (before anything is rebound: the holder copies the name it gets back at uninstall())
        if not kgrank_compat.install():
            raise _lib_error("install(kg_eval=True): TripleModelWrapper.eval_step / cal_mrr could not be rebound")
    if kg_train:
        from . import kgtrain_compat

        for name in (kgtrain_compat._MODULE,) + tuple(m for _, m, _ in kgtrain_compat._MODELS):
            _import_target(name, "kg_train")
        if not kgtrain_compat.install():
            raise _lib_error("install(kg_train=True): KGEModel.forward could not be rebound")
    if graph2vec:
        from . import graph2vec_compat

        _serve_gensim_where_absent()  # (cogdl.models.emb.graph2vec imports gensim.models.doc2vec)
        _import_target(graph2vec_compat._MODULE, "graph2vec")
        if not graph2vec_compat.install():
            raise _lib_error("install(graph2vec=True): Graph2Vec.forward could not be rebound")
    if kg_sample:
        from . import kgsample_compat

        _import_target(kgsample_compat._MODULE, "kg_sample")
        if not kgsample_compat.install():
            raise _lib_error("install(kg_sample=True): TripleDataWrapper.train_wrapper could not be rebound")
    if line:
        from . import line_compat

        _import_target(line_compat._MODULE, "line")
        if not line_compat.install():
            raise _lib_error("install(line=True): LINE.forward could not be rebound")
    if gatne:
        from . import gatne_compat

        _serve_gensim_where_absent()  # (cogdl.models.emb.gatne imports gensim.models.keyedvectors.Vocab)
        _import_target(gatne_compat._MODULE, "gatne")
        if not gatne_compat.install():
            raise _lib_error("install(gatne=True): GATNE.forward could not be rebound")
    su =sys.modules.get("cogdl.utils.spmm_utils")
    if su is not None:  # force the dispatcher to re-resolve the callables
        for k in ("spmm_flag", "mh_spmm_flag", "fused_gat_flag", "spmm_cpu_flag"):
            su.CONFIGS[k] = False
        for k in ("fast_spmm", "csrmhspmm", "csr_edge_softmax", "fused_gat_func", "fast_spmm_cpu"):
            su.CONFIGS[k] = None
        if fused_gat:
            import torch

            if torch.cuda.is_available():
                su.initialize_fused_gat()
    return [_PREFIX + op for op in REPLACED]


def uninstall():
    """Revert every recorded rebind, newest first (cogdl_amd/_rebind.py), then drop the finder and what it served."""
    _rebind.undo()
    global _finder
    if _finder is not None:
        sys.meta_path.remove(_finder)
        _finder = None
    for op in REPLACED:
        mod = sys.modules.get(_PREFIX + op)
        if mod is not None and getattr(mod, "__name__", "").startswith("cogdl_amd."):
            del sys.modules[_PREFIX + op]


def _lib_error(msg):
    from ._lib import BackendError

    return BackendError(msg)


def _import_target(name, flag):
    """The opt-in rebinds patch a cogdl module: import it now (install() may be called before `import cogdl`) instead of
    silently doing nothing; an installation without cogdl gets an error naming the flag, not the slow path."""
    try:
        importlib.import_module(name)
    except ImportError as e:
        raise _lib_error("install(%s=True) needs the cogdl package (importing %s failed: %s)" % (flag, name, e)) from e


def _serve_where_absent(name):
    """Register cogdl_amd.<name>_compat as the module `name` unless that name is taken or the real package imports."""
    if name not in sys.modules:
        try:
            importlib.import_module(name)  # the real one wins where it exists
        except Exception:  # (ImportError, or the metis wrapper's RuntimeError when libmetis is missing)
            _rebind.put(name, sys.modules, name, importlib.import_module("cogdl_amd.%s_compat" % name))


_GRAPH_BUILD_NAMES = ("coo2csr_index", "add_remaining_self_loops", "symmetric_normalization", "row_normalization")


def _rebind_graph_build():
    """CSR construction, self loops and normalisation stay on the GPU (cogdl_amd/graph_build.py; CPU
    tensors keep the reference's arithmetic).  Every cogdl module that holds one of the helpers by name is rebound
    (`from cogdl.utils import ...` copies the reference); effective for the modules already imported -- call install()
    again after `import cogdl` if it ran before (install() is idempotent)."""
    from . import graph_build

    for fn in _GRAPH_BUILD_NAMES:
        _rebind.put_where_held("graph_build", fn, getattr(graph_build, fn),
                               lambda cur: getattr(cur, "__module__", "") == "cogdl.utils.graph_utils")


_RANDOM_WALKER_MODULES = ("cogdl.utils.sampling", "cogdl.utils", "cogdl.data.data", "cogdl.data.sampler")


def _rebind_random_walker():
    """The four modules that hold the reference's RandomWalker by name (`from cogdl.utils import RandomWalker` copies it) are
    imported if need be and rebound."""
    from .random_walk_compat import RandomWalker

    for name in _RANDOM_WALKER_MODULES:
        _import_target(name, "random_walk")
        if getattr(sys.modules[name], "RandomWalker", None) is None:
            raise _lib_error("install(random_walk=True): %s has no RandomWalker to rebind" % name)
        _rebind.put("random_walk", sys.modules[name], "RandomWalker", RandomWalker)


_PPR_NAMES = ("ppr_topk", "topk_ppr_matrix", "build_topk_ppr_matrix_from_data")
_PPR_UTILS = "cogdl.utils.ppr_utils"
_PPR_HOLDERS = ("cogdl.wrappers.data_wrapper.node_classification.pprgo_dw", "cogdl.models.nn.mvgrl")


def _rebind_ppr():
    """cogdl.utils.ppr_utils is imported (or, where numba is missing, served by cogdl_amd.ppr_compat under that name), then
    the three functions are rebound there and in the two modules that copied one by name."""
    from . import ppr_compat

    _import_target("cogdl.utils", "ppr")
    try:
        importlib.import_module(_PPR_UTILS)
    except ImportError:  # numba missing: the reference module cannot load
        _rebind.put("ppr", sys.modules, _PPR_UTILS, ppr_compat)
        _rebind.put("ppr", sys.modules["cogdl.utils"], "ppr_utils", ppr_compat)
    for name in _PPR_HOLDERS:  # (before anything is rebound: they copy the names they will get back at uninstall())
        _import_target(name, "ppr")
    for name in (_PPR_UTILS,) + _PPR_HOLDERS:
        mod = sys.modules[name]
        if mod is ppr_compat:
            continue
        for fn in _PPR_NAMES:
            if getattr(mod, fn, None) is not None:
                _rebind.put("ppr", mod, fn, getattr(ppr_compat, fn))


_READOUT_NAMES = ("batch_sum_pooling", "batch_mean_pooling", "batch_max_pooling")
_READOUT_HOLDERS = ("cogdl.utils.utils", "cogdl.utils", "cogdl.models.nn.gcc_model", "cogdl.models.nn.infograph",
                    "cogdl.layers.deepergcn_layer", "cogdl.layers.set2set")
_READOUT_MODELS = (("cogdl.models.nn.gin", "GIN", "gin_forward"), ("cogdl.models.nn.sortpool", "SortPool", "sortpool_forward"))


def _rebind_readout():
    """The modules that hold a pooling function by name and the two models are imported (before anything is rebound: they
    copy the names they will get back at uninstall()), then every holder of a reference pooling function and the two forward
    methods are rebound."""
    from . import readout_compat

    for name in _READOUT_HOLDERS + tuple(m for m, _, _ in _READOUT_MODELS):
        _import_target(name, "readout")
    for fn in _READOUT_NAMES:
        _rebind.put_where_held("readout", fn, getattr(readout_compat, fn),
                               lambda cur: getattr(cur, "__module__", "") == "cogdl.utils.utils")
    for name, cls_name, fwd in _READOUT_MODELS:
        _rebind.put("readout", getattr(sys.modules[name], cls_name), "forward", getattr(readout_compat, fwd))


_EMB_MODELS = (("cogdl.models.emb.deepwalk", "DeepWalk"), ("cogdl.models.emb.node2vec", "Node2vec"))


def _embedding_matrix(model, graph, return_dict, emb):
    import numpy as np

    features_matrix = emb.detach().cpu().numpy().astype(np.float64)
    if return_dict:
        return dict((vid, features_matrix[vid]) for vid in range(graph.num_nodes))
    return features_matrix


def _deepwalk_forward(self, graph, embedding_model_creator=None, return_dict=False):
    from . import embedding

    emb = embedding.deepwalk(graph, dim=self.dimension, walk_length=self.walk_length, walk_num=self.walk_num,
                             window=self.window_size, epochs=self.iteration)
    return _embedding_matrix(self, graph, return_dict, emb)


def _node2vec_forward(self, graph, return_dict=False):
    from . import embedding

    emb = embedding.node2vec(graph, dim=self.dimension, walk_length=self.walk_length, walk_num=self.walk_num,
                             window=self.window_size, epochs=self.iteration, p=self.p, q=self.q)
    return _embedding_matrix(self, graph, return_dict, emb)


def _serve_gensim_where_absent():
    """gensim is served by cogdl_amd.gensim_compat where the real package is absent (the real one wins where it exists)."""
    from . import gensim_compat

    if getattr(sys.modules.get("gensim"), "__name__", None) is None:  # not imported yet (or marked absent)
        try:
            sys.modules.pop("gensim", None)
            importlib.import_module("gensim")
        except Exception:
            gensim_compat.register()


def _install_skipgram():
    """The gensim registration step, then the two models are imported and their forward rebound.  Without the cogdl package
    only the module registration happens."""
    _serve_gensim_where_absent()
    try:
        importlib.import_module("cogdl")
    except ImportError:
        return
    for (name, cls_name), fwd in zip(_EMB_MODELS, (_deepwalk_forward, _node2vec_forward)):
        _import_target(name, "skipgram")
        _rebind.put("skipgram", getattr(sys.modules[name], cls_name), "forward", fwd)

