"""cogdl_amd.operators -- same module layout and exported names as cogdl/operators/.

    spmm.py          csrspmm, spmm_cpu                      (cogdl/operators/spmm.py)
    edge_softmax.py  csr_edge_softmax                       (cogdl/operators/edge_softmax.py)
    mhspmm.py        csrmhspmm                              (cogdl/operators/mhspmm.py)
    scatter_max.py   scatter_max                            (cogdl/operators/scatter_max.py)
    fused_gat.py     fused_gat_func                         (cogdl/operators/fused_gat.py)
    sample.py        sample_adj_c, subgraph_c, coo2csr_cpu, coo2csr_cpu_index  (cogdl/operators/sample.py)

    walk.py          random_walk, node2vec_walk (also exported here)   (cogdl/utils/sampling.py, models/emb/node2vec.py)
                     typed_rows, metapath_walk (also exported here)    (models/emb/metapath2vec.py:87-125)
    ppr.py           topk_ppr, full_ppr (also exported here)           (cogdl/utils/ppr_utils.py)
    sgns.py          skipgram (also exported here)                     (gensim's Word2Vec(sg=1) in models/emb/deepwalk.py)
    readout.py       segment_ptr, segment_pool, sort_pool (also exported here)   (cogdl/utils/utils.py batch_*_pooling,
                                                                                  models/nn/gin.py, models/nn/sortpool.py)

    relational.py    rel_gspmm (also exported here)                    (CompGCNLayer.message_passing, models/nn/compgcn.py)

    genaggr.py       gen_aggregate (also exported here)                (GENConv.forward, layers/deepergcn_layer.py:67-93)

    disen.py         disen_route, neighbor_routing (also exported here)  (DisenGCNLayer.forward, layers/disengcn_layer.py:48-69)

    contrast.py      pair_lse, grace_loss (also exported here)         (GRACEModelWrapper.contrastive_loss,
                                                                        wrappers/model_wrapper/node_classification/grace_mw.py:64-77)

    netsmf.py        path_pairs, path_counts, sparsifier, randomized_svd (also exported here)   (models/emb/netsmf.py)

    spectral.py      filter_step, bessel_i, spectral_filter (also exported here)   (cogdl/utils/prone_utils.py:26-176,
                                                                                    ProNE._chebyshev_gaussian, models/emb/prone.py)

    kgrank.py        rank_all, ranks (also exported here)              (TripleModelWrapper.eval_step,
                                                                        wrappers/model_wrapper/link_prediction/triple_link_prediction_mw.py:84-132;
                                                                        cal_mrr, cogdl/utils/link_prediction_utils.py:8-28)

    kgscore.py       sampled_scores (also exported here)               (KGEModel.forward, models/emb/knowledge_base.py:52-101)

    kgsample.py      negative_batch (also exported here)               (TrainDataset.__getitem__ / collate_fn,
                                                                        cogdl/datasets/kg_data.py:98-135)

    wl.py            wl_labels (also exported here)                    (Graph2Vec.wl_iterations, models/emb/graph2vec.py:63-78)
    pvdbow.py        doc2vec_dbow (also exported here)                 (gensim's Doc2Vec(dm=0) in models/emb/graph2vec.py:99-109)
    line.py          line_train (also exported here)                   (LINE._train_line, models/emb/line.py:127-158)

    multiplex.py     multiplex_embed (also exported here)              (GATNEModel.forward, models/emb/gatne.py:221-241)

    actq.py          quantize, dequantize, relu_packed, dropout_regen, linear_q (also exported here)
                                                                       (actnn.ops / actnn.layers as the reference uses them:
                                                                        operators/linear.py, operators/spmm.py:89-133,
                                                                        layers/act*_layer.py)

    ops.py           scatter_add, op_aggr, s_*_e_sum / s_*_e_mean (fused HIP), s_*_e, s_*_t   (cogdl/operators/ops.py)

Submodules are imported lazily: GPU modules load libcogdl_hip.so at import and raise if it
is missing; `sample` only needs libcogdl_host.so and is safe in forked CPU workers.
"""


def __getattr__(name):
    if name in ("random_walk", "node2vec_walk", "typed_rows", "metapath_walk"):
        from . import walk

        return getattr(walk, name)
    if name in ("topk_ppr", "full_ppr"):
        from . import ppr

        return getattr(ppr, name)
    if name == "skipgram":
        from . import sgns

        return sgns.skipgram
    if name in ("segment_ptr", "segment_pool", "sort_pool"):
        from . import readout

        return getattr(readout, name)
    if name == "rel_gspmm":
        from . import relational

        return relational.rel_gspmm
    if name == "gen_aggregate":
        from . import genaggr

        return genaggr.gen_aggregate
    if name in ("disen_route", "neighbor_routing"):
        from . import disen

        return getattr(disen, name)
    if name in ("pair_lse", "grace_loss"):
        from . import contrast

        return getattr(contrast, name)
    if name in ("path_pairs", "path_counts", "sparsifier", "randomized_svd"):
        from . import netsmf

        return getattr(netsmf, name)
    if name in ("filter_step", "bessel_i", "spectral_filter"):
        from . import spectral

        return getattr(spectral, name)
    if name in ("rank_all", "ranks"):
        from . import kgrank

        return getattr(kgrank, name)
    if name == "sampled_scores":
        from . import kgscore

        return kgscore.sampled_scores
    if name == "negative_batch":
        from . import kgsample

        return kgsample.negative_batch
    if name == "wl_labels":
        from . import wl

        return wl.wl_labels
    if name == "doc2vec_dbow":
        from . import pvdbow

        return pvdbow.doc2vec_dbow
    if name == "line_train":
        from . import line

        return line.line_train
    if name == "multiplex_embed":
        from . import multiplex

        return multiplex.multiplex_embed
    if name in ("quantize", "dequantize", "relu_packed", "dropout_regen", "linear_q", "Quantized"):
        from . import actq

        return getattr(actq, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
