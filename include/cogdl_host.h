/*
 * cogdl_host.h -- C ABI of libcogdl_host.so: the HIP-free host operators of the message-
 * passing path (CSR construction, neighbour sampling, CPU SpMM).  They run inside forked
 * DataLoader worker processes in CogDL (cogdl/data/sampler.py:82-116), so this library
 * never touches the HIP runtime.  All index arrays are int64 (what cogdl/operators/sample/
 * sample.cpp uses: data_ptr<int64_t>, :8-10).  Return 0 on success, COGDL_HOST_E* otherwise.
 */
#ifndef COGDL_HOST_H
#define COGDL_HOST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#if defined(COGDL_HOST_BUILD)
#define COGDL_HOST_API __attribute__((visibility("default")))
#else
#define COGDL_HOST_API
#endif

enum cogdl_host_status {
    COGDL_HOST_OK = 0,
    COGDL_HOST_EINVAL = 1,   /* null pointer / negative size */
    COGDL_HOST_ERANGE = 2,   /* an index lies outside [0, num_nodes) */
    COGDL_HOST_ECAP = 3      /* caller-provided output capacity too small */
};

COGDL_HOST_API const char *cogdl_host_strerror(int status);

/* coo2csr_cpu(row, col, val, num_nodes) -> (row_ptr, col_ind, out_val)
 * Replaces sampler.coo2csr_cpu (cogdl/operators/sample/sample.cpp:191-231): stable counting
 * sort by row (edges of a row keep their COO order).  val/out_val may be NULL. */
COGDL_HOST_API int cogdl_host_coo2csr(const int64_t *row, const int64_t *col, const float *val, int64_t nnz,
                                      int64_t num_nodes, int64_t *row_ptr, int64_t *col_ind, float *out_val);

/* coo2csr_cpu_index(row, col, num_nodes) -> (row_ptr, perm); perm[j] = COO position of CSR
 * entry j.  Replaces sampler.coo2csr_cpu_index (sample.cpp:234-270).  `row` must be
 * contiguous (the Python binding makes it so; the reference silently mis-reads strided views). */
COGDL_HOST_API int cogdl_host_coo2csr_index(const int64_t *row, int64_t nnz, int64_t num_nodes, int64_t *row_ptr,
                                            int64_t *perm);

/* sample_adj(indptr, indices, node_idx, num_neighbors, replace)
 *   -> (out_indptr[batch+1], out_indices[E'], out_nodes[N'], out_edges[E'])
 * Replaces sampler.sample_adj (sample.cpp:6-144).  Relabelling contract: seeds get ids
 * 0..batch-1 in order, new neighbours get the next id in discovery order (row by row, in
 * the order the row's sampled edges are emitted).
 *   num_neighbors < 0 : all neighbours, deterministic, identical to the reference.
 *   replace != 0      : num_neighbors uniform draws with replacement per seed.
 *   else              : min(deg, num_neighbors) distinct neighbours, uniform without
 *                       replacement (Floyd), emitted in ascending CSR position.
 * Randomness comes from an explicit 64-bit seed (splitmix64/xoshiro256**), NOT libc rand():
 * reproducible, thread- and fork-safe.  Capacities: cap_edges >= sum of per-seed counts,
 * cap_nodes >= batch + cap_edges always suffices.  out_counts = {N', E'}. */
COGDL_HOST_API int cogdl_host_sample_adj(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                                         const int64_t *node_idx, int64_t batch, int64_t num_neighbors,
                                         int replace, uint64_t seed, int64_t *out_indptr, int64_t *out_indices,
                                         int64_t *out_nodes, int64_t *out_edges, int64_t cap_edges,
                                         int64_t cap_nodes, int64_t *out_counts);

/* The same with the picks (two of the three dependent random reads per sampled edge) split over `nthreads` host
 * OpenMP threads (the runtime a torch process already has workers of; nthreads = 1 -- what torch gives DataLoader
 * workers -- never enters a parallel region, so forked workers stay clear of OpenMP); the relabelling in discovery
 * order stays sequential.  Bit-identical results for every nthreads >= 1 (the random stream
 * of a seed row depends on (seed, row) only). */
COGDL_HOST_API int cogdl_host_sample_adj_mt(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                                            const int64_t *node_idx, int64_t batch, int64_t num_neighbors,
                                            int replace, uint64_t seed, int64_t *out_indptr, int64_t *out_indices,
                                            int64_t *out_nodes, int64_t *out_edges, int64_t cap_edges,
                                            int64_t cap_nodes, int64_t *out_counts, int nthreads);

/* subgraph(indptr, indices, node_idx) -> induced subgraph in CSR, relabelled by position in
 * node_idx.  Replaces sampler.subgraph (sample.cpp:146-188).  out_counts = {E'}. */
COGDL_HOST_API int cogdl_host_subgraph(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                                       const int64_t *node_idx, int64_t batch, int64_t *out_indptr,
                                       int64_t *out_indices, int64_t *out_edges, int64_t cap_edges,
                                       int64_t *out_counts);

/* csr_spmm_cpu(rowptr, colind, val, dense) -> out   (CPU tensors; CogDL's CPU inference path)
 * Replaces spmm_cpu.csr_spmm_cpu (cogdl/operators/spmm/spmm_cpu.cpp:6-58): rows in parallel
 * over `nthreads` host threads, each output element accumulated sequentially in CSR order
 * with fp32 multiply then add (bit-identical to the reference).  int32 indices, 64-bit offsets. */
COGDL_HOST_API int cogdl_host_csr_spmm_f32(const int32_t *rowptr, const int32_t *colind, const float *val,
                                           const float *dense, float *out, int64_t m, int64_t k, int nthreads);
/* The same with int64 row pointers: graphs of 2^31 edges and more on the host (the reference's `int key` / `int ik = i * k`
 * loop, spmm_cpu.cpp:24-33, overflows at 2^31 edges and already at 16.7 M rows x 128 columns).  Same arithmetic. */
COGDL_HOST_API int cogdl_host_csr_spmm_f32_i64(const int64_t *rowptr, const int32_t *colind, const float *val,
                                               const float *dense, float *out, int64_t m, int64_t k, int nthreads);

/* Random walks on a CSR graph (int64 indptr[num_nodes + 1], indices[num_edges]), one walker per entry of start[W],
 * written to walks[W, length] row-major; the host twin of cogdl_hip_random_walk / cogdl_hip_node2vec_walk
 * (include/cogdl_hip.h, where the contract is spelled out): same arguments minus the stream, and for equal inputs and
 * seed EXACTLY the array the GPU returns -- both read their draws from csrc/walk_draw.h.  OpenMP over the walkers; the
 * result does not depend on the number of threads.  *flags (host int): bit 0 a start id outside [0, num_nodes), bit 1 a
 * neighbour id outside, bit 2 a malformed row of indptr; non-zero marks an invalid result (nothing is read out of bounds).
 * fallback_steps: NULL, or int32[W] receiving per walker the number of steps decided by the exact pass. */
COGDL_HOST_API int cogdl_host_random_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                                          int64_t num_edges, const int64_t *start, int64_t n_walkers, int64_t length,
                                          double restart_p, uint64_t seed, int64_t *walks, int *flags);
COGDL_HOST_API int cogdl_host_node2vec_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                                            int64_t num_edges, const int64_t *start, int64_t n_walkers, int64_t length,
                                            double p, double q, int max_trials, uint64_t seed, int64_t *walks,
                                            int32_t *fallback_steps, int *flags);

/* Metapath-constrained random walk on the typed row layout, the host twin of cogdl_hip_metapath_walk (include/cogdl_hip.h,
 * where the contract is spelled out): same arguments minus the stream, and for equal inputs and seed EXACTLY the arrays the
 * GPU returns -- both run step_metapath of csrc/walk_draw.h.  seg: int64[num_nodes * num_types + 1], indices_t the
 * neighbours ordered by type inside each row; pattern / path_off / walker_path: int32, one period per metapath; an empty
 * segment ends the walk and the rest of the row holds -1; lengths: NULL, or int32[W].  OpenMP over the walkers; the result
 * does not depend on the number of threads.  *flags (host int): bits 0 .. 2 as above, bit 3 (8) a start node whose type is
 * not the first of its metapath (node_type non-NULL), bit 4 (16) a wanted type outside [0, num_types), a walker_path entry
 * outside [0, n_paths) or a malformed path_off.  num_types outside [1, 64], n_paths < 1, a null walker_path / pattern /
 * path_off with W > 0: COGDL_HOST_EINVAL. */
COGDL_HOST_API int cogdl_host_metapath_walk(const int64_t *seg, const int64_t *indices_t, int64_t num_nodes,
                                            int32_t num_types, int64_t num_edges, const int32_t *node_type,
                                            const int64_t *start, const int32_t *walker_path, int64_t n_walkers,
                                            int64_t length, const int32_t *pattern, const int32_t *path_off,
                                            int32_t n_paths, uint64_t seed, int64_t *walks, int32_t *lengths, int *flags);

/* NetSMF path sampling, the host twin of cogdl_hip_netsmf_sample (include/cogdl_hip.h, where the contract is spelled out):
 * same arguments minus the stream, and for equal inputs and seed EXACTLY the arrays the GPU returns -- both run
 * csrc/netsmf_law.h.  out_row / out_col: int32[window * n_samples], sample (s, r) at (r - 1) * n_samples + (s - first_sample).
 * OpenMP over the output positions; the result does not depend on the number of threads.  *flags (host int): bit 1 a
 * neighbour id outside [0, num_nodes), bit 2 a malformed row of indptr; such samples are (-1, -1), nothing is read out of
 * bounds.  Bad sizes: COGDL_HOST_EINVAL; num_nodes >= 2^31 or n_samples > 2^53: COGDL_HOST_ERANGE. */
COGDL_HOST_API int cogdl_host_netsmf_sample(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                                            int64_t num_edges, int64_t first_sample, int64_t n_samples, int window,
                                            uint64_t seed, int32_t *out_row, int32_t *out_col, int *flags);

/* Top-k personalised PageRank by forward push; the host twin of cogdl_hip_ppr_topk (include/cogdl_hip.h, where the contract
 * is spelled out): same arguments minus workspace and stream, and for equal inputs EXACTLY the arrays the GPU returns --
 * both run the fixed-point arithmetic of csrc/ppr_fixed.h in the same synchronous rounds.  OpenMP over the sources; the
 * result does not depend on the number of threads.  *flags (host int) as in the GPU entry point.
 * cogdl_host_ppr_plan validates (alpha, eps) for a graph size and reports what both twins derive from them:
 * out[0] = push budget floor(2^62 / thr) + 1, out[1] = table slots, out[2] = round bound, out[3] = 1 if the GPU keeps a
 * table of that size in LDS.  COGDL_HOST_EINVAL: a parameter outside its domain (alpha in (0, 1), eps > 0);
 * COGDL_HOST_ERANGE: alpha * eps < 2^-20, or the proven rounding loss 4 (E + budget + 2) / alpha * 2^-62 is not below
 * 2^-24, or the table would exceed 2^23 slots. */
COGDL_HOST_API int cogdl_host_ppr_plan(int64_t num_nodes, int64_t num_edges, int64_t max_source_degree, double alpha,
                                       double eps, int64_t *out);
COGDL_HOST_API int cogdl_host_ppr_topk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                       const int64_t *sources, int64_t n_sources, int64_t max_source_degree, double alpha,
                                       double eps, int64_t topk, int64_t *nbr, float *val, int32_t *count, int32_t *stats,
                                       int *flags);

/* Skip-gram training with negative sampling; the host twin of cogdl_hip_sgns_init / cogdl_hip_sgns_train (include/cogdl_hip.h,
 * where the contract is spelled out): same arguments minus rows_in_flight and the stream, all pointers host memory.
 * workers == 1 is strictly sequential and returns EXACTLY the tables of the GPU's serial mode (both run csrc/sgns_law.h);
 * workers == 0 (OpenMP's default thread count) or > 1 runs the rows of an epoch in parallel without locks.
 * trace: NULL, or double [trace_cap, 6] filled in the sequential mode only (COGDL_HOST_EINVAL otherwise) with one record
 * (epoch, row, input id, target id, label, learning rate) per applied target, in order; *trace_n receives the number of
 * applied targets, which may exceed trace_cap (the surplus is not written). */
COGDL_HOST_API int cogdl_host_sgns_init(float *syn0, float *syn1, int64_t V, int D, uint64_t seed);
COGDL_HOST_API int cogdl_host_sgns_train(const int64_t *walks, int64_t W, int64_t L, int64_t V, int D, int window,
                                         int negative, int64_t epochs, double alpha, double min_alpha, const uint32_t *keep,
                                         const uint32_t *cum, const float *exp_table, uint64_t seed, int workers,
                                         float *syn0, float *syn1, int *flags, double *trace, int64_t trace_cap,
                                         int64_t *trace_n);

/* Batched graph readout; the host twins of cogdl_hip_segment_ptr / segment_pool_fwd / segment_pool_bwd / sort_pool_fwd /
 * sort_pool_bwd (include/cogdl_hip.h, where the contract is spelled out): same arguments minus workspace and stream, all
 * pointers host memory, *flag a host int.  Both sides follow csrc/readout_law.h, so for equal inputs they return EXACTLY the
 * same arrays in every mode, above cogdl_host_segment_exact_nodes() rows per segment as well.  OpenMP over the graphs; the
 * result does not depend on the number of threads. */
COGDL_HOST_API int cogdl_host_segment_exact_nodes(void);
COGDL_HOST_API int cogdl_host_segment_ptr(const int64_t *batch, int64_t N, int64_t B, int32_t *ptr, int *flag);
COGDL_HOST_API int cogdl_host_segment_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int mode,
                                               float *out, int32_t *argmax);
COGDL_HOST_API int cogdl_host_segment_pool_bwd(const float *grad, const int32_t *ptr, const int64_t *batch,
                                               const int32_t *argmax, int64_t N, int64_t B, int64_t F, int mode,
                                               float *grad_x);
COGDL_HOST_API int cogdl_host_sort_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int64_t k,
                                            int64_t key_col, float *out, int32_t *idx);
COGDL_HOST_API int cogdl_host_sort_pool_bwd(const float *grad, const int32_t *idx, int64_t N, int64_t B, int64_t F, int64_t k,
                                            float *grad_x);

/* One step of a polynomial graph filter; the host twin of cogdl_hip_csr_filter_step (include/cogdl_hip.h, where the contract
 * is spelled out): same arguments minus workspace and stream, all pointers host memory, dtype 0 (fp32) only.  An OpenMP loop
 * over the rows; every row's sum is sequential fp32 in CSR order and the epilogue follows the header's statement order with
 * separately rounded products and sums, so for equal inputs it returns EXACTLY the GPU's arrays in every row of at most the
 * long-row threshold (cogdl_hip_long_row_threshold) edges; a longer row's sum is re-associated on the GPU and agrees to
 * fp32 summation error.  The result does not depend on the number of threads.  The aliasing rules are the GPU's
 * (COGDL_HOST_EINVAL); a malformed rowptr or a column id outside [0, n): COGDL_HOST_ERANGE, nothing is read out of bounds. */
COGDL_HOST_API int cogdl_host_csr_filter_step(const int32_t *rowptr, const int32_t *colind, const float *val, const float *x,
                                              float *out, int64_t n, int64_t k, int64_t nnz, int dtype, float a, float b,
                                              const float *z1, float c1, const float *z2, float c2, const float *dst_scale,
                                              float *acc, float d);

/* All-entity ranking counts; the host twin of cogdl_hip_kg_rank (include/cogdl_hip.h, where the contract is spelled out): same
 * arguments minus workspace and stream, all pointers host memory.  Both sides follow csrc/kgrank_law.h, so for equal inputs
 * all three counts of every query are EXACTLY the GPU's.  OpenMP over the queries; the result does not depend on the number
 * of threads. */
COGDL_HOST_API int cogdl_host_kg_rank(const float *q, const float *table, const int32_t *target, int64_t M, int64_t N,
                                      int64_t D, int kind, float gamma, const int32_t *filt_ptr, const int32_t *filt_idx,
                                      int64_t filt_len, int32_t *counts);

/* Sampled triple scores and their two gradients; the host twins of cogdl_hip_kg_score, cogdl_hip_kg_score_grad_q and
 * cogdl_hip_kg_score_grad_table (include/cogdl_hip.h, where the contract is spelled out): same arguments minus the stream, all
 * pointers host memory, no alignment requirement, no limit on D.  Both sides follow csrc/kgscore_law.h, so for equal inputs
 * scores and both gradients are EXACTLY the GPU's.  OpenMP over the query rows (the entities for grad_table); the result does
 * not depend on the number of threads. */
COGDL_HOST_API int cogdl_host_kg_score(const float *q, const float *table, const int32_t *idx, int64_t B, int64_t K, int64_t N,
                                       int64_t D, int kind, float gamma, float *scores);
COGDL_HOST_API int cogdl_host_kg_score_grad_q(const float *q, const float *table, const int32_t *idx, const float *g, int64_t B,
                                              int64_t K, int64_t N, int64_t D, int kind, float *grad_q);
COGDL_HOST_API int cogdl_host_kg_score_grad_table(const float *q, const float *table, const float *g, const int32_t *occ_ptr,
                                                  const int32_t *occ_pos, int64_t B, int64_t K, int64_t N, int64_t D, int kind,
                                                  float *grad_table);

/* Weisfeiler-Lehman subtree relabelling; the host twin of cogdl_hip_wl_labels (include/cogdl_hip.h, where the contract is
 * spelled out): same arguments minus the workspace and the stream, all pointers host memory.  Signatures are compared
 * outright, so the result never depends on a hash; labels and classes are EXACTLY the GPU's.  hash_bits < 128 emulates the
 * GPU's truncated hash: *flags gets bit 3 (8) where two different signatures of a round share the truncated hash, which is
 * where the GPU's verification raises it.  The same degree cap applies (bit 2).  The result does not depend on the number
 * of threads. */
COGDL_HOST_API int cogdl_host_wl_max_degree(void);
COGDL_HOST_API int cogdl_host_wl_labels(const int32_t *indptr, const int32_t *indices, const int64_t *label0, int64_t N,
                                        int64_t E, int64_t rounds, int hash_bits, uint64_t salt, int32_t *labels,
                                        int64_t *classes, int *flags);

/* PV-DBOW training; the host twins of cogdl_hip_pvdbow_init / cogdl_hip_pvdbow_train (include/cogdl_hip.h): same arguments
 * minus docs_in_flight and the stream, all pointers host memory.  workers == 1 is strictly sequential and returns EXACTLY
 * the tables of the GPU's serial mode (both run csrc/pvdbow_law.h); workers == 0 (OpenMP's default thread count) or > 1
 * runs the documents of an epoch in parallel without locks. */
COGDL_HOST_API int cogdl_host_pvdbow_init(float *dv, int64_t G, float *syn1, int64_t V, int D, uint64_t seed);
COGDL_HOST_API int cogdl_host_pvdbow_train(const int64_t *doc_ptr, int64_t G, const int64_t *words, int64_t T, int64_t V, int D,
                                           int negative, int64_t epochs, double alpha, double min_alpha, const uint32_t *keep,
                                           const uint32_t *cum, const float *exp_table, uint64_t seed, int workers, float *dv,
                                           float *syn1, int *flags);

/* One training batch of a knowledge-graph embedding model; the host twin of cogdl_hip_kg_train_batch (include/cogdl_hip.h,
 * where the contract is spelled out): same arguments minus the stream, all pointers host memory, no alignment requirement.
 * Both sides follow csrc/kgsample_law.h, so for equal inputs positive, negative, weight and *status are EXACTLY the GPU's.
 * OpenMP over the rows of the batch; the result does not depend on the number of threads.  Sizes of 2^31 - 1 and more:
 * COGDL_HOST_ERANGE. */
COGDL_HOST_API int cogdl_host_kg_train_batch(const int32_t *triples, const float *weight_tab, const int32_t *group,
                                             const int32_t *list_ptr, const int32_t *list_idx, int64_t T, int64_t G,
                                             int64_t list_len, const int32_t *order, int64_t B, int64_t K, int64_t N,
                                             uint64_t seed, uint32_t tag, uint64_t first_sid, int index64, int64_t *positive,
                                             void *negative, float *weight, int *status);

/* Edge-sampled skip-gram training (LINE, orders 1 and 2); the host twin of cogdl_hip_line_train (include/cogdl_hip.h, where
 * the contract is spelled out): same arguments minus samples_in_flight and the stream, all pointers host memory.
 * workers == 1 is strictly sequential and returns EXACTLY the tables of the GPU's serial mode (both run csrc/line_law.h);
 * workers == 0 (OpenMP's default thread count) or > 1 runs the samples in parallel without locks.
 * trace: NULL, or double [trace_cap, 5] filled in the sequential mode only (COGDL_HOST_EINVAL otherwise) with one record
 * (sample, input id u, target id, label, learning rate) per applied target, in order; *trace_n receives the number of
 * applied targets, which may exceed trace_cap (the surplus is not written). */
COGDL_HOST_API int cogdl_host_line_train(const int64_t *eu, const int64_t *ev, const int64_t *ecum, int64_t M, int64_t V,
                                         const uint32_t *ncum, const float *exp_table, int D, int negative, int order,
                                         int64_t S, double alpha, uint64_t seed, int workers, float *emb, float *ctx,
                                         int *flags, double *trace, int64_t trace_cap, int64_t *trace_n);

/* Activation compression; the host twins of cogdl_hip_actq_quantize / _actq_dequantize / _relu_mask / _mask_apply /
 * _drop_apply (include/cogdl_hip.h, where the contract is spelled out): same arguments minus the stream, all pointers host
 * memory, no alignment requirement.  Both sides follow csrc/actq_law.h, so for equal inputs every output byte is the GPU's.
 * OpenMP over tiles of 256 elements; the result does not depend on the number of threads. */
COGDL_HOST_API int cogdl_host_actq_quantize(const float *x, int64_t n, int bits, int group, uint64_t seed, uint64_t call,
                                            uint32_t *codes, float *meta);
COGDL_HOST_API int cogdl_host_actq_dequantize(const uint32_t *codes, const float *meta, int64_t n, int bits, int group,
                                              float *out);
COGDL_HOST_API int cogdl_host_relu_mask(const float *x, int64_t n, float *y, uint64_t *mask);
COGDL_HOST_API int cogdl_host_mask_apply(const float *g, const uint64_t *mask, int64_t n, float *out);
COGDL_HOST_API int cogdl_host_drop_apply(const float *x, int64_t n, uint64_t seed, uint64_t call, uint32_t thresh, float scale,
                                         float *y);

#ifdef __cplusplus
}
#endif
#endif
