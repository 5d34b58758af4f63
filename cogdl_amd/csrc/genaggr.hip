// genaggr.hip -- the aggregation of GENConv (DeeperGCN; cogdl/layers/deepergcn_layer.py:67-93) for gfx950, fused.  The
// reference gathers x[col] into [E, F], adds the encoded edge features, applies relu(.) + eps, multiplies by beta, takes an
// edge softmax with one channel per feature column, multiplies and scatter_add_s: five [E, F] tensors and float atomics.
// Here, over the destination-sorted (CSR) view of the edges,
//
//     m[j, f]   = relu(x[colind[j], f] + t[id_j, f]) + eps                                               id_j = eid[j] | j
//     softmax:    out[v, f] = SUM_{j in row v} softmax_{j in row v}(beta * m[j, f]) * m[j, f]
//     sum / mean: out[v, f] = SUM_{j in row v} w_v * m[j, f]                   w_v = 1 | 1 / deg(v) (0 for an empty row)
//
// is ONE pass of the row-reduce engine (rowreduce.h): per column the state of an online softmax {max, denom, numer} (and
// sq = SUM exp(.) m^2 when beta needs a gradient), updated in CSR edge order with one expf per (edge, column); hub rows are
// cut into pieces whose states merge with the usual rescaling, in a fixed order.  Nothing of size [E, F] is written.
//
// The backward runs over the SOURCE-sorted view (rows = sources u, the engine's column of an edge = its destination v):
// x[u, :] is a per-row operand; per edge g[v, :], out[v, :] and lse[v, :] are gathered, m is recomputed and
//
//     softmax:    d = g[v] * s * (1 + beta * (m - out[v])) * [x[u] + t > 0]           s = exp(beta * m - lse[v])
//     sum / mean: d = g[v] * [x[u] + t > 0]                                           (g already scaled by w_v)
//
// is added to g_x[u, :] in the caller's edge order and, when the edge term needs a gradient, stored to g_t[id, :].
// No atomics.  Algorithmic bytes per edge (F columns, fp32): forward 4 (colind) [+ 4 eid + 4 F t] + 4 F (source row);
// backward 4 [+ 4 + 4 F t] + 12 F (softmax: g, out, lse rows) | 4 F (sum / mean) [+ 4 F g_t].
// The functors are in genaggr_op.h, over the element type of the tables; this file holds the fp32 entries, genaggr16.hip the
// fp16 / bf16 ones.
#include "genaggr_op.h"

namespace cogdl {

// Vector width 4 -> 2 -> 1 by the alignment of every gathered / stored table and by k (spmm_geometry).
static int gen_dispatch(const GenArgs<float> &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    uintptr_t v = 0;
    for (const void *p : {(const void *)a.x, (const void *)a.t, a.grad, (const void *)a.fout,
                          (const void *)a.lse_in, (const void *)a.out, (const void *)a.lse, (const void *)a.q,
                          (const void *)a.gt})
        v |= reinterpret_cast<uintptr_t>(p);
    if (v % 4 != 0 || (a.beta_dev && reinterpret_cast<uintptr_t>(a.beta_dev) % 4 != 0)) return COGDL_HIP_EALIGN;
    const int align = (v % 16 == 0) ? 16 : (v % 8 == 0) ? 8 : 4;
    const RowGeometry g = spmm_geometry(a.k, a.k, 4, align);
    // The workspace was sized for the 16-byte-aligned geometry; a narrower one needs at most as many floats.
    switch (g.vec) {
        case 4: return gen_lpr<float, 4>(a, kind, g.lpr, ws, wsb, s);
        case 2: return gen_lpr<float, 2>(a, kind, g.lpr, ws, wsb, s);
        default: return gen_lpr<float, 1>(a, kind, g.lpr, ws, wsb, s);
    }
}

// rec_floats: floats of a piece record per column (4: the softmax state with sq; 1: the additive state of the backward)
static size_t gen_workspace_bytes(int64_t nnz, int64_t k, int rec_floats) {
    if (nnz <= 0 || k <= 0) return 0;
    const RowGeometry g = spmm_geometry(k, k, 4, 16);
    return rowreduce_workspace_bytes(nnz, g.tiles * g.vec * g.lpr * rec_floats);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_gen_aggr_fwd_workspace_bytes(int64_t nnz, int64_t k) { return gen_workspace_bytes(nnz, k, 4); }

extern "C" int cogdl_hip_gen_aggr_fwd(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const float *x,
                                      const float *eterm, int mode, const float *beta_dev, float beta, float eps, float *out,
                                      float *lse, float *q, int64_t m, int64_t k, int64_t nnz, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    const int rc = gen_check(m, k, nnz, mode);
    if (rc != COGDL_HIP_OK) return rc;
    if (m == 0 || k == 0) return COGDL_HIP_OK;
    if (!rowptr || !out || !x || (nnz > 0 && !colind)) return COGDL_HIP_EINVAL;
    if (q && !lse) return COGDL_HIP_EINVAL;
    if (mode != COGDL_HIP_GEN_SOFTMAX && (lse || q)) return COGDL_HIP_EINVAL;
    GenArgs<float> a{};
    a.rowptr = rowptr, a.colind = colind, a.eid = eid, a.x = x, a.t = eterm, a.beta_dev = beta_dev;
    a.out = out, a.lse = lse, a.q = q, a.m = m, a.nnz = nnz, a.k = (int)k, a.mode = mode, a.beta = beta, a.eps = eps;
    return gen_dispatch(a, 0, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t cogdl_hip_gen_aggr_bwd_workspace_bytes(int64_t nnz, int64_t k) { return gen_workspace_bytes(nnz, k, 1); }

extern "C" int cogdl_hip_gen_aggr_bwd(const int32_t *srcptr, const int32_t *dst_sorted, const int32_t *eid, const float *x,
                                      const float *eterm, const float *grad, const float *out, const float *lse, int mode,
                                      const float *beta_dev, float beta, float eps, float *grad_x, float *grad_eterm,
                                      int64_t n_src, int64_t k, int64_t nnz, void *workspace, size_t workspace_bytes,
                                      void *stream) {
    const int rc = gen_check(n_src, k, nnz, mode);
    if (rc != COGDL_HIP_OK) return rc;
    if (n_src == 0 || k == 0) return COGDL_HIP_OK;
    if (!srcptr || !grad_x || !x || !grad || (nnz > 0 && !dst_sorted)) return COGDL_HIP_EINVAL;
    if (mode == COGDL_HIP_GEN_SOFTMAX && (!out || !lse)) return COGDL_HIP_EINVAL;
    GenArgs<float> a{};
    a.rowptr = srcptr, a.colind = dst_sorted, a.eid = eid, a.x = x, a.t = eterm, a.grad = grad, a.beta_dev = beta_dev;
    if (mode == COGDL_HIP_GEN_SOFTMAX) a.fout = out, a.lse_in = lse;
    a.out = grad_x, a.gt = grad_eterm, a.m = n_src, a.nnz = nnz, a.k = (int)k, a.mode = mode, a.beta = beta, a.eps = eps;
    return gen_dispatch(a, 1, workspace, workspace_bytes, (hipStream_t)stream);
}
