// genaggr16.hip -- the GENConv aggregation (genaggr.hip) on fp16 / bf16 tables: what the layer's inputs are under torch AMP.
// x, eterm, out and the gradients are 16-bit; everything between a load and a store is the fp32 arithmetic of genaggr_op.h.
//
//   forward    out is stored in the tables' type with ONE rounding from the fp32 state (fp16: beyond 65504 that rounding gives
//              inf, nothing is clamped); lse and q stay fp32; when lse is asked for a backward will follow, and it takes
//              out32, the same output before its rounding: 1 + beta * (m - out[v]) must not inherit the store's error.
//   backward   grad in the tables' type -- or fp32 for sum / mean, where the caller's 1 / deg(v) scaling was an fp32 product
//              that is not rounded back --, out32 and lse in fp32; grad_x and grad_eterm rounded once, every grad_eterm row
//              written exactly once.  No atomics: equal from run to run.
//
// Algorithmic bytes per edge (F columns): forward 4 (colind) [+ 4 eid + 2 F t] + 2 F (source row), against 4 + 4 F in fp32:
// (4 + 4 F) / (4 + 2 F) = 1.98 at F = 128.  Backward of the softmax 4 [+ 4 + 2 F t] + 2 F (g) + 8 F (out32, lse) [+ 2 F g_t]
// against 4 + 12 F: the two fp32 rows the backward must not round keep it at 1.2x; sum / mean 4 + 2 F | 4 + 4 F (fp32 grad).
//
// Geometry: the fp32 kernels' (spmm_geometry for 4-byte elements): VEC = 4 / 2 / 1 columns per lane, F = 64 / 128 / 256 on 16 / 64 /
// 64 lanes, so a lane gathers 8 / 4 / 2 bytes.  Measured, not assumed: a first version gave a lane 8 columns and one 128-bit
// load -- F = 128 on 16 lanes, four rows per wave, 123 VGPRs -- and lost to the fp32 kernels on 32 of the benchmark's 48 rows
// (forward, F = 128, arxiv-shaped R-MAT graph: 0.80 ms against 0.48 ms; forward + backward 1.58 against 1.15).  With the fp32
// mapping a lane evaluates the fp32 kernel's expressions on half the bytes: profiles/genconv16_bench.txt has the forward at
// parity (0.85x .. 1.05x of the fp32 kernels' time ratio; the losses are forwards with an edge term on a skewed graph, cause
// not known) and forward + backward at 1.07x .. 1.33x.  The expressions, not the instruction stream: this file is built without
// packed fp32 instructions (csrc/Makefile), which was measured to make no difference.
// The widest VEC is bounded by k and by every table's address -- a 16-bit table needs 2 VEC bytes, an fp32 table 4 VEC -- so an
// operand that starts mid-allocation is served by a narrower width, never refused.
#include "genaggr_op.h"

namespace cogdl {

// The widest vector k and the tables allow; 0: a table that is not aligned to its own element.
static int gen16_vec(int64_t k, std::initializer_list<const void *> half_tables, std::initializer_list<const void *> float_tables) {
    int vec = 4;
    while (vec > 1 && k % vec != 0) vec >>= 1;
    for (const void *p : half_tables) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (a % 2 != 0) return 0;
        while (vec > 1 && a % (2 * vec) != 0) vec >>= 1;
    }
    for (const void *p : float_tables) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (a % 4 != 0) return 0;
        while (vec > 1 && a % (4 * vec) != 0) vec >>= 1;
    }
    return vec;
}

template <typename T>
static int gen16_dispatch(const GenArgs<T> &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    const void *g16 = a.grad_f32 ? nullptr : a.grad, *g32 = a.grad_f32 ? a.grad : nullptr;
    const int vec = gen16_vec(a.k, {a.x, a.t, a.out, a.gt, g16}, {g32, a.fout, a.lse_in, a.lse, a.q, a.out32});
    if (vec == 0 || reinterpret_cast<uintptr_t>(a.beta_dev) % 4 != 0) return COGDL_HIP_EALIGN;
    const RowGeometry g = spmm_geometry(a.k, a.k, 4, 4 * vec);  // (as for 4-byte elements whose tables allow `vec` of them)
    // The workspace was sized for the 16-byte-aligned geometry; a narrower one needs at most as many floats.
    switch (g.vec) {
        case 4: return gen_lpr<T, 4>(a, kind, g.lpr, ws, wsb, s);
        case 2: return gen_lpr<T, 2>(a, kind, g.lpr, ws, wsb, s);
        default: return gen_lpr<T, 1>(a, kind, g.lpr, ws, wsb, s);
    }
}

// rec_floats: floats of a piece record per column (4: the softmax state with sq; 1: the additive state of the backward)
static size_t gen16_workspace_bytes(int64_t nnz, int64_t k, int dtype, int rec_floats) {
    if (nnz <= 0 || k <= 0 || (dtype != COGDL_HIP_F16 && dtype != COGDL_HIP_BF16)) return 0;
    const RowGeometry g = spmm_geometry(k, k, 4, 16);
    return rowreduce_workspace_bytes(nnz, g.tiles * g.vec * g.lpr * rec_floats);
}

template <typename T>
static int gen16_fwd(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const void *x, const void *eterm,
                     int mode, const float *beta_dev, float beta, float eps, void *out, float *out32, float *lse, float *q,
                     int64_t m, int64_t k, int64_t nnz, void *ws, size_t wsb, void *stream) {
    GenArgs<T> a{};
    a.rowptr = rowptr, a.colind = colind, a.eid = eid, a.x = (const T *)x, a.t = (const T *)eterm, a.beta_dev = beta_dev;
    a.out = (T *)out, a.out32 = out32, a.lse = lse, a.q = q, a.m = m, a.nnz = nnz, a.k = (int)k, a.mode = mode;
    a.beta = beta, a.eps = eps;
    return gen16_dispatch<T>(a, 0, ws, wsb, (hipStream_t)stream);
}

template <typename T>
static int gen16_bwd(const int32_t *srcptr, const int32_t *dst_sorted, const int32_t *eid, const void *x, const void *eterm,
                     const void *grad, int grad_f32, const float *out32, const float *lse, int mode, const float *beta_dev,
                     float beta, float eps, void *grad_x, void *grad_eterm, int64_t n_src, int64_t k, int64_t nnz, void *ws,
                     size_t wsb, void *stream) {
    GenArgs<T> a{};
    a.rowptr = srcptr, a.colind = dst_sorted, a.eid = eid, a.x = (const T *)x, a.t = (const T *)eterm, a.grad = grad;
    a.grad_f32 = grad_f32, a.beta_dev = beta_dev;
    if (mode == COGDL_HIP_GEN_SOFTMAX) a.fout = out32, a.lse_in = lse;
    a.out = (T *)grad_x, a.gt = (T *)grad_eterm, a.m = n_src, a.nnz = nnz, a.k = (int)k, a.mode = mode;
    a.beta = beta, a.eps = eps;
    return gen16_dispatch<T>(a, 1, ws, wsb, (hipStream_t)stream);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_gen_aggr16_fwd_workspace_bytes(int64_t nnz, int64_t k, int dtype) {
    return gen16_workspace_bytes(nnz, k, dtype, 4);
}

extern "C" int cogdl_hip_gen_aggr16_fwd(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const void *x,
                                        const void *eterm, int mode, const float *beta_dev, float beta, float eps, void *out,
                                        float *out32, float *lse, float *q, int64_t m, int64_t k, int64_t nnz, int dtype,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    if (dtype != COGDL_HIP_F16 && dtype != COGDL_HIP_BF16) return COGDL_HIP_EDTYPE;
    const int rc = gen_check(m, k, nnz, mode);
    if (rc != COGDL_HIP_OK) return rc;
    if (m == 0 || k == 0) return COGDL_HIP_OK;
    if (!rowptr || !out || !x || (nnz > 0 && !colind)) return COGDL_HIP_EINVAL;
    if ((q && !lse) || (lse && !out32) || (out32 && !lse)) return COGDL_HIP_EINVAL;
    if (mode != COGDL_HIP_GEN_SOFTMAX && (lse || q)) return COGDL_HIP_EINVAL;
    if (dtype == COGDL_HIP_F16)
        return gen16_fwd<__half>(rowptr, colind, eid, x, eterm, mode, beta_dev, beta, eps, out, out32, lse, q, m, k, nnz,
                                 workspace, workspace_bytes, stream);
    return gen16_fwd<__hip_bfloat16>(rowptr, colind, eid, x, eterm, mode, beta_dev, beta, eps, out, out32, lse, q, m, k, nnz,
                                     workspace, workspace_bytes, stream);
}

extern "C" size_t cogdl_hip_gen_aggr16_bwd_workspace_bytes(int64_t nnz, int64_t k, int dtype) {
    return gen16_workspace_bytes(nnz, k, dtype, 1);
}

extern "C" int cogdl_hip_gen_aggr16_bwd(const int32_t *srcptr, const int32_t *dst_sorted, const int32_t *eid, const void *x,
                                        const void *eterm, const void *grad, int grad_dtype, const float *out32,
                                        const float *lse, int mode, const float *beta_dev, float beta, float eps, void *grad_x,
                                        void *grad_eterm, int64_t n_src, int64_t k, int64_t nnz, int dtype, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    if (dtype != COGDL_HIP_F16 && dtype != COGDL_HIP_BF16) return COGDL_HIP_EDTYPE;
    if (grad_dtype != dtype && !(grad_dtype == COGDL_HIP_F32 && mode != COGDL_HIP_GEN_SOFTMAX)) return COGDL_HIP_EDTYPE;
    const int rc = gen_check(n_src, k, nnz, mode);
    if (rc != COGDL_HIP_OK) return rc;
    if (n_src == 0 || k == 0) return COGDL_HIP_OK;
    if (!srcptr || !grad_x || !x || !grad || (nnz > 0 && !dst_sorted)) return COGDL_HIP_EINVAL;
    if (mode == COGDL_HIP_GEN_SOFTMAX && (!out32 || !lse)) return COGDL_HIP_EINVAL;
    const int grad_f32 = grad_dtype == COGDL_HIP_F32;
    if (dtype == COGDL_HIP_F16)
        return gen16_bwd<__half>(srcptr, dst_sorted, eid, x, eterm, grad, grad_f32, out32, lse, mode, beta_dev, beta, eps,
                                 grad_x, grad_eterm, n_src, k, nnz, workspace, workspace_bytes, stream);
    return gen16_bwd<__hip_bfloat16>(srcptr, dst_sorted, eid, x, eterm, grad, grad_f32, out32, lse, mode, beta_dev, beta, eps,
                                     grad_x, grad_eterm, n_src, k, nnz, workspace, workspace_bytes, stream);
}
