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
// fp32 only, no atomics.  Algorithmic bytes per edge (F columns): forward 4 (colind) [+ 4 eid + 4 F t] + 4 F (source row);
// backward 4 [+ 4 + 4 F t] + 12 F (softmax: g, out, lse rows) | 4 F (sum / mean) [+ 4 F g_t].
#include <cmath>

#include "rowreduce.h"

namespace cogdl {

constexpr float kGenNegInf = -INFINITY;

// relu(x + t) + eps, rounded like the torch expression (the library is built with -ffp-contract=off)
__device__ __forceinline__ float gen_message(float pre, float eps) { return fmaxf(pre, 0.f) + eps; }

// ---------------------------------------------------------------------------------------------------------------- forward
// SOFTMAX: online softmax per column; otherwise the additive state of sum / mean.  SQ: also carry SUM exp(.) m^2.
template <int VEC_, int LPR_, int UNROLL_, bool SOFTMAX, bool SQ>
struct GenFwdOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_;
    static constexpr int kRec = SOFTMAX ? (SQ ? 4 : 3) * VEC_ : VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *rowptr;  // for the mean
    const int32_t *eid;     // CSR position -> edge id of t (NULL: identity)
    const float *x;         // [n_src, k]
    const float *t;         // [E, k] or NULL
    const float *beta_dev;  // one float on the device, or NULL: `beta`
    float *out, *lse, *q;   // [m, k]; lse / q may be NULL
    int k, mean;
    float beta, eps;

    struct Ctx {
        int col0;
        bool col_ok;
        const float *xcol, *tcol;
        float w, beta;
    };
    struct State {
        float mx[SOFTMAX ? VEC : 1], den[SOFTMAX ? VEC : 1], num[VEC], sq[SQ ? VEC : 1];
    };
    struct LaneVals { int id; };
    struct Batch {
        float v[UNROLL][VEC];
        float t[UNROLL][VEC];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx c;
        c.col0 = (tile * LPR + l) * VEC;
        c.col_ok = c.col0 < k;
        const int cc = c.col_ok ? c.col0 : 0;
        c.xcol = x + cc;
        c.tcol = t ? t + cc : nullptr;
        c.w = 1.f;
        c.beta = beta_dev ? *beta_dev : beta;
        return c;
    }
    __device__ __forceinline__ void row_load(Ctx &c, int64_t row, bool ok) const {
        if constexpr (!SOFTMAX) {
            if (mean && ok) {  // deg.pow(-1) with 1 / 0 -> 0 (deepergcn_layer.py:83-86)
                const int deg = rowptr[row + 1] - rowptr[row];
                c.w = deg > 0 ? 1.0f / (float)deg : 0.f;
            }
        }
    }
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s.num[i] = 0.f;
            if constexpr (SOFTMAX) s.mx[i] = kGenNegInf, s.den[i] = 0.f;
            if constexpr (SQ) s.sq[i] = 0.f;
        }
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &lv, int64_t e) const { lv.id = eid ? eid[e] : (int)e; }
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        load_vec<float, VEC>(c.xcol + (int64_t)col * k, b.v[u]);
        if (c.tcol) {
            const int id = group_bcast<LPR>(lv.id, sub, jj);
            load_vec<float, VEC>(c.tcol + (int64_t)id * k, b.t[u]);
        }
    }
    // Online softmax with ONE expf per (edge, column): d = z - max; e = exp(-|d|) rescales the state (d > 0: a new max) or
    // weighs the edge (d <= 0).  The first edge of a row meets max = -inf: e = exp(-inf) = 0, the edge's weight is exactly 1,
    // so a row of one edge returns m bit for bit (num = 0 * 0 + 1 * m, den = 1).
    __device__ __forceinline__ void apply(const Ctx &c, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;  // (group-uniform)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float m = gen_message(c.tcol ? b.v[u][i] + b.t[u][i] : b.v[u][i], eps);
            if constexpr (SOFTMAX) {
                const float z = c.beta * m;
                const float d = z - s.mx[i];
                const float e = expf(-fabsf(d));
                const bool up = d > 0.f;
                const float sc = up ? e : 1.f, p = up ? 1.f : e;
                const float pm = p * m;
                s.den[i] = s.den[i] * sc + p;
                s.num[i] = s.num[i] * sc + pm;
                if constexpr (SQ) s.sq[i] = s.sq[i] * sc + pm * m;
                s.mx[i] = up ? z : s.mx[i];
            } else {
                s.num[i] = s.num[i] + m * c.w;  // the product rounded before the add: edge_msg * deg_rev[row], scatter_add_
            }
        }
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (!(ok && c.col_ok)) return;
        const int64_t at = row * (int64_t)k + c.col0;
        if constexpr (SOFTMAX) {
            float o[VEC], l[VEC], qq[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const bool any = s.den[i] > 0.f;  // an empty row: 0 everywhere
                o[i] = any ? s.num[i] / s.den[i] : 0.f;
                l[i] = any ? s.mx[i] + logf(s.den[i]) : 0.f;
                qq[i] = (SQ && any) ? s.sq[SQ ? i : 0] / s.den[i] : 0.f;
            }
            store_vec<float, VEC>(out + at, o);
            if (lse) store_vec<float, VEC>(lse + at, l);
            if (SQ && q) store_vec<float, VEC>(q + at, qq);
        } else {
            store_vec<float, VEC>(out + at, s.num);
        }
    }
    __device__ __forceinline__ void pack(const State &s, float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            rec[i] = s.num[i];
            if constexpr (SOFTMAX) rec[VEC + i] = s.mx[i], rec[2 * VEC + i] = s.den[i];
            if constexpr (SQ) rec[3 * VEC + i] = s.sq[i];
        }
    }
    __device__ __forceinline__ void unpack(State &s, const float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s.num[i] = rec[i];
            if constexpr (SOFTMAX) s.mx[i] = rec[VEC + i], s.den[i] = rec[2 * VEC + i];
            if constexpr (SQ) s.sq[i] = rec[3 * VEC + i];
        }
    }
    // b's edges follow a's.  A state without edges has max = -inf and weight 0 (never exp(-inf + inf)).
    __device__ __forceinline__ void merge(const Ctx &, State &a, const State &b) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if constexpr (SOFTMAX) {
                const float nm = fmaxf(a.mx[i], b.mx[i]);
                const float sa = a.mx[i] == kGenNegInf ? 0.f : expf(a.mx[i] - nm);
                const float sb = b.mx[i] == kGenNegInf ? 0.f : expf(b.mx[i] - nm);
                a.den[i] = a.den[i] * sa + b.den[i] * sb;
                a.num[i] = a.num[i] * sa + b.num[i] * sb;
                if constexpr (SQ) a.sq[i] = a.sq[i] * sa + b.sq[i] * sb;
                a.mx[i] = nm;
            } else {
                a.num[i] += b.num[i];
            }
        }
    }
};

// --------------------------------------------------------------------------------------------------------------- backward
template <int VEC_, int LPR_, int UNROLL_, bool SOFTMAX>
struct GenBwdOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *eid;     // sorted position -> edge id of t / g_t (NULL: identity)
    const float *x;         // [n_src, k]: the rows of this view
    const float *t;         // [E, k] or NULL
    const float *grad;      // [m, k] upstream gradient (sum / mean: already times w_v)
    const float *fout;      // [m, k] forward output (SOFTMAX)
    const float *lse;       // [m, k] max + log(denom) of the forward (SOFTMAX)
    const float *beta_dev;  // one float on the device, or NULL: `beta`
    float *gx;              // [n_src, k]
    float *gt;              // [E, k] or NULL
    int k;
    float beta, eps;

    struct Ctx {
        int col0;
        bool col_ok;
        const float *gcol, *ocol, *lcol, *tcol;
        float *gtcol;
        float xr[VEC];
        float beta;
    };
    struct State { float acc[VEC]; };
    struct LaneVals { int id; };
    struct Batch {
        float g[UNROLL][VEC];
        float o[SOFTMAX ? UNROLL : 1][VEC];
        float l[SOFTMAX ? UNROLL : 1][VEC];
        float t[UNROLL][VEC];
        int id[UNROLL];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx c;
        c.col0 = (tile * LPR + l) * VEC;
        c.col_ok = c.col0 < k;
        const int cc = c.col_ok ? c.col0 : 0;
        c.gcol = grad + cc;
        c.ocol = SOFTMAX ? fout + cc : nullptr;
        c.lcol = SOFTMAX ? lse + cc : nullptr;
        c.tcol = t ? t + cc : nullptr;
        c.gtcol = gt ? gt + cc : nullptr;
#pragma unroll
        for (int i = 0; i < VEC; ++i) c.xr[i] = 0.f;
        c.beta = beta_dev ? *beta_dev : beta;
        return c;
    }
    __device__ __forceinline__ void row_load(Ctx &c, int64_t row, bool ok) const {
        if (ok && c.col_ok) load_vec<float, VEC>(x + row * (int64_t)k + c.col0, c.xr);
    }
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &lv, int64_t e) const { lv.id = eid ? eid[e] : (int)e; }
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        load_vec<float, VEC>(c.gcol + (int64_t)col * k, b.g[u]);
        if constexpr (SOFTMAX) {
            load_vec<float, VEC>(c.ocol + (int64_t)col * k, b.o[u]);
            load_vec<float, VEC>(c.lcol + (int64_t)col * k, b.l[u]);
        }
        b.id[u] = 0;
        if (c.tcol || c.gtcol) {
            b.id[u] = group_bcast<LPR>(lv.id, sub, jj);
            if (c.tcol) load_vec<float, VEC>(c.tcol + (int64_t)b.id[u] * k, b.t[u]);
        }
    }
    __device__ __forceinline__ void apply(const Ctx &c, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;  // (group-uniform; a slot past the chunk's end must not store its g_t row twice)
        float d[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float pre = c.tcol ? c.xr[i] + b.t[u][i] : c.xr[i];
            const bool on = pre > 0.f;  // torch: the gradient of relu at 0 is 0
            if constexpr (SOFTMAX) {
                const float m = gen_message(pre, eps);
                const float sm = expf(c.beta * m - b.l[u][i]);
                d[i] = on ? b.g[u][i] * sm * (1.f + c.beta * (m - b.o[u][i])) : 0.f;
            } else {
                d[i] = on ? b.g[u][i] : 0.f;
            }
            s.acc[i] = s.acc[i] + d[i];
        }
        if (c.gtcol && c.col_ok) store_vec<float, VEC>(c.gtcol + (int64_t)b.id[u] * k, d);
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (!(ok && c.col_ok)) return;
        store_vec<float, VEC>(gx + row * (int64_t)k + c.col0, s.acc);
    }
    __device__ __forceinline__ void pack(const State &s, float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) rec[i] = s.acc[i];
    }
    __device__ __forceinline__ void unpack(State &s, const float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = rec[i];
    }
    __device__ __forceinline__ void merge(const Ctx &, State &a, const State &b) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) a.acc[i] += b.acc[i];
    }
};

struct GenArgs {
    const int32_t *rowptr, *colind, *eid;
    const float *x, *t, *grad, *fout, *lse_in, *beta_dev;
    float *out, *lse, *q, *gt;
    int64_t m, nnz;
    int k, mode;
    float beta, eps;
};

// Forward: one or two gathers per edge (source row, edge-term row).  Backward of the softmax: three or four (g, out, lse,
// edge term), so half the unroll keeps the same number of loads in flight; sum / mean gathers the gradient row alone.
constexpr int kGenFwdUnroll = 4, kGenBwdUnroll = 2, kGenBwdAddUnroll = 4;

template <int VEC, int LPR>
static int launch_gen(const GenArgs &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    const int64_t tiles = ((int64_t)a.k + (int64_t)LPR * VEC - 1) / ((int64_t)LPR * VEC);
    const bool softmax = a.mode == COGDL_HIP_GEN_SOFTMAX;
    if (kind == 0) {
        if (!softmax) {
            GenFwdOp<VEC, LPR, kGenFwdUnroll, false, false> op{a.rowptr, a.eid, a.x, a.t, nullptr, a.out, nullptr, nullptr,
                                                                a.k, a.mode == COGDL_HIP_GEN_MEAN, 1.f, a.eps};
            return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
        }
        if (a.q) {
            GenFwdOp<VEC, LPR, kGenFwdUnroll, true, true> op{a.rowptr, a.eid, a.x, a.t, a.beta_dev, a.out, a.lse, a.q,
                                                              a.k, 0, a.beta, a.eps};
            return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
        }
        GenFwdOp<VEC, LPR, kGenFwdUnroll, true, false> op{a.rowptr, a.eid, a.x, a.t, a.beta_dev, a.out, a.lse, nullptr,
                                                           a.k, 0, a.beta, a.eps};
        return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
    }
    if (softmax) {
        GenBwdOp<VEC, LPR, kGenBwdUnroll, true> op{a.eid, a.x, a.t, a.grad, a.fout, a.lse_in, a.beta_dev, a.out, a.gt,
                                                    a.k, a.beta, a.eps};
        return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
    }
    GenBwdOp<VEC, LPR, kGenBwdAddUnroll, false> op{a.eid, a.x, a.t, a.grad, nullptr, nullptr, nullptr, a.out, a.gt,
                                                    a.k, 1.f, a.eps};
    return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
}

template <int VEC>
static int gen_lpr(const GenArgs &a, int kind, int lpr, void *ws, size_t wsb, hipStream_t s) {
    switch (lpr) {
        case 4: return launch_gen<VEC, 4>(a, kind, ws, wsb, s);
        case 8: return launch_gen<VEC, 8>(a, kind, ws, wsb, s);
        case 16: return launch_gen<VEC, 16>(a, kind, ws, wsb, s);
        case 32: return launch_gen<VEC, 32>(a, kind, ws, wsb, s);
        case 64: return launch_gen<VEC, 64>(a, kind, ws, wsb, s);
        default: return COGDL_HIP_ERANGE;  // a lane group the functors are not built for
    }
}

// Vector width 4 -> 2 -> 1 by the alignment of every gathered / stored table and by k (spmm_geometry).
static int gen_dispatch(const GenArgs &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    uintptr_t v = 0;
    for (const void *p : {(const void *)a.x, (const void *)a.t, (const void *)a.grad, (const void *)a.fout,
                          (const void *)a.lse_in, (const void *)a.out, (const void *)a.lse, (const void *)a.q,
                          (const void *)a.gt})
        v |= reinterpret_cast<uintptr_t>(p);
    if (v % 4 != 0 || (a.beta_dev && reinterpret_cast<uintptr_t>(a.beta_dev) % 4 != 0)) return COGDL_HIP_EALIGN;
    const int align = (v % 16 == 0) ? 16 : (v % 8 == 0) ? 8 : 4;
    const RowGeometry g = spmm_geometry(a.k, a.k, 4, align);
    // The workspace was sized for the 16-byte-aligned geometry; a narrower one needs at most as many floats.
    switch (g.vec) {
        case 4: return gen_lpr<4>(a, kind, g.lpr, ws, wsb, s);
        case 2: return gen_lpr<2>(a, kind, g.lpr, ws, wsb, s);
        default: return gen_lpr<1>(a, kind, g.lpr, ws, wsb, s);
    }
}

// rec_floats: floats of a piece record per column (4: the softmax state with sq; 1: the additive state of the backward)
static size_t gen_workspace_bytes(int64_t nnz, int64_t k, int rec_floats) {
    if (nnz <= 0 || k <= 0) return 0;
    const RowGeometry g = spmm_geometry(k, k, 4, 16);
    return rowreduce_workspace_bytes(nnz, g.tiles * g.vec * g.lpr * rec_floats);
}

static int gen_check(int64_t m, int64_t k, int64_t nnz, int mode) {
    if (m < 0 || k < 0 || nnz < 0) return COGDL_HIP_EINVAL;
    if (mode < COGDL_HIP_GEN_SOFTMAX || mode > COGDL_HIP_GEN_MEAN) return COGDL_HIP_EINVAL;
    if (k > 0x7fffffff || m > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    return COGDL_HIP_OK;
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
    GenArgs a{};
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
    GenArgs a{};
    a.rowptr = srcptr, a.colind = dst_sorted, a.eid = eid, a.x = x, a.t = eterm, a.grad = grad, a.beta_dev = beta_dev;
    if (mode == COGDL_HIP_GEN_SOFTMAX) a.fout = out, a.lse_in = lse;
    a.out = grad_x, a.gt = grad_eterm, a.m = n_src, a.nnz = nnz, a.k = (int)k, a.mode = mode, a.beta = beta, a.eps = eps;
    return gen_dispatch(a, 1, workspace, workspace_bytes, (hipStream_t)stream);
}
