// genaggr_op.h -- the functors of the GENConv aggregation on the row-reduce engine (rowreduce.h), over the element type T of
// the tables: float (genaggr.hip) and __half / __hip_bfloat16 (genaggr16.hip).  The mathematics, the engine's view of forward
// and backward and the byte counts are in the header of genaggr.hip.
//
// Whatever T is, every value is an fp32 register from its load to its store: elements are converted as they arrive (exact),
// the message, the online-softmax state {max, denom, numer[, sq]}, the merge of long-row pieces and the backward's per-edge
// term are the same fp32 expressions in the same order, and a 16-bit result is rounded once, to nearest, where it is stored.
// T = float compiles to what these functors were before they took a type.
//
// 16-bit data movement.  The lane mapping is the fp32 kernels' (genaggr16.hip says why): a lane owns VEC = 4 / 2 / 1 consecutive
// columns and gathers them with one 8 / 4 / 2-byte load, which stays packed (GenLanes) until apply() converts an element, so a
// batch of UNROLL gathers in flight holds half the registers of its fp32 values.  lse, q, the unrounded out32 and a pre-scaled
// gradient are fp32 tables of the 16-bit kernels and move as in the fp32 kernels.
#pragma once
#include <cmath>
#include <type_traits>

#include "rowreduce.h"

namespace cogdl {

constexpr float kGenNegInf = -INFINITY;

// relu(x + t) + eps, rounded like the torch expression (the library is built with -ffp-contract=off)
__device__ __forceinline__ float gen_message(float pre, float eps) { return fmaxf(pre, 0.f) + eps; }

// VEC consecutive 16-bit elements as a lane loaded them: one vector load, each element converted where it is used (get(i), i
// a constant once the column loops are unrolled).
template <typename E, int VEC>
struct GenLanes {
    union {
        typename RawVec<sizeof(E) * VEC>::type r;
        E e[VEC];
    };
    __device__ __forceinline__ void load(const E *p) { r = load_raw<E, VEC>(p); }
    __device__ __forceinline__ float get(int i) const { return to_f32<E>(e[i]); }
};
// ... and of floats: the registers load_vec fills, as the fp32 kernels always held them.
template <int VEC>
struct GenLanes<float, VEC> {
    float v[VEC];
    __device__ __forceinline__ void load(const float *p) { load_vec<float, VEC>(p, v); }
    __device__ __forceinline__ float get(int i) const { return v[i]; }
};

// ---------------------------------------------------------------------------------------------------------------- forward
// SOFTMAX: online softmax per column; otherwise the additive state of sum / mean.  SQ: also carry SUM exp(.) m^2.
template <typename T, int VEC_, int LPR_, int UNROLL_, bool SOFTMAX, bool SQ>
struct GenFwdOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_;
    static constexpr int kRec = SOFTMAX ? (SQ ? 4 : 3) * VEC_ : VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    static constexpr bool kHalf = !std::is_same_v<T, float>;
    const int32_t *rowptr;  // for the mean
    const int32_t *eid;     // CSR position -> edge id of t (NULL: identity)
    const T *x;             // [n_src, k]
    const T *t;             // [E, k] or NULL
    const float *beta_dev;  // one float on the device, or NULL: `beta`
    T *out;                 // [m, k]
    float *lse, *q;         // [m, k]; may be NULL
    float *out32;           // [m, k] or NULL (16-bit T): `out` before its rounding, what the backward reads
    int k, mean;
    float beta, eps;

    struct Ctx {
        int col0;
        bool col_ok;
        const T *xcol, *tcol;
        float w, beta;
    };
    struct State {
        float mx[SOFTMAX ? VEC : 1], den[SOFTMAX ? VEC : 1], num[VEC], sq[SQ ? VEC : 1];
    };
    struct LaneVals { int id; };
    struct Batch {
        GenLanes<T, VEC> v[UNROLL];
        GenLanes<T, VEC> t[UNROLL];
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
        b.v[u].load(c.xcol + (int64_t)col * k);
        if (c.tcol) {
            const int id = group_bcast<LPR>(lv.id, sub, jj);
            b.t[u].load(c.tcol + (int64_t)id * k);
        }
    }
    // Online softmax with ONE expf per (edge, column): d = z - max; e = exp(-|d|) rescales the state (d > 0: a new max) or
    // weighs the edge (d <= 0).  The first edge of a row meets max = -inf: e = exp(-inf) = 0, the edge's weight is exactly 1,
    // so a row of one edge returns m bit for bit (num = 0 * 0 + 1 * m, den = 1).
    __device__ __forceinline__ void apply(const Ctx &c, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;  // (group-uniform)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float m = gen_message(c.tcol ? b.v[u].get(i) + b.t[u].get(i) : b.v[u].get(i), eps);
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
            store_vec<T, VEC>(out + at, o);
            if constexpr (kHalf) {
                if (out32) store_vec<float, VEC>(out32 + at, o);
            }
            if (lse) store_vec<float, VEC>(lse + at, l);
            if (SQ && q) store_vec<float, VEC>(q + at, qq);
        } else {
            store_vec<T, VEC>(out + at, s.num);
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
// TG: the element type of the upstream gradient -- T, or float where the caller scaled it per destination in fp32 (mean).
template <typename T, typename TG, int VEC_, int LPR_, int UNROLL_, bool SOFTMAX>
struct GenBwdOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *eid;     // sorted position -> edge id of t / g_t (NULL: identity)
    const T *x;             // [n_src, k]: the rows of this view
    const T *t;             // [E, k] or NULL
    const TG *grad;         // [m, k] upstream gradient (sum / mean: already times w_v)
    const float *fout;      // [m, k] forward output, unrounded (SOFTMAX)
    const float *lse;       // [m, k] max + log(denom) of the forward (SOFTMAX)
    const float *beta_dev;  // one float on the device, or NULL: `beta`
    T *gx;                  // [n_src, k]
    T *gt;                  // [E, k] or NULL
    int k;
    float beta, eps;

    struct Ctx {
        int col0;
        bool col_ok;
        const TG *gcol;
        const float *ocol, *lcol;
        const T *tcol;
        T *gtcol;
        float xr[VEC];
        float beta;
    };
    struct State { float acc[VEC]; };
    struct LaneVals { int id; };
    struct Batch {
        GenLanes<TG, VEC> g[UNROLL];
        GenLanes<float, VEC> o[SOFTMAX ? UNROLL : 1];
        GenLanes<float, VEC> l[SOFTMAX ? UNROLL : 1];
        GenLanes<T, VEC> t[UNROLL];
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
        if (ok && c.col_ok) load_vec<T, VEC>(x + row * (int64_t)k + c.col0, c.xr);
    }
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &lv, int64_t e) const { lv.id = eid ? eid[e] : (int)e; }
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        b.g[u].load(c.gcol + (int64_t)col * k);
        if constexpr (SOFTMAX) {
            b.o[u].load(c.ocol + (int64_t)col * k);
            b.l[u].load(c.lcol + (int64_t)col * k);
        }
        b.id[u] = 0;
        if (c.tcol || c.gtcol) {
            b.id[u] = group_bcast<LPR>(lv.id, sub, jj);
            if (c.tcol) b.t[u].load(c.tcol + (int64_t)b.id[u] * k);
        }
    }
    __device__ __forceinline__ void apply(const Ctx &c, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;  // (group-uniform; a slot past the chunk's end must not store its g_t row twice)
        float d[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float pre = c.tcol ? c.xr[i] + b.t[u].get(i) : c.xr[i];
            const bool on = pre > 0.f;  // torch: the gradient of relu at 0 is 0
            if constexpr (SOFTMAX) {
                const float m = gen_message(pre, eps);
                const float sm = expf(c.beta * m - b.l[u].get(i));
                d[i] = on ? b.g[u].get(i) * sm * (1.f + c.beta * (m - b.o[u].get(i))) : 0.f;
            } else {
                d[i] = on ? b.g[u].get(i) : 0.f;
            }
            s.acc[i] = s.acc[i] + d[i];
        }
        if (c.gtcol && c.col_ok) store_vec<T, VEC>(c.gtcol + (int64_t)b.id[u] * k, d);
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (!(ok && c.col_ok)) return;
        store_vec<T, VEC>(gx + row * (int64_t)k + c.col0, s.acc);
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

template <typename T>
struct GenArgs {
    const int32_t *rowptr, *colind, *eid;
    const T *x, *t;
    const void *grad;  // T, or float when grad_f32
    const float *fout, *lse_in, *beta_dev;
    T *out;            // the forward's output | the backward's grad_x
    float *lse, *q, *out32;
    T *gt;
    int64_t m, nnz;
    int k, mode, grad_f32;
    float beta, eps;
};

// Forward: one or two gathers per edge (source row, edge-term row).  Backward of the softmax: three or four (g, out, lse,
// edge term), so half the unroll keeps the same number of loads in flight; sum / mean gathers the gradient row alone.
constexpr int kGenFwdUnroll = 4, kGenBwdUnroll = 2, kGenBwdAddUnroll = 4;

template <typename T, int VEC, int LPR>
static int launch_gen(const GenArgs<T> &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    const int64_t tiles = ((int64_t)a.k + (int64_t)LPR * VEC - 1) / ((int64_t)LPR * VEC);
    const bool softmax = a.mode == COGDL_HIP_GEN_SOFTMAX;
    if (kind == 0) {
        if (!softmax) {
            GenFwdOp<T, VEC, LPR, kGenFwdUnroll, false, false> op{a.rowptr, a.eid, a.x, a.t, nullptr, a.out, nullptr, nullptr,
                                                                   nullptr, a.k, a.mode == COGDL_HIP_GEN_MEAN, 1.f, a.eps};
            return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
        }
        if (a.q) {
            GenFwdOp<T, VEC, LPR, kGenFwdUnroll, true, true> op{a.rowptr, a.eid, a.x, a.t, a.beta_dev, a.out, a.lse, a.q,
                                                                 a.out32, a.k, 0, a.beta, a.eps};
            return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
        }
        GenFwdOp<T, VEC, LPR, kGenFwdUnroll, true, false> op{a.rowptr, a.eid, a.x, a.t, a.beta_dev, a.out, a.lse, nullptr,
                                                              a.out32, a.k, 0, a.beta, a.eps};
        return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
    }
    if (softmax) {
        GenBwdOp<T, T, VEC, LPR, kGenBwdUnroll, true> op{a.eid, a.x, a.t, (const T *)a.grad, a.fout, a.lse_in, a.beta_dev,
                                                          a.out, a.gt, a.k, a.beta, a.eps};
        return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
    }
    if constexpr (!std::is_same_v<T, float>) {
        if (a.grad_f32) {
            GenBwdOp<T, float, VEC, LPR, kGenBwdAddUnroll, false> op{a.eid, a.x, a.t, (const float *)a.grad, nullptr, nullptr,
                                                                      nullptr, a.out, a.gt, a.k, 1.f, a.eps};
            return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
        }
    }
    GenBwdOp<T, T, VEC, LPR, kGenBwdAddUnroll, false> op{a.eid, a.x, a.t, (const T *)a.grad, nullptr, nullptr, nullptr, a.out,
                                                          a.gt, a.k, 1.f, a.eps};
    return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
}

template <typename T, int VEC>
static int gen_lpr(const GenArgs<T> &a, int kind, int lpr, void *ws, size_t wsb, hipStream_t s) {
    switch (lpr) {
        case 4: return launch_gen<T, VEC, 4>(a, kind, ws, wsb, s);
        case 8: return launch_gen<T, VEC, 8>(a, kind, ws, wsb, s);
        case 16: return launch_gen<T, VEC, 16>(a, kind, ws, wsb, s);
        case 32: return launch_gen<T, VEC, 32>(a, kind, ws, wsb, s);
        case 64: return launch_gen<T, VEC, 64>(a, kind, ws, wsb, s);
        default: return COGDL_HIP_ERANGE;  // a lane group the functors are not built for
    }
}

static inline int gen_check(int64_t m, int64_t k, int64_t nnz, int mode) {
    if (m < 0 || k < 0 || nnz < 0) return COGDL_HIP_EINVAL;
    if (mode < COGDL_HIP_GEN_SOFTMAX || mode > COGDL_HIP_GEN_MEAN) return COGDL_HIP_EINVAL;
    if (k > 0x7fffffff || m > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    return COGDL_HIP_OK;
}

}  // namespace cogdl
