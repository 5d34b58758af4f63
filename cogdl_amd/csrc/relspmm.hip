// relspmm.hip -- relational gspmm for gfx950: "source (op) relation embedding, then aggregate" on a graph whose edges carry a
// TYPE.  The message passing of CompGCN (cogdl/models/nn/compgcn.py:124-140), which the reference composes from torch ops: it
// gathers x[col] into [E, k], gathers rel_embed[edge_type] into a second [E, k], combines them, multiplies the [E, k] result
// by the layer weight, scales it per edge and scatter_add_s it (atomics on a GPU: the sums depend on the run).  Here, over the
// destination-sorted (CSR) view of the edges,
//
//     out[v, :] = SUM_{j in row v}  w[id_j] * ( x[colind[j], :]  OP  rel[etype[id_j], :] )              id_j = eid[j] | j
//
// is one pass of the row-reduce engine (rowreduce.h), exactly as gspmm.hip -- a group of LPR lanes per row, coalesced vector
// gathers, strictly sequential accumulation in the caller's edge order, hub rows split over workgroups and merged in a fixed
// order, no atomics -- with the edge operand looked up through the edge's type: the [R, k] table is a few hundred KB and is
// served by the L2, nothing of size [E, k] exists.  The layer weight is shared by the edges of a direction, so the matmul
// moves behind the sum: SUM_e n_e (comp_e W) = (SUM_e n_e comp_e) W.
//
// The gradient of the relation table is the same engine over the TYPE-sorted view (one row per type, stable sort: the edges
// of a type keep the caller's order): no atomics either, the long rows (E / R edges each; N for a self-loop type) are what
// the chunk path is for.  fp32 only.
// Algorithmic bytes per edge: 4 (colind) [+ 4 eid] + 4 (etype) [+ 4 w] + 4 k (source row); the relation rows come from L2.
#include "rowreduce.h"

namespace cogdl {

template <int VEC_, int LPR_, int UNROLL_>
struct RelSpmmOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *eid;    // CSR position -> edge id of etype / weight (NULL: identity)
    const int32_t *etype;  // [E] relation of every edge, in the caller's edge order
    const float *x;        // [n_src, k]
    const float *rel;      // [n_rel, k] (NULL: the message is the source row alone)
    const float *w;        // [E] or NULL
    float *out;            // [m, k]
    int k;
    int op;     // COGDL_HIP_GSPMM_{ADD,SUB,MUL,WMUL}
    int n_rel;  // types are clamped into [0, n_rel): a bad id gives a wrong number, never a read outside rel

    struct Ctx {
        int col0;
        bool col_ok;
        const float *xcol, *relcol;
    };
    struct State { float acc[VEC]; };
    struct LaneVals {
        int t;
        float w;
    };
    struct Batch {
        float v[UNROLL][VEC];
        float r[UNROLL][VEC];
        float w[UNROLL];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx c;
        c.col0 = (tile * LPR + l) * VEC;
        c.col_ok = c.col0 < k;
        const int cc = c.col_ok ? c.col0 : 0;
        c.xcol = x + cc;
        c.relcol = rel ? rel + cc : nullptr;
        return c;
    }
    __device__ __forceinline__ void row_load(Ctx &, int64_t, bool) const {}
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &lv, int64_t e) const {
        const int id = eid ? eid[e] : (int)e;
        lv.w = w ? w[id] : 1.f;
        lv.t = rel ? min(max(etype[id], 0), n_rel - 1) : 0;
    }
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        b.w[u] = group_bcast<LPR>(lv.w, sub, jj);
        load_vec<float, VEC>(c.xcol + (int64_t)col * k, b.v[u]);
        if (c.relcol) {
            const int t = group_bcast<LPR>(lv.t, sub, jj);
            load_vec<float, VEC>(c.relcol + (int64_t)t * k, b.r[u]);
        }
    }
    // msg = (src OP rel) * w, then out += msg: the torch expression of the layer, each step rounded to fp32 (the library is
    // built with -ffp-contract=off).  WMUL: (src * w) * rel, the order of autograd's chain for the source gradient of MUL.
    __device__ __forceinline__ void apply(const Ctx &c, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float msg;
            if (!c.relcol) msg = b.v[u][i];
            else if (op == COGDL_HIP_GSPMM_ADD) msg = b.v[u][i] + b.r[u][i];
            else if (op == COGDL_HIP_GSPMM_SUB) msg = b.v[u][i] - b.r[u][i];
            else if (op == COGDL_HIP_GSPMM_WMUL) msg = (w ? b.v[u][i] * b.w[u] : b.v[u][i]) * b.r[u][i];
            else msg = b.v[u][i] * b.r[u][i];
            if (w && !(c.relcol && op == COGDL_HIP_GSPMM_WMUL)) msg = msg * b.w[u];
            s.acc[i] = s.acc[i] + (valid ? msg : 0.f);
        }
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (!(ok && c.col_ok)) return;
        store_vec<float, VEC>(out + row * (int64_t)k + c.col0, s.acc);
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

// Gradient of the relation table over the type-sorted view: row t = the edges of type t in the caller's order, the engine's
// column array = the DESTINATION of every edge (the upstream gradient row to gather), `src` = the source of every edge in
// the same order (MUL only: the second gathered row).
//     SUB: -(G[row_e] * w_e)      ADD: G[row_e] * w_e      MUL: (G[row_e] * w_e) * x[col_e]
// with autograd's roundings in autograd's order, summed per element in edge order (rows up to the exact-row bound) or in the
// engine's fixed chunk order (the usual case here: a type owns E / R edges).
template <int VEC_, int LPR_, int UNROLL_, bool HAS_X>
struct RelGradOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *eid;  // sorted position -> edge id of weight (NULL: identity)
    const int32_t *src;  // [E] source ids in sorted order (HAS_X)
    const float *grad;   // [m, k] upstream gradient
    const float *x;      // [n_src, k] (HAS_X)
    const float *w;      // [E] or NULL
    float *out;          // [n_rel, k]
    int k;
    int negate;  // SUB

    struct Ctx {
        int col0;
        bool col_ok;
        const float *gcol, *xcol;
    };
    struct State { float acc[VEC]; };
    struct LaneVals {
        int c;
        float w;
    };
    struct Batch {
        float g[UNROLL][VEC];
        float v[HAS_X ? UNROLL : 1][VEC];
        float w[UNROLL];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx c;
        c.col0 = (tile * LPR + l) * VEC;
        c.col_ok = c.col0 < k;
        const int cc = c.col_ok ? c.col0 : 0;
        c.gcol = grad + cc;
        c.xcol = HAS_X ? x + cc : nullptr;
        return c;
    }
    __device__ __forceinline__ void row_load(Ctx &, int64_t, bool) const {}
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &lv, int64_t e) const {
        const int id = eid ? eid[e] : (int)e;
        lv.w = w ? w[id] : 1.f;
        lv.c = HAS_X ? src[e] : 0;
    }
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        b.w[u] = group_bcast<LPR>(lv.w, sub, jj);
        load_vec<float, VEC>(c.gcol + (int64_t)col * k, b.g[u]);
        if constexpr (HAS_X) {
            const int s = group_bcast<LPR>(lv.c, sub, jj);
            load_vec<float, VEC>(c.xcol + (int64_t)s * k, b.v[u]);
        }
    }
    __device__ __forceinline__ void apply(const Ctx &, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float g = w ? b.g[u][i] * b.w[u] : b.g[u][i];
            if constexpr (HAS_X) g = g * b.v[u][i];
            else g = negate ? -g : g;
            s.acc[i] = s.acc[i] + (valid ? g : 0.f);
        }
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (!(ok && c.col_ok)) return;
        store_vec<float, VEC>(out + row * (int64_t)k + c.col0, s.acc);
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

struct RelArgs {
    const int32_t *rowptr, *colind, *eid, *aux;  // aux: etype (forward) | source ids in sorted order (relation gradient)
    const float *a, *b, *w;                      // forward: x, rel | relation gradient: grad, x
    float *out;
    int64_t m, nnz;
    int k, op, n_rel;
};

// Two gathers per edge (source row + relation row; gradient row + source row): half of csr_spmm's unroll keeps the same
// number of loads in flight, as in gspmm.hip.  The relation gradient of SUB / ADD gathers ONE row per edge and takes the
// whole unroll; MUL, with its second row, half of that.
constexpr int kRelUnroll = 4;
constexpr int kRelGradUnroll1 = 8, kRelGradUnroll2 = kRelGradUnroll1 / 2;

template <int VEC, int LPR>
static int launch_rel(const RelArgs &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    const int64_t tiles = ((int64_t)a.k + (int64_t)LPR * VEC - 1) / ((int64_t)LPR * VEC);
    if (kind == 0) {
        RelSpmmOp<VEC, LPR, kRelUnroll> op{a.eid, a.aux, a.a, a.b, a.w, a.out, a.k, a.op, a.n_rel};
        return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
    }
    if (kind == 1) {
        RelGradOp<VEC, LPR, kRelGradUnroll1, false> op{a.eid, nullptr, a.a, nullptr, a.w, a.out, a.k, a.op == COGDL_HIP_GSPMM_SUB};
        return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
    }
    RelGradOp<VEC, LPR, kRelGradUnroll2, true> op{a.eid, a.aux, a.a, a.b, a.w, a.out, a.k, 0};
    return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
}

template <int VEC>
static int rel_lpr(const RelArgs &a, int kind, int lpr, void *ws, size_t wsb, hipStream_t s) {
    switch (lpr) {
        case 4: return launch_rel<VEC, 4>(a, kind, ws, wsb, s);
        case 8: return launch_rel<VEC, 8>(a, kind, ws, wsb, s);
        case 16: return launch_rel<VEC, 16>(a, kind, ws, wsb, s);
        case 32: return launch_rel<VEC, 32>(a, kind, ws, wsb, s);
        default: return launch_rel<VEC, 64>(a, kind, ws, wsb, s);
    }
}

// Vector width 4 -> 2 -> 1 by the alignment of every gathered / stored table and by k (spmm_geometry).
static int rel_dispatch(const RelArgs &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    uintptr_t v = reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.a);
    if (a.b) v |= reinterpret_cast<uintptr_t>(a.b);
    if (v % 4 != 0) return COGDL_HIP_EALIGN;
    const int align = (v % 16 == 0) ? 16 : (v % 8 == 0) ? 8 : 4;
    const RowGeometry g = spmm_geometry(a.k, a.k, 4, align);
    // The workspace was sized for the 16-byte-aligned geometry; a narrower one needs at most as many floats.
    switch (g.vec) {
        case 4: return rel_lpr<4>(a, kind, g.lpr, ws, wsb, s);
        case 2: return rel_lpr<2>(a, kind, g.lpr, ws, wsb, s);
        default: return rel_lpr<1>(a, kind, g.lpr, ws, wsb, s);
    }
}

static size_t rel_workspace_bytes(int64_t nnz, int64_t k) {
    if (nnz <= 0 || k <= 0) return 0;
    const RowGeometry g = spmm_geometry(k, k, 4, 16);
    return rowreduce_workspace_bytes(nnz, g.tiles * g.vec * g.lpr);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_rel_gspmm_workspace_bytes(int64_t nnz, int64_t k) { return rel_workspace_bytes(nnz, k); }

extern "C" int cogdl_hip_rel_gspmm(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const int32_t *etype,
                                   const float *x, const float *rel, const float *weight, int op, float *out, int64_t m,
                                   int64_t k, int64_t nnz, int64_t n_rel, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    if (m < 0 || k < 0 || nnz < 0 || n_rel < 0) return COGDL_HIP_EINVAL;
    if (m == 0 || k == 0) return COGDL_HIP_OK;
    if (!rowptr || !out || !x || (nnz > 0 && !colind)) return COGDL_HIP_EINVAL;
    if (rel && (!etype || n_rel < 1)) return COGDL_HIP_EINVAL;
    if (op < COGDL_HIP_GSPMM_ADD || op > COGDL_HIP_GSPMM_WMUL) return COGDL_HIP_EINVAL;
    if (k > 0x7fffffff || n_rel > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    const RelArgs a{rowptr, colind, eid, etype, x, rel, weight, out, m, nnz, (int)k, op, (int)n_rel};
    return rel_dispatch(a, 0, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t cogdl_hip_rel_gspmm_grad_rel_workspace_bytes(int64_t nnz, int64_t k) { return rel_workspace_bytes(nnz, k); }

extern "C" int cogdl_hip_rel_gspmm_grad_rel(const int32_t *typeptr, const int32_t *dst_sorted, const int32_t *src_sorted,
                                            const int32_t *eid, const float *grad, const float *x, const float *weight,
                                            int op, float *grad_rel, int64_t n_rel, int64_t k, int64_t nnz,
                                            void *workspace, size_t workspace_bytes, void *stream) {
    if (n_rel < 0 || k < 0 || nnz < 0) return COGDL_HIP_EINVAL;
    if (n_rel == 0 || k == 0) return COGDL_HIP_OK;
    if (!typeptr || !grad_rel || !grad || (nnz > 0 && !dst_sorted)) return COGDL_HIP_EINVAL;
    if (op < COGDL_HIP_GSPMM_ADD || op > COGDL_HIP_GSPMM_MUL) return COGDL_HIP_EINVAL;
    const bool mul = op == COGDL_HIP_GSPMM_MUL;
    if (mul && (!x || (nnz > 0 && !src_sorted))) return COGDL_HIP_EINVAL;
    if (k > 0x7fffffff || n_rel > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    const RelArgs a{typeptr, dst_sorted, eid, mul ? src_sorted : nullptr, grad, mul ? x : nullptr, weight, grad_rel, n_rel, nnz,
                    (int)k, op, (int)n_rel};
    return rel_dispatch(a, mul ? 2 : 1, workspace, workspace_bytes, (hipStream_t)stream);
}
