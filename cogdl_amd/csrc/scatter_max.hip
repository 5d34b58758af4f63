// scatter_max.hip -- neighbourhood max aggregation (GraphSAGE MaxAggregator) for gfx950.
// Replaces cogdl/operators/scatter_max/scatter_max.cu:5-75.
// forward : out[r,c] = max_{e in row r} feat[colind[e],c], max_id[r,c] = colind of the FIRST
//           maximum in CSR order; empty row -> 0 / -1.  (The reference starts from FLT_MIN --
//           the smallest positive float -- so all-negative rows return 1.18e-38 with an
//           uninitialised argmax; that is not reproduced.)  Non-finite values: out = the maximum over the row's
//           non-NaN values (+inf and -inf are ordinary values), max_id = the colind of its first occurrence; a NaN never
//           wins over a number, wherever it stands in the row.  Only a column whose values in the row are ALL NaN gives
//           NaN, with the first edge's colind.
// backward: grad_src[max_id[r,c], c] += grad[r,c] into a buffer zeroed here (the reference
//           accumulates into torch::empty memory).  fp32 hardware atomics, one per element.
// Same row-group decomposition, coalesced row gathers and long-row path as spmm.hip (engine: rowreduce.h).
#include "rowreduce.h"

namespace cogdl {

// v replaces the accumulator: it is larger, or it is a number and the accumulator is the NaN that a range's first edge
// left there (the first edge of a range is taken unconditionally).  A NaN v never replaces anything.
__device__ __forceinline__ bool beats(float v, float acc) { return !(v <= acc) && v == v; }

// State = (running max, colind of its first occurrence) per column; two edge ranges merge by keeping the
// earlier range's entry on ties, so the chunk-parallel path returns the same argmax as the sequential walk.  A range whose
// state is NaN held nothing but NaN, so the rule of `beats` gives the same result for every placement of the chunk borders.
template <int VEC_, int LPR_, int UNROLL_>
struct ScatterMaxOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, kRec = 2 * VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const float *x;
    float *out;
    int32_t *max_id;
    int k;

    struct Ctx {
        int col0;
        bool col_ok;
        const float *xcol;
    };
    struct State {
        float acc[VEC];
        int id[VEC];
    };
    struct LaneVals {};
    struct Batch {
        float v[UNROLL][VEC];
        int c[UNROLL];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx c;
        c.col0 = (tile * LPR + l) * VEC;
        c.col_ok = c.col0 < k;
        c.xcol = x + (c.col_ok ? c.col0 : 0);
        return c;
    }
    __device__ __forceinline__ void row_load(Ctx &, int64_t, bool) const {}
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s.acc[i] = 0.f;
            s.id[i] = -1;
        }
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &, int64_t) const {}
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &, int,
                                          int) const {
        b.c[u] = col;
        load_vec<float, VEC>(c.xcol + (int64_t)col * k, b.v[u]);
    }
    __device__ __forceinline__ void apply(const Ctx &, State &s, const Batch &b, int u, bool valid, int64_t,
                                          int) const {
        if (valid) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const bool take = (s.id[i] < 0) || beats(b.v[u][i], s.acc[i]);
                s.acc[i] = take ? b.v[u][i] : s.acc[i];
                s.id[i] = take ? b.c[u] : s.id[i];
            }
        }
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (ok && c.col_ok) {
            store_vec<float, VEC>(out + row * (int64_t)k + c.col0, s.acc);
#pragma unroll
            for (int i = 0; i < VEC; ++i) max_id[row * (int64_t)k + c.col0 + i] = s.id[i];
        }
    }
    __device__ __forceinline__ void pack(const State &s, float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            rec[i] = s.acc[i];
            rec[VEC + i] = __int_as_float(s.id[i]);
        }
    }
    __device__ __forceinline__ void unpack(State &s, const float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s.acc[i] = rec[i];
            s.id[i] = __float_as_int(rec[VEC + i]);
        }
    }
    __device__ __forceinline__ void merge(const Ctx &, State &a, const State &b) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const bool take = b.id[i] >= 0 && ((a.id[i] < 0) || beats(b.acc[i], a.acc[i]));
            a.acc[i] = take ? b.acc[i] : a.acc[i];
            a.id[i] = take ? b.id[i] : a.id[i];
        }
    }
};

// Backward as a GATHER over the transposed structure (colptr / rowind from cogdl_hip_csr2csc): source node u sums
// grad[v, c] over its out-edges (u -> v) whose forward winner was u.  No atomics, no zero-fill (every element of
// grad_src is written once), contributions added in ascending v -- the order of the sequential reference loop -- so
// rows up to the long-row threshold are bit-identical to it and the result is the same on every run.  A multi-edge
// (u, v) appears as adjacent CSC entries (the transpose is stable) and counts once, as one winner does.
// Algorithmic bytes per edge: 4 + F * 4 (grad row) + F * 4 (max_id row): twice the forward's.
template <int VEC_, int LPR_, int UNROLL_>
struct ScatterMaxBwdOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *colptr;
    const int32_t *rowind;
    const float *grad;
    const int32_t *max_id;
    float *out;
    int k;

    struct Ctx {
        int col0, row, start;
        bool col_ok;
        const float *gcol;
        const int32_t *mcol;
    };
    struct State { float acc[VEC]; };
    struct LaneVals { int prev; };
    struct Batch {
        float g[UNROLL][VEC];
        int id[UNROLL][VEC];
        bool dup[UNROLL];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx c;
        c.col0 = (tile * LPR + l) * VEC;
        c.col_ok = c.col0 < k;
        const int cc = c.col_ok ? c.col0 : 0;
        c.gcol = grad + cc;
        c.mcol = max_id + cc;
        c.row = -1;
        c.start = 0;
        return c;
    }
    __device__ __forceinline__ void row_load(Ctx &c, int64_t row, bool ok) const {
        c.row = (int)row;
        c.start = ok ? colptr[row] : 0;
    }
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &c, LaneVals &lv, int64_t e) const {
        lv.prev = (e > c.start) ? rowind[e - 1] : -1;  // the entry before e in the same column (multi-edge test)
    }
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        b.dup[u] = group_bcast<LPR>(lv.prev, sub, jj) == col;
        load_vec<float, VEC>(c.gcol + (int64_t)col * k, b.g[u]);
        float t[VEC];
        load_vec<float, VEC>(reinterpret_cast<const float *>(c.mcol) + (int64_t)col * k, t);
#pragma unroll
        for (int i = 0; i < VEC; ++i) b.id[u][i] = __float_as_int(t[i]);
    }
    __device__ __forceinline__ void apply(const Ctx &c, State &s, const Batch &b, int u, bool valid, int64_t,
                                          int) const {
        const bool take = valid && !b.dup[u];
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = s.acc[i] + ((take && b.id[u][i] == c.row) ? b.g[u][i] : 0.f);
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (ok && c.col_ok) store_vec<float, VEC>(out + row * (int64_t)k + c.col0, s.acc);
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

__global__ void scatter_max_bwd_kernel(const float *__restrict__ grad, const int32_t *__restrict__ max_id,
                                       float *__restrict__ grad_src, int64_t total, int k) {
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int32_t id = max_id[idx];
        if (id >= 0) unsafeAtomicAdd(grad_src + (int64_t)id * k + (idx % k), grad[idx]);  // global_atomic_add_f32, no CAS loop
    }
}

static RowGeometry smax_geometry(int64_t k, int align) {
    int vec = (k % 4 == 0 && align >= 16) ? 4 : (k % 2 == 0 && align >= 8) ? 2 : 1;
    const int64_t need = (k + vec - 1) / vec;
    int lpr = 8;
    while (lpr < kWave && lpr < need) lpr <<= 1;
    RowGeometry g;
    g.vec = vec;
    g.lpr = lpr;
    g.tiles = (k + (int64_t)lpr * vec - 1) / ((int64_t)lpr * vec);
    return g;
}

struct SmaxArgs {
    const int32_t *rowptr, *colind;
    const float *x;
    float *out;
    int32_t *max_id;
    int64_t m, k, nnz;
};

template <int VEC, int LPR>
static int launch_smax(const SmaxArgs &a, int64_t tiles, void *ws, size_t wsb, hipStream_t s) {
    ScatterMaxOp<VEC, LPR, 8> op{a.x, a.out, a.max_id, (int)a.k};
    return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
}

template <int VEC>
static int dispatch_smax(const SmaxArgs &a, const RowGeometry &g, void *ws, size_t wsb, hipStream_t s) {
    switch (g.lpr) {
        case 8: return launch_smax<VEC, 8>(a, g.tiles, ws, wsb, s);
        case 16: return launch_smax<VEC, 16>(a, g.tiles, ws, wsb, s);
        case 32: return launch_smax<VEC, 32>(a, g.tiles, ws, wsb, s);
        default: return launch_smax<VEC, 64>(a, g.tiles, ws, wsb, s);
    }
}

struct SmaxBwdArgs {
    const int32_t *colptr, *rowind;
    const float *grad;
    const int32_t *max_id;
    float *out;
    int64_t n_src, k, nnz;
};

template <int VEC, int LPR>
static int launch_smax_bwd(const SmaxBwdArgs &a, int64_t tiles, void *ws, size_t wsb, hipStream_t s) {
    ScatterMaxBwdOp<VEC, LPR, 4> op{a.colptr, a.rowind, a.grad, a.max_id, a.out, (int)a.k};  // two gathers per edge
    return launch_rowreduce(op, a.colptr, a.rowind, a.n_src, a.nnz, tiles, ws, wsb, s);
}

template <int VEC>
static int dispatch_smax_bwd(const SmaxBwdArgs &a, const RowGeometry &g, void *ws, size_t wsb, hipStream_t s) {
    switch (g.lpr) {
        case 8: return launch_smax_bwd<VEC, 8>(a, g.tiles, ws, wsb, s);
        case 16: return launch_smax_bwd<VEC, 16>(a, g.tiles, ws, wsb, s);
        case 32: return launch_smax_bwd<VEC, 32>(a, g.tiles, ws, wsb, s);
        default: return launch_smax_bwd<VEC, 64>(a, g.tiles, ws, wsb, s);
    }
}
}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_scatter_max_workspace_bytes(int64_t nnz, int64_t k) {
    if (nnz <= 0 || k <= 0) return 0;
    const RowGeometry g = smax_geometry(k, 16);
    return rowreduce_workspace_bytes(nnz, g.tiles * 2 * g.vec * g.lpr);
}

extern "C" int cogdl_hip_scatter_max_fwd(const int32_t *rowptr, const int32_t *colind, const float *feat,
                                         float *out, int32_t *max_id, int64_t m, int64_t k, int64_t nnz,
                                         void *workspace, size_t workspace_bytes, void *stream) {
    if (m < 0 || k < 0 || nnz < 0) return COGDL_HIP_EINVAL;
    if (m == 0 || k == 0) return COGDL_HIP_OK;
    if (!rowptr || !feat || !out || !max_id) return COGDL_HIP_EINVAL;
    if (k > 0x7fffffff || nnz > 0x7fffffff) return COGDL_HIP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(out);
    const RowGeometry g = smax_geometry(k, (bits % 16 == 0) ? 16 : (bits % 8 == 0) ? 8 : 4);
    SmaxArgs a{rowptr, colind, feat, out, max_id, m, k, nnz};
    switch (g.vec) {
        case 4: return dispatch_smax<4>(a, g, workspace, workspace_bytes, s);
        case 2: return dispatch_smax<2>(a, g, workspace, workspace_bytes, s);
        default: return dispatch_smax<1>(a, g, workspace, workspace_bytes, s);
    }
}

extern "C" int cogdl_hip_scatter_max_bwd(const float *grad, const int32_t *max_id, float *grad_src, int64_t m,
                                         int64_t k, int64_t n_src, void *stream) {
    if (m < 0 || k < 0 || n_src < 0) return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_src > 0 && k > 0) {
        if (!grad_src) return COGDL_HIP_EINVAL;
        hipError_t e = fill_u32_async(grad_src, 0u, (size_t)n_src * (size_t)k, s);
        if (e != hipSuccess) {
            g_last_hip_error = (int)e;
            return COGDL_HIP_ELAUNCH;
        }
    }
    if (m == 0 || k == 0) return COGDL_HIP_OK;
    if (!grad || !max_id) return COGDL_HIP_EINVAL;
    const int64_t total = m * k;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(scatter_max_bwd_kernel, dim3(blocks), dim3(256), 0, s, grad, max_id, grad_src, total, (int)k);
    return launch_status();
}

extern "C" size_t cogdl_hip_scatter_max_bwd_workspace_bytes(int64_t nnz, int64_t k) {
    if (nnz <= 0 || k <= 0) return 0;
    const RowGeometry g = smax_geometry(k, 16);
    return rowreduce_workspace_bytes(nnz, g.tiles * g.vec * g.lpr);
}

extern "C" int cogdl_hip_scatter_max_bwd_csc(const int32_t *colptr, const int32_t *rowind, const float *grad,
                                             const int32_t *max_id, float *grad_src, int64_t n_src, int64_t k,
                                             int64_t nnz, void *workspace, size_t workspace_bytes, void *stream) {
    if (n_src < 0 || k < 0 || nnz < 0) return COGDL_HIP_EINVAL;
    if (n_src == 0 || k == 0) return COGDL_HIP_OK;
    if (!colptr || !grad_src || (nnz > 0 && (!rowind || !grad || !max_id))) return COGDL_HIP_EINVAL;
    if (k > 0x7fffffff || nnz > 0x7fffffff) return COGDL_HIP_ERANGE;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(max_id) |
                           reinterpret_cast<uintptr_t>(grad_src);
    const RowGeometry g = smax_geometry(k, (bits % 16 == 0) ? 16 : (bits % 8 == 0) ? 8 : 4);
    SmaxBwdArgs a{colptr, rowind, grad, max_id, grad_src, n_src, k, nnz};
    hipStream_t s = (hipStream_t)stream;
    switch (g.vec) {
        case 4: return dispatch_smax_bwd<4>(a, g, workspace, workspace_bytes, s);
        case 2: return dispatch_smax_bwd<2>(a, g, workspace, workspace_bytes, s);
        default: return dispatch_smax_bwd<1>(a, g, workspace, workspace_bytes, s);
    }
}
