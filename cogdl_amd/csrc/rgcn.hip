// rgcn.hip -- the message passing of a relational GCN layer for gfx950, in the two weight regularisations of the paper
// (Schlichtkrull et al., "Modeling Relational Data with Graph Convolutional Networks"): every edge (row <- col) carries a type
// t and its message is the source row times a MATRIX W[t],
//
//     h[v] = SUM_{e: row[e] == v}  w_e * x[col[e]] @ W[type[e]]
//
//   basis           W[t] = SUM_b alpha[t, b] V[b].  The sum over the edges moves in front of V:
//                       Z[v, b, :] = SUM_e w_e alpha[t_e, b] x[col_e, :]          h = Z.view(N, B * in) @ V.view(B * in, out)
//                   so the sparse part is an aggregation into B accumulators per column and the dense part is ONE matmul.
//   block diagonal  W[t] = diag(W[t, 0], .., W[t, B-1]), blocks of bi x bo.  Inside a destination row the edges are ordered by
//                   type, the source rows of a run of one type are summed first and multiplied once:
//                       h[v] = SUM_{runs (v, t)} ( SUM_{e in run} w_e x[col_e] ) @ W[t]
//
// Nothing of size [E, .] is written, nothing scales with n_rel * N, no float atomics: equal from run to run.  fp32.
//
// Kernels
//   basis forward      an Op on the row-reduce engine (rowreduce.h) over the destination-sorted view; the state of a lane is
//                      BP x VEC accumulators (BP = 4 | 8 bases per pass: kRec = BP * VEC fits the engine's piece record as it
//                      is, so hub rows take its chunk path and fixed merge order).  The source row is gathered ONCE per edge;
//                      the lane that owns an edge fetches its BP coefficients w_e * alpha[t_e, b] with the edge's id and they
//                      are broadcast across the lane group with the gather.  More than 8 bases: further passes that re-gather.
//   basis grad x       the transposed law on the same engine over the source-sorted view: one accumulator per owned column, B
//                      gathered rows of the upstream gradient per edge (four loads in flight).
//   basis grad alpha   a kernel of its own over the type-sorted view (rows of E / n_rel edges): a type's edges are cut into
//                      chunks of kChunk edges dealt round-robin to S workgroups, a wave takes an edge, its lanes the columns;
//                      the BP dot products stay lane partials until the workgroup's last chunk, are then reduced across the
//                      lanes and the four waves in a fixed order, and a second kernel adds the S partials in order.
//   bdd forward        one wave per destination row (one 64-lane workgroup: its barrier is a wave barrier): the lanes sum the
//                      source rows of a (row, type) run in registers (columns lane, lane + 64, ..), put the sum through LDS,
//                      and every lane accumulates SUM_i s[b * bi + i] * W[t, b, i, o] for its output columns; W is read
//                      coalesced over o and served by the L2.  Four gathers in flight.  The gradient of x is the same kernel
//                      over the source-sorted view with the blocks transposed and the upstream gradient gathered.
//   bdd grad W         over the type-sorted view, a batched outer-product sum per type: workgroup (t, block group, s) stages
//                      the x and g block rows of 8 edges in LDS (w_e folded into x) and its lanes own (b, i, o) entries, up to
//                      16 each; S partials merged in order by the second kernel.  VALU for every block size.
//
// Algorithmic bytes per edge (ids 4 + 4, [+ 4 eid] [+ 4 w]; tables from L2):
//   basis forward 4 k per pass, 2 BP k flops;  grad x 4 B k, 2 B k flops;  grad alpha 4 (B + passes) k, 2 B k flops;
//   bdd forward 4 in (+ 4 in * bo per RUN from L2), 2 in flops per edge + 2 in * bo per run;  grad W 4 (in + out), 2 in * bo.
#include "rowreduce.h"

namespace cogdl {

// ---------------------------------------------------------------------------------------------------------------- basis forward
template <int VEC_, int LPR_, int BP_>
struct RgcnBasisOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = 4, BP = BP_, kRec = BP_ * VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *eid;    // CSR position -> edge id of etype / weight (NULL: identity)
    const int32_t *etype;  // [E] in the caller's edge order
    const float *x;        // [n_src, k]
    const float *alpha;    // [n_rel, n_bases], or NULL: the identity (n_bases == n_rel)
    const float *w;        // [E] or NULL
    float *out;            // [m, n_bases, k]
    int k, n_rel, n_bases;
    int b0;  // first base of this pass

    struct Ctx {
        int col0;
        bool col_ok;
        const float *xcol;
    };
    struct State { float acc[BP][VEC]; };
    struct LaneVals { float c[BP]; };
    struct Batch {
        float v[UNROLL][VEC];
        float c[UNROLL][BP];
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
        for (int b = 0; b < BP; ++b)
#pragma unroll
            for (int i = 0; i < VEC; ++i) s.acc[b][i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    // The coefficients of edge e for the bases of this pass, by the lane that owns the edge (types are clamped into
    // [0, n_rel): a bad id gives a wrong number, never a read outside alpha).
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &lv, int64_t e) const {
        const int id = eid ? eid[e] : (int)e;
        const float we = w ? w[id] : 1.f;
        const int t = min(max(etype[id], 0), n_rel - 1);
#pragma unroll
        for (int b = 0; b < BP; ++b) {
            const int bb = b0 + b;
            float c = 0.f;
            if (bb < n_bases) c = alpha ? we * alpha[(int64_t)t * n_bases + bb] : (t == bb ? we : 0.f);
            lv.c[b] = c;
        }
    }
    __device__ __forceinline__ void fetch(const Ctx &c, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        load_vec<float, VEC>(c.xcol + (int64_t)col * k, b.v[u]);
#pragma unroll
        for (int q = 0; q < BP; ++q) b.c[u][q] = group_bcast<LPR>(lv.c[q], sub, jj);
    }
    __device__ __forceinline__ void apply(const Ctx &, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
#pragma unroll
        for (int q = 0; q < BP; ++q)
#pragma unroll
            for (int i = 0; i < VEC; ++i) s.acc[q][i] = s.acc[q][i] + (valid ? b.c[u][q] * b.v[u][i] : 0.f);
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &c, const State &s, int64_t row, bool ok) const {
        if (!(ok && c.col_ok)) return;
#pragma unroll
        for (int q = 0; q < BP; ++q)
            if (b0 + q < n_bases) store_vec<float, VEC>(out + (row * n_bases + b0 + q) * (int64_t)k + c.col0, s.acc[q]);
    }
    __device__ __forceinline__ void pack(const State &s, float (&rec)[kRec]) const {
#pragma unroll
        for (int q = 0; q < BP; ++q)
#pragma unroll
            for (int i = 0; i < VEC; ++i) rec[q * VEC + i] = s.acc[q][i];
    }
    __device__ __forceinline__ void unpack(State &s, const float (&rec)[kRec]) const {
#pragma unroll
        for (int q = 0; q < BP; ++q)
#pragma unroll
            for (int i = 0; i < VEC; ++i) s.acc[q][i] = rec[q * VEC + i];
    }
    __device__ __forceinline__ void merge(const Ctx &, State &a, const State &b) const {
#pragma unroll
        for (int q = 0; q < BP; ++q)
#pragma unroll
            for (int i = 0; i < VEC; ++i) a.acc[q][i] += b.acc[q][i];
    }
};

// ----------------------------------------------------------------------------------------------------------------- basis grad x
// Rows = sources, the engine's column array = the DESTINATION of every edge: gx[u, :] = SUM_e w_e SUM_b alpha[t_e, b] gz[row_e, b, :].
template <int VEC_, int LPR_>
struct RgcnBasisGradXOp {
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = 4, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const int32_t *eid;
    const int32_t *etype;
    const float *gz;     // [m, n_bases, k]
    const float *alpha;  // [n_rel, n_bases] or NULL (identity)
    const float *w;
    float *out;  // [n_src, k]
    int k, n_rel, n_bases;

    struct Ctx {
        int col0;
        bool col_ok;
        const float *gcol;
    };
    struct State { float acc[VEC]; };
    struct LaneVals {
        int t;
        float w;
    };
    struct Batch {
        int col[UNROLL], t[UNROLL];
        float w[UNROLL];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx c;
        c.col0 = (tile * LPR + l) * VEC;
        c.col_ok = c.col0 < k;
        c.gcol = gz + (c.col_ok ? c.col0 : 0);
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
        lv.t = min(max(etype[id], 0), n_rel - 1);
    }
    __device__ __forceinline__ void fetch(const Ctx &, Batch &b, int u, int col, int64_t, const LaneVals &lv, int sub,
                                          int jj) const {
        b.col[u] = col;
        b.t[u] = group_bcast<LPR>(lv.t, sub, jj);
        b.w[u] = group_bcast<LPR>(lv.w, sub, jj);
    }
    // The B rows of one edge: four loads in flight, added in base order.
    __device__ __forceinline__ void apply(const Ctx &c, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;  // (group-uniform)
        const float *g = c.gcol + (int64_t)b.col[u] * n_bases * k;
        if (!alpha) {
            float v[VEC];
            load_vec<float, VEC>(g + (int64_t)b.t[u] * k, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) s.acc[i] = s.acc[i] + b.w[u] * v[i];
            return;
        }
        const float *a = alpha + (int64_t)b.t[u] * n_bases;
        for (int q0 = 0; q0 < n_bases; q0 += 4) {
            float v[4][VEC], cf[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int bb = min(q0 + q, n_bases - 1);
                load_vec<float, VEC>(g + (int64_t)bb * k, v[q]);
                cf[q] = (q0 + q < n_bases) ? b.w[u] * a[bb] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < VEC; ++i) s.acc[i] = s.acc[i] + cf[q] * v[q][i];
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

struct BasisArgs {
    const int32_t *rowptr, *colind, *eid, *etype;
    const float *table, *alpha, *w;  // table: x (forward) | gz (grad x)
    float *out;
    int64_t m, nnz;
    int k, n_rel, n_bases;
};
constexpr int kBasisPass = 8;  // bases per pass of the forward (BP = 4 for a pass of at most 4)
constexpr int kMaxBases = 32;

template <int VEC, int LPR>
static int launch_basis(const BasisArgs &a, bool grad_x, void *ws, size_t wsb, hipStream_t s) {
    const int64_t tiles = ((int64_t)a.k + (int64_t)LPR * VEC - 1) / ((int64_t)LPR * VEC);
    if (grad_x) {
        RgcnBasisGradXOp<VEC, LPR> op{a.eid, a.etype, a.table, a.alpha, a.w, a.out, a.k, a.n_rel, a.n_bases};
        return launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
    }
    for (int b0 = 0; b0 < a.n_bases; b0 += kBasisPass) {  // (the passes share the workspace: stream order)
        int rc;
        if (a.n_bases - b0 <= 4) {
            RgcnBasisOp<VEC, LPR, 4> op{a.eid, a.etype, a.table, a.alpha, a.w, a.out, a.k, a.n_rel, a.n_bases, b0};
            rc = launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
        } else {
            RgcnBasisOp<VEC, LPR, 8> op{a.eid, a.etype, a.table, a.alpha, a.w, a.out, a.k, a.n_rel, a.n_bases, b0};
            rc = launch_rowreduce(op, a.rowptr, a.colind, a.m, a.nnz, tiles, ws, wsb, s);
        }
        if (rc != COGDL_HIP_OK) return rc;
    }
    return COGDL_HIP_OK;
}

template <int VEC>
static int basis_lpr(const BasisArgs &a, bool grad_x, int lpr, void *ws, size_t wsb, hipStream_t s) {
    switch (lpr) {
        case 4: return launch_basis<VEC, 4>(a, grad_x, ws, wsb, s);
        case 8: return launch_basis<VEC, 8>(a, grad_x, ws, wsb, s);
        case 16: return launch_basis<VEC, 16>(a, grad_x, ws, wsb, s);
        case 32: return launch_basis<VEC, 32>(a, grad_x, ws, wsb, s);
        default: return launch_basis<VEC, 64>(a, grad_x, ws, wsb, s);
    }
}

// Vector width 4 -> 2 -> 1 by the alignment of the gathered and the stored table and by k (spmm_geometry), as relspmm.hip.
static int basis_dispatch(const BasisArgs &a, bool grad_x, void *ws, size_t wsb, hipStream_t s) {
    const uintptr_t v = reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.table);
    if (v % 4 != 0) return COGDL_HIP_EALIGN;
    const int align = (v % 16 == 0) ? 16 : (v % 8 == 0) ? 8 : 4;
    const RowGeometry g = spmm_geometry(a.k, a.k, 4, align);
    switch (g.vec) {
        case 4: return basis_lpr<4>(a, grad_x, g.lpr, ws, wsb, s);
        case 2: return basis_lpr<2>(a, grad_x, g.lpr, ws, wsb, s);
        default: return basis_lpr<1>(a, grad_x, g.lpr, ws, wsb, s);
    }
}

// Sized for the widest record (8 bases per pass) at the 16-byte-aligned geometry; a narrower one needs at most as many floats.
static size_t basis_workspace_bytes(int64_t nnz, int64_t k) {
    if (nnz <= 0 || k <= 0) return 0;
    const RowGeometry g = spmm_geometry(k, k, 4, 16);
    return rowreduce_workspace_bytes(nnz, g.tiles * g.vec * g.lpr * kBasisPass);
}

// ------------------------------------------------------------------------------------------------- type-sorted views: the slices
// A type's edges [typeptr[t], typeptr[t + 1]) are cut into chunks of `chunk` edges; workgroup s of the type takes the chunks
// s, s + S, s + 2 S, ..  S depends on (nnz, n_rel) and the record size only, never on the data: a fixed summation order.
constexpr int kAlphaChunk = 64;  // grad alpha: 16 edges per wave and chunk
constexpr int kGradWChunk = 8;   // grad W: the edges staged in LDS at a time
constexpr int kMaxSlices = 32;
constexpr int64_t kMaxPartialBytes = (int64_t)64 << 20;

static int type_slices(int64_t nnz, int64_t n_rel, int chunk, int64_t rec_floats) {
    int64_t s = (2 * nnz + n_rel * chunk * 4 - 1) / (n_rel * chunk * 4);  // ~ two workgroups' worth of 4 chunks per average type
    s = std::min<int64_t>(s, kMaxSlices);
    s = std::min<int64_t>(s, kMaxPartialBytes / std::max<int64_t>(1, n_rel * rec_floats * 4));
    return (int)std::max<int64_t>(s, 1);
}

// out[i] = SUM_s partial[(i / rec) * S + s][i % rec], s ascending.
__global__ __launch_bounds__(256) void rgcn_merge_slices_kernel(const float *__restrict__ partial, float *__restrict__ out,
                                                                int64_t n, int rec, int S) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = i / rec;
    const int c = (int)(i - r * rec);
    const float *p = partial + r * S * (int64_t)rec + c;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += p[(int64_t)s * rec];
    out[i] = acc;
}

// ------------------------------------------------------------------------------------------------------------ basis grad alpha
// galpha[t, b] = SUM_{e of type t} w_e <x[col_e, :], gz[row_e, b, :]>.  Workgroup (t, s), 4 waves: wave q takes the edges q,
// q + 4, .. of each of the workgroup's chunks, lane l the columns l, l + 64, ..; acc[b] stays a lane partial until the end.
template <int BP>
__global__ __launch_bounds__(256) void rgcn_basis_grad_alpha_kernel(const int32_t *__restrict__ typeptr,
                                                                    const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                                                    const int32_t *__restrict__ eid, const float *__restrict__ x,
                                                                    const float *__restrict__ gz, const float *__restrict__ w,
                                                                    float *__restrict__ partial, int k, int n_bases, int b0, int S) {
    __shared__ float red[4][BP];
    const int t = blockIdx.x, s = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int lo = typeptr[t], hi = typeptr[t + 1];
    float acc[BP];
#pragma unroll
    for (int b = 0; b < BP; ++b) acc[b] = 0.f;
    for (int64_t c0 = (int64_t)lo + (int64_t)s * kAlphaChunk; c0 < hi; c0 += (int64_t)S * kAlphaChunk) {
        const int c1 = (int)min((int64_t)hi, c0 + kAlphaChunk);
        for (int j = (int)c0 + wave; j < c1; j += 4) {
            const float we = w ? w[eid ? eid[j] : j] : 1.f;
            const float *xr = x + (int64_t)src[j] * k;
            const float *gr = gz + ((int64_t)dst[j] * n_bases + b0) * k;
            for (int c = lane; c < k; c += kWave) {
                const float xv = we * xr[c];
#pragma unroll
                for (int b = 0; b < BP; ++b) {
                    const int bb = min(b, n_bases - b0 - 1);  // (a pass of fewer than BP bases re-reads its last one: unused)
                    acc[b] = acc[b] + xv * gr[(int64_t)bb * k + c];
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < BP; ++b) {
        const float v = group_sum<kWave>(acc[b]);
        if (lane == 0) red[wave][b] = v;
    }
    __syncthreads();
    if (threadIdx.x < BP && b0 + (int)threadIdx.x < n_bases) {
        const int b = threadIdx.x;
        partial[((int64_t)t * S + s) * n_bases + b0 + b] = ((red[0][b] + red[1][b]) + red[2][b]) + red[3][b];
    }
}

// --------------------------------------------------------------------------------------------------------- block-diagonal forward
// One wave per row of the (row, type)-sorted view.  NT = column tiles of 64 per lane, for max(in, out).
//   col   [E] gathered row of every edge in sorted order;   typ [E] its type;   eid [E] its edge id (weight) or NULL
//   tab   [n_tab, in] gathered table;   W [n_rel, B, bi, bo];   out [m, out]
template <int NT>
__global__ __launch_bounds__(64) void rgcn_bdd_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      const int32_t *__restrict__ typ, const int32_t *__restrict__ eid,
                                                      const float *__restrict__ tab, const float *__restrict__ W,
                                                      const float *__restrict__ w, float *__restrict__ out, int in, int outw,
                                                      int bi, int bo, int n_rel) {
    constexpr int U = 4;
    __shared__ float srun[NT * kWave];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int start = rowptr[row], end = rowptr[row + 1];
    // this lane's output columns: which block, and where its column of the block starts in W[t] / in the run sum
    int woff[NT], soff[NT];
    float acc[NT], s[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        const int og = min(lane + q * kWave, outw - 1);
        const int b = og / bo;
        woff[q] = b * bi * bo + (og - b * bo);
        soff[q] = b * bi;
        acc[q] = 0.f;
        s[q] = 0.f;
    }
    const int64_t wsz = (int64_t)(in / bi) * bi * bo;  // floats of one type's blocks
    auto flush = [&](int t) {  // acc += (run sum) @ W[t], then clear the run sum
#pragma unroll
        for (int q = 0; q < NT; ++q) srun[q * kWave + lane] = s[q];
        __syncthreads();  // (one wave per workgroup)
        const float *Wt = W + (int64_t)t * wsz;
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            if (lane + q * kWave < outw) {
                const float *wp = Wt + woff[q];
                const float *sp = srun + soff[q];
                float a = acc[q];
                for (int i = 0; i < bi; ++i) a = a + sp[i] * wp[(int64_t)i * bo];
                acc[q] = a;
            }
            s[q] = 0.f;
        }
        __syncthreads();
    };
    int cur_t = -1;
    for (int j = start; j < end; j += U) {
        int c[U], t[U];
        float we[U], v[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jj = min(j + u, end - 1);
            c[u] = col[jj];
            t[u] = min(max(typ[jj], 0), n_rel - 1);  // (clamped as in the basis ops: a bad id gives a wrong number, never a read outside W)
            we[u] = w ? w[eid ? eid[jj] : jj] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float *r = tab + (int64_t)c[u] * in;
#pragma unroll
            for (int q = 0; q < NT; ++q) v[u][q] = r[min(lane + q * kWave, in - 1)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (j + u < end) {  // (wave-uniform, as every branch below)
                if (t[u] != cur_t) {
                    if (cur_t >= 0) flush(cur_t);
                    cur_t = t[u];
                }
#pragma unroll
                for (int q = 0; q < NT; ++q) s[q] = s[q] + we[u] * v[u][q];
            }
        }
    }
    if (cur_t >= 0) flush(cur_t);
#pragma unroll
    for (int q = 0; q < NT; ++q)
        if (lane + q * kWave < outw) out[(int64_t)row * outw + lane + q * kWave] = acc[q];
}

// ---------------------------------------------------------------------------------------------------------- block-diagonal grad W
// gW[t, b, i, o] = SUM_{e of type t} w_e x[col_e, b * bi + i] g[row_e, b * bo + o].  Workgroup (t * n_groups + group, s): the
// group holds nb consecutive blocks (nb * bi * bo <= 4096 entries, NA <= 16 per lane).  Per chunk of 8 edges the block rows of
// x (times w_e) and g go through LDS: at most 512 floats each per edge.
constexpr int kGradWEntries = 4096;
template <int NA>
__global__ __launch_bounds__(256) void rgcn_bdd_grad_w_kernel(const int32_t *__restrict__ typeptr, const int32_t *__restrict__ src,
                                                              const int32_t *__restrict__ dst, const int32_t *__restrict__ eid,
                                                              const float *__restrict__ x, const float *__restrict__ g,
                                                              const float *__restrict__ w, float *__restrict__ partial, int in,
                                                              int outw, int bi, int bo, int nb, int n_groups, int S) {
    __shared__ float xs[kGradWChunk][512];
    __shared__ float gs[kGradWChunk][512];
    const int t = blockIdx.x / n_groups, grp = blockIdx.x - t * n_groups, s = blockIdx.y;
    const int n_blocks = in / bi;
    const int b_first = grp * nb;
    const int nbl = min(nb, n_blocks - b_first);  // blocks of this group
    const int entries = nbl * bi * bo;
    const int xw = nbl * bi, gw = nbl * bo;  // staged widths (<= 512)
    const int tid = threadIdx.x;
    int xo[NA], go[NA];
    float acc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const int idx = min(a * 256 + tid, entries - 1);
        const int bl = idx / (bi * bo);
        const int rem = idx - bl * bi * bo;
        const int i = rem / bo;
        xo[a] = bl * bi + i;
        go[a] = bl * bo + (rem - i * bo);
        acc[a] = 0.f;
    }
    const int lo = typeptr[t], hi = typeptr[t + 1];
    const int se = tid >> 5, sl = tid & 31;  // staging: 32 lanes per edge
    for (int64_t c0 = (int64_t)lo + (int64_t)s * kGradWChunk; c0 < hi; c0 += (int64_t)S * kGradWChunk) {
        const int ce = (int)min((int64_t)kGradWChunk, hi - c0);
        if (se < ce) {
            const int j = (int)c0 + se;
            const float we = w ? w[eid ? eid[j] : j] : 1.f;
            const float *xr = x + (int64_t)src[j] * in + b_first * bi;
            const float *gr = g + (int64_t)dst[j] * outw + b_first * bo;
            for (int c = sl; c < xw; c += 32) xs[se][c] = we * xr[c];
            for (int c = sl; c < gw; c += 32) gs[se][c] = gr[c];
        }
        __syncthreads();
        for (int e = 0; e < ce; ++e) {
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[a] = acc[a] + xs[e][xo[a]] * gs[e][go[a]];
        }
        __syncthreads();
    }
    // partial[(t, s)][b, i, o]: the record of a type is its whole [B, bi, bo] block set
    float *p = partial + ((int64_t)t * S + s) * ((int64_t)n_blocks * bi * bo) + (int64_t)b_first * bi * bo;
#pragma unroll
    for (int a = 0; a < NA; ++a)
        if (a * 256 + tid < entries) p[a * 256 + tid] = acc[a];
}

static int bdd_group_blocks(int64_t n_blocks, int64_t bi, int64_t bo) {
    return (int)std::min<int64_t>(n_blocks, std::max<int64_t>(1, kGradWEntries / (bi * bo)));
}

}  // namespace cogdl

using namespace cogdl;

static bool basis_args_ok(int64_t m, int64_t k, int64_t nnz, int64_t n_rel, int64_t n_bases) {
    return m >= 0 && k >= 0 && nnz >= 0 && n_rel >= 1 && n_bases >= 1;
}

extern "C" size_t cogdl_hip_rgcn_basis_workspace_bytes(int64_t nnz, int64_t k) { return basis_workspace_bytes(nnz, k); }

extern "C" int cogdl_hip_rgcn_basis_fwd(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const int32_t *etype,
                                        const float *x, const float *alpha, const float *weight, float *z, int64_t m, int64_t k,
                                        int64_t nnz, int64_t n_rel, int64_t n_bases, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    if (!basis_args_ok(m, k, nnz, n_rel, n_bases)) return COGDL_HIP_EINVAL;
    if (m == 0 || k == 0) return COGDL_HIP_OK;
    if (!rowptr || !z || !x || (nnz > 0 && (!colind || !etype))) return COGDL_HIP_EINVAL;
    if (!alpha && n_bases != n_rel) return COGDL_HIP_EINVAL;
    if (n_bases > kMaxBases) return COGDL_HIP_EUNSUPPORTED;
    if (k > 0x7fffffff / kMaxBases || n_rel > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    const BasisArgs a{rowptr, colind, eid, etype, x, alpha, weight, z, m, nnz, (int)k, (int)n_rel, (int)n_bases};
    return basis_dispatch(a, false, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int cogdl_hip_rgcn_basis_grad_x(const int32_t *srcptr, const int32_t *dst_sorted, const int32_t *eid,
                                           const int32_t *etype, const float *grad_z, const float *alpha, const float *weight,
                                           float *grad_x, int64_t n_src, int64_t k, int64_t nnz, int64_t n_rel, int64_t n_bases,
                                           void *workspace, size_t workspace_bytes, void *stream) {
    if (!basis_args_ok(n_src, k, nnz, n_rel, n_bases)) return COGDL_HIP_EINVAL;
    if (n_src == 0 || k == 0) return COGDL_HIP_OK;
    if (!srcptr || !grad_x || !grad_z || (nnz > 0 && (!dst_sorted || !etype))) return COGDL_HIP_EINVAL;
    if (!alpha && n_bases != n_rel) return COGDL_HIP_EINVAL;
    if (n_bases > kMaxBases) return COGDL_HIP_EUNSUPPORTED;
    if (k > 0x7fffffff / kMaxBases || n_rel > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    const BasisArgs a{srcptr, dst_sorted, eid, etype, grad_z, alpha, weight, grad_x, n_src, nnz, (int)k, (int)n_rel, (int)n_bases};
    return basis_dispatch(a, true, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t cogdl_hip_rgcn_basis_grad_alpha_workspace_bytes(int64_t nnz, int64_t n_rel, int64_t n_bases) {
    if (nnz <= 0 || n_rel <= 0 || n_bases <= 0) return 0;
    return ((size_t)n_rel * type_slices(nnz, n_rel, kAlphaChunk, n_bases) * n_bases * sizeof(float) + 255) / 256 * 256;
}

extern "C" int cogdl_hip_rgcn_basis_grad_alpha(const int32_t *typeptr, const int32_t *src_sorted, const int32_t *dst_sorted,
                                               const int32_t *eid, const float *x, const float *grad_z, const float *weight,
                                               float *grad_alpha, int64_t n_rel, int64_t n_bases, int64_t k, int64_t nnz,
                                               void *workspace, size_t workspace_bytes, void *stream) {
    if (n_rel < 1 || n_bases < 1 || k < 1 || nnz < 1) return COGDL_HIP_EINVAL;
    if (!typeptr || !src_sorted || !dst_sorted || !x || !grad_z || !grad_alpha) return COGDL_HIP_EINVAL;
    if (n_bases > kMaxBases) return COGDL_HIP_EUNSUPPORTED;
    if (k > 0x7fffffff / kMaxBases || n_rel > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    if (!workspace || workspace_bytes < cogdl_hip_rgcn_basis_grad_alpha_workspace_bytes(nnz, n_rel, n_bases))
        return COGDL_HIP_EWORKSPACE;
    if (!aligned_to(workspace, 4)) return COGDL_HIP_EALIGN;
    const int S = type_slices(nnz, n_rel, kAlphaChunk, n_bases);
    if (S > 65535) return COGDL_HIP_ERANGE;
    float *partial = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_rel, (unsigned)S);
    for (int b0 = 0; b0 < n_bases; b0 += kBasisPass) {
        if (n_bases - b0 <= 4)
            hipLaunchKernelGGL((rgcn_basis_grad_alpha_kernel<4>), grid, dim3(256), 0, st, typeptr, src_sorted, dst_sorted, eid, x,
                               grad_z, weight, partial, (int)k, (int)n_bases, b0, S);
        else
            hipLaunchKernelGGL((rgcn_basis_grad_alpha_kernel<8>), grid, dim3(256), 0, st, typeptr, src_sorted, dst_sorted, eid, x,
                               grad_z, weight, partial, (int)k, (int)n_bases, b0, S);
    }
    const int64_t n = n_rel * n_bases;
    hipLaunchKernelGGL(rgcn_merge_slices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partial, grad_alpha, n,
                       (int)n_bases, S);
    return launch_status();
}

static int bdd_shape_ok(int64_t n_blocks, int64_t bi, int64_t bo) {
    if (n_blocks < 1 || bi < 1 || bo < 1) return COGDL_HIP_EINVAL;
    if (n_blocks * bi > 512 || n_blocks * bo > 512 || bi * bo > kGradWEntries) return COGDL_HIP_EUNSUPPORTED;
    return COGDL_HIP_OK;
}

extern "C" int cogdl_hip_rgcn_bdd_fwd(const int32_t *rowptr, const int32_t *col_sorted, const int32_t *type_sorted,
                                      const int32_t *eid, const float *table, const float *blocks, const float *weight, float *out,
                                      int64_t m, int64_t nnz, int64_t n_rel, int64_t n_blocks, int64_t bi, int64_t bo,
                                      void *stream) {
    if (m < 0 || nnz < 0 || n_rel < 1) return COGDL_HIP_EINVAL;
    const int rc = bdd_shape_ok(n_blocks, bi, bo);
    if (rc != COGDL_HIP_OK) return rc;
    if (m == 0) return COGDL_HIP_OK;
    if (!rowptr || !out || !table || !blocks || (nnz > 0 && (!col_sorted || !type_sorted))) return COGDL_HIP_EINVAL;
    if (m > 0x7fffffff || n_rel > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    const int in = (int)(n_blocks * bi), outw = (int)(n_blocks * bo);
    const int nt = (std::max(in, outw) + kWave - 1) / kWave;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)m);
#define COGDL_RGCN_BDD(NT)                                                                                                    \
    hipLaunchKernelGGL((rgcn_bdd_kernel<NT>), grid, dim3(kWave), 0, st, rowptr, col_sorted, type_sorted, eid, table, blocks, \
                       weight, out, in, outw, (int)bi, (int)bo, (int)n_rel)
    if (nt <= 1) COGDL_RGCN_BDD(1);
    else if (nt <= 2) COGDL_RGCN_BDD(2);
    else if (nt <= 4) COGDL_RGCN_BDD(4);
    else COGDL_RGCN_BDD(8);
#undef COGDL_RGCN_BDD
    return launch_status();
}

extern "C" size_t cogdl_hip_rgcn_bdd_grad_w_workspace_bytes(int64_t nnz, int64_t n_rel, int64_t n_blocks, int64_t bi,
                                                            int64_t bo) {
    if (nnz <= 0 || n_rel <= 0 || bdd_shape_ok(n_blocks, bi, bo) != COGDL_HIP_OK) return 0;
    const int64_t rec = n_blocks * bi * bo;
    return ((size_t)n_rel * type_slices(nnz, n_rel, kGradWChunk, rec) * rec * sizeof(float) + 255) / 256 * 256;
}

extern "C" int cogdl_hip_rgcn_bdd_grad_w(const int32_t *typeptr, const int32_t *src_sorted, const int32_t *dst_sorted,
                                         const int32_t *eid, const float *x, const float *grad, const float *weight,
                                         float *grad_blocks, int64_t n_rel, int64_t n_blocks, int64_t bi, int64_t bo, int64_t nnz,
                                         void *workspace, size_t workspace_bytes, void *stream) {
    if (n_rel < 1 || nnz < 1) return COGDL_HIP_EINVAL;
    const int rc = bdd_shape_ok(n_blocks, bi, bo);
    if (rc != COGDL_HIP_OK) return rc;
    if (!typeptr || !src_sorted || !dst_sorted || !x || !grad || !grad_blocks) return COGDL_HIP_EINVAL;
    if (n_rel > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    if (!workspace || workspace_bytes < cogdl_hip_rgcn_bdd_grad_w_workspace_bytes(nnz, n_rel, n_blocks, bi, bo))
        return COGDL_HIP_EWORKSPACE;
    if (!aligned_to(workspace, 4)) return COGDL_HIP_EALIGN;
    const int64_t rec = n_blocks * bi * bo;
    const int S = type_slices(nnz, n_rel, kGradWChunk, rec);
    const int nb = bdd_group_blocks(n_blocks, bi, bo);
    const int64_t n_groups = (n_blocks + nb - 1) / nb;
    if (n_rel * n_groups > 0x7fffffff || S > 65535) return COGDL_HIP_ERANGE;
    const int na = (int)((std::min<int64_t>(nb, n_blocks) * bi * bo + 255) / 256);
    float *partial = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(n_rel * n_groups), (unsigned)S);
#define COGDL_RGCN_GW(NA)                                                                                                      \
    hipLaunchKernelGGL((rgcn_bdd_grad_w_kernel<NA>), grid, dim3(256), 0, st, typeptr, src_sorted, dst_sorted, eid, x, grad,     \
                       weight, partial, (int)(n_blocks * bi), (int)(n_blocks * bo), (int)bi, (int)bo, nb, (int)n_groups, S)
    if (na <= 1) COGDL_RGCN_GW(1);
    else if (na <= 4) COGDL_RGCN_GW(4);
    else COGDL_RGCN_GW(16);
#undef COGDL_RGCN_GW
    const int64_t n = n_rel * rec;
    hipLaunchKernelGGL(rgcn_merge_slices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partial, grad_blocks, n,
                       (int)rec, S);
    return launch_status();
}
