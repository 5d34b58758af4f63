// disen.hip -- one step of DisenGCN's neighbourhood routing (cogdl/layers/disengcn_layer.py:56-69) for gfx950, fused.  The
// reference gathers h_dst[row] and h_src[col] into two [E, K, d] tensors, multiplies and reduces them to [E, K] scores, takes an
// edge softmax with K channels, gathers h_src[col] a second time, scales it, builds an int64 [K, E, d] index and
// scatter_add_s: [E, K d] traffic six times over and float atomics.  Here, with c, z of shape [N, K d] (channel k = columns
// k d .. (k + 1) d - 1) and over the destination-sorted (CSR) view of the edges,
//
//     s[e, k]   = <c[i, k], z[j, k]> / tau                                    i = the row, j = colind[e]
//     a[i, k]   = z[i, k] + SUM_{e in row i} softmax_{e in row i}(s[e, k]) * z[j, k]
//     out[i, k] = a[i, k] / nrm[i, k],   nrm = ||a[i, k]||_2                  (no epsilon: a zero `a` gives nan, as the reference)
//
// is ONE pass of the row-reduce engine (rowreduce.h): c[i, :] is a per-row operand, z[j, :] is gathered once per edge and used
// for the score and for the accumulation; the score is a dot product over the d columns of a channel -- in the lane when the
// lane's vector holds whole channels, a butterfly over the d / VEC lanes of the channel otherwise.  Per channel the state of an
// online softmax {max, denom}, per column its numerator, one expf per (edge, channel); hub rows are cut into pieces whose
// states merge with the usual rescaling, in a fixed order.  Nothing of size [E, K d] or [E, K] is written.
//
// Backward, given ga = d loss / d a  and  dl[i, k] = <ga[i, k], a[i, k] - z[i, k]>  (both [N, .], from the caller):
//
//     p = exp(s - lse[i, k]),   t = <ga[i, k], z[j, k]>,   r = p * (t - dl[i, k]) / tau
//     g_c[i, k] = SUM_{e in row i} r * z[j, k]                                          (destination-sorted pass)
//     g_z[j, k] = ga[j, k] + SUM_{e: colind[e] == j} (p * ga[i, k] + r * c[i, k])       (source-sorted pass)
//
// Both passes recompute s, p and r from the rows they hold or gather: no per-edge scratch, no edge ids.  The products of a
// dot product are formed with the same operands in the same lane order in all three kernels, so s is the forward's bit for bit.
// fp32 only, no atomics.  Algorithmic bytes per edge (F = K d columns): forward and the g_c pass 4 (colind) + 4 F (the source
// row); the g_z pass 4 + 8 F (the c and ga rows of the destination) + 8 K (its lse and dl).
#include <cmath>

#include "rowreduce.h"

namespace cogdl {

constexpr float kDisenNegInf = -INFINITY;

// A lane holds VEC consecutive columns: NCH whole channels of VEC / NCH columns (GW == 1), or a 1 / GW slice of one channel.
template <int VEC, int GW, int NCH>
struct DisenLane {
    static_assert(NCH == 1 || GW == 1, "several channels per lane: each of them whole");
    static constexpr int DPL = VEC / NCH;  // columns of one channel in this lane
    static constexpr int D = DPL * GW;     // the channel width d

    // r[ch] = <a, b> over the d columns of the lane's channel ch: in-lane in column order, then a butterfly over the channel's
    // GW lanes (every lane of the channel gets the same bits).  Callers keep the operand order (c | ga first, z second).
    static __device__ __forceinline__ void dot(const float (&a)[VEC], const float (&b)[VEC], float (&r)[NCH]) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            float p = a[ch * DPL] * b[ch * DPL];
#pragma unroll
            for (int i = 1; i < DPL; ++i) p = p + a[ch * DPL + i] * b[ch * DPL + i];
            r[ch] = group_sum<GW>(p);
        }
    }
};

// ---------------------------------------------------------------------------------------------------------------- forward
template <int VEC_, int LPR_, int GW, int NCH, int UNROLL_>
struct DisenFwdOp {
    using Lane = DisenLane<VEC_, GW, NCH>;
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, DPL = Lane::DPL;
    static constexpr int kRec = VEC_ + 2 * NCH;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const float *c, *z;      // [n, k]
    float *out;              // [n, k]
    float *nrm, *lse;        // [n, nk]; lse may be NULL
    int k, nk;               // columns K d, channels K
    float tau;

    struct Ctx {
        int col0, chan0;
        bool col_ok;
        const float *zcol;
        float cr[VEC];
    };
    struct State {
        float mx[NCH], den[NCH], num[VEC];
    };
    struct LaneVals {};
    struct Batch {
        float v[UNROLL][VEC];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx x;
        x.col0 = (tile * LPR + l) * VEC;
        x.col_ok = x.col0 < k;  // (k is a multiple of d and a tile of whole channels: uniform over the lanes of a channel)
        const int cc = x.col_ok ? x.col0 : 0;
        x.chan0 = cc / Lane::D;
        x.zcol = z + cc;
#pragma unroll
        for (int i = 0; i < VEC; ++i) x.cr[i] = 0.f;
        return x;
    }
    __device__ __forceinline__ void row_load(Ctx &x, int64_t row, bool ok) const {
        if (ok && x.col_ok) load_vec<float, VEC>(c + row * (int64_t)k + x.col0, x.cr);
    }
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.num[i] = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) s.mx[ch] = kDisenNegInf, s.den[ch] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &, int64_t) const {}
    __device__ __forceinline__ void fetch(const Ctx &x, Batch &b, int u, int col, int64_t, const LaneVals &, int, int) const {
        load_vec<float, VEC>(x.zcol + (int64_t)col * k, b.v[u]);
    }
    // Online softmax with ONE expf per (edge, channel), as GenFwdOp::apply: d = s - max; e = exp(-|d|) rescales the state
    // (d > 0: a new max) or weighs the edge (d <= 0).  |s| <= ||c|| ||z|| / tau stays in the exponent's argument only as a
    // difference: 1 / tau = 100 is finite.
    __device__ __forceinline__ void apply(const Ctx &x, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;  // (uniform over the row's lane group, which holds the channel's lanes)
        float sc[NCH];
        Lane::dot(x.cr, b.v[u], sc);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const float sv = sc[ch] / tau;
            const float d = sv - s.mx[ch];
            const float e = expf(-fabsf(d));
            const bool up = d > 0.f;
            const float rs = up ? e : 1.f, p = up ? 1.f : e;
            s.den[ch] = s.den[ch] * rs + p;
#pragma unroll
            for (int i = 0; i < DPL; ++i) s.num[ch * DPL + i] = s.num[ch * DPL + i] * rs + p * b.v[u][ch * DPL + i];
            s.mx[ch] = up ? sv : s.mx[ch];
        }
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &x, const State &s, int64_t row, bool ok) const {
        if (!(ok && x.col_ok)) return;  // (uniform over the lanes of a channel)
        const int64_t at = row * (int64_t)k + x.col0;
        float a[VEC], o[VEC], sq[NCH];
        load_vec<float, VEC>(z + at, a);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const bool any = s.den[ch] > 0.f;  // a row without edges: z alone
#pragma unroll
            for (int i = 0; i < DPL; ++i)
                a[ch * DPL + i] = any ? a[ch * DPL + i] + s.num[ch * DPL + i] / s.den[ch] : a[ch * DPL + i];
        }
        Lane::dot(a, a, sq);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const float nr = sqrtf(sq[ch]);
#pragma unroll
            for (int i = 0; i < DPL; ++i) o[ch * DPL + i] = a[ch * DPL + i] / nr;
            if (x.col0 % Lane::D == 0 || NCH > 1) {  // the channel's first lane
                const int64_t cat = row * (int64_t)nk + x.chan0 + ch;
                nrm[cat] = nr;
                if (lse) lse[cat] = s.den[ch] > 0.f ? s.mx[ch] + logf(s.den[ch]) : 0.f;
            }
        }
        store_vec<float, VEC>(out + at, o);
    }
    __device__ __forceinline__ void pack(const State &s, float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) rec[i] = s.num[i];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) rec[VEC + ch] = s.mx[ch], rec[VEC + NCH + ch] = s.den[ch];
    }
    __device__ __forceinline__ void unpack(State &s, const float (&rec)[kRec]) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.num[i] = rec[i];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) s.mx[ch] = rec[VEC + ch], s.den[ch] = rec[VEC + NCH + ch];
    }
    // b's edges follow a's.  A state without edges has max = -inf and weight 0 (never exp(-inf + inf)).
    __device__ __forceinline__ void merge(const Ctx &, State &a, const State &b) const {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const float nm = fmaxf(a.mx[ch], b.mx[ch]);
            const float sa = a.mx[ch] == kDisenNegInf ? 0.f : expf(a.mx[ch] - nm);
            const float sb = b.mx[ch] == kDisenNegInf ? 0.f : expf(b.mx[ch] - nm);
            a.den[ch] = a.den[ch] * sa + b.den[ch] * sb;
#pragma unroll
            for (int i = 0; i < DPL; ++i) a.num[ch * DPL + i] = a.num[ch * DPL + i] * sa + b.num[ch * DPL + i] * sb;
            a.mx[ch] = nm;
        }
    }
};

// ------------------------------------------------------------------------------------------- backward: the additive state
template <int VEC>
struct DisenAcc {
    float acc[VEC];
};

// ------------------------------------------------------------------------ backward over the destination-sorted view: g_c
template <int VEC_, int LPR_, int GW, int NCH, int UNROLL_>
struct DisenBwdCOp {
    using Lane = DisenLane<VEC_, GW, NCH>;
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, DPL = Lane::DPL, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const float *c, *z, *ga;  // [n, k]
    const float *lse, *dl;    // [n, nk]
    float *gc;                // [n, k]
    int k, nk;
    float tau;

    struct Ctx {
        int col0, chan0;
        bool col_ok;
        const float *zcol;
        float cr[VEC], gar[VEC], lser[NCH], dlr[NCH];
    };
    using State = DisenAcc<VEC>;
    struct LaneVals {};
    struct Batch {
        float v[UNROLL][VEC];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx x;
        x.col0 = (tile * LPR + l) * VEC;
        x.col_ok = x.col0 < k;
        const int cc = x.col_ok ? x.col0 : 0;
        x.chan0 = cc / Lane::D;
        x.zcol = z + cc;
#pragma unroll
        for (int i = 0; i < VEC; ++i) x.cr[i] = 0.f, x.gar[i] = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) x.lser[ch] = 0.f, x.dlr[ch] = 0.f;
        return x;
    }
    __device__ __forceinline__ void row_load(Ctx &x, int64_t row, bool ok) const {
        if (!(ok && x.col_ok)) return;
        load_vec<float, VEC>(c + row * (int64_t)k + x.col0, x.cr);
        load_vec<float, VEC>(ga + row * (int64_t)k + x.col0, x.gar);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            x.lser[ch] = lse[row * (int64_t)nk + x.chan0 + ch];
            x.dlr[ch] = dl[row * (int64_t)nk + x.chan0 + ch];
        }
    }
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &, int64_t) const {}
    __device__ __forceinline__ void fetch(const Ctx &x, Batch &b, int u, int col, int64_t, const LaneVals &, int, int) const {
        load_vec<float, VEC>(x.zcol + (int64_t)col * k, b.v[u]);
    }
    __device__ __forceinline__ void apply(const Ctx &x, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;
        float sc[NCH], t[NCH];
        Lane::dot(x.cr, b.v[u], sc);
        Lane::dot(x.gar, b.v[u], t);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const float p = expf(sc[ch] / tau - x.lser[ch]);
            const float r = p * (t[ch] - x.dlr[ch]) / tau;
#pragma unroll
            for (int i = 0; i < DPL; ++i) s.acc[ch * DPL + i] = s.acc[ch * DPL + i] + r * b.v[u][ch * DPL + i];
        }
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &x, const State &s, int64_t row, bool ok) const {
        if (!(ok && x.col_ok)) return;
        store_vec<float, VEC>(gc + row * (int64_t)k + x.col0, s.acc);
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

// ----------------------------------------------------------------------------- backward over the source-sorted view: g_z
// Rows = sources j (z[j, :] is the per-row operand), the engine's column of an edge = its destination i: the c and ga rows
// of i and its lse / dl entries are gathered.
template <int VEC_, int LPR_, int GW, int NCH, int UNROLL_>
struct DisenBwdZOp {
    using Lane = DisenLane<VEC_, GW, NCH>;
    static constexpr int VEC = VEC_, LPR = LPR_, UNROLL = UNROLL_, DPL = Lane::DPL, kRec = VEC_;
    static constexpr bool kReduce = true;
    static constexpr int kLds = 0;
    const float *c, *z, *ga;  // [n, k]
    const float *lse, *dl;    // [n, nk]
    float *gz;                // [n, k]
    int k, nk;
    float tau;

    struct Ctx {
        int col0;
        bool col_ok;
        const float *ccol, *gacol, *lcol, *dcol;
        float zr[VEC];
    };
    using State = DisenAcc<VEC>;
    struct LaneVals {};
    struct Batch {
        float cv[UNROLL][VEC], gv[UNROLL][VEC], l[UNROLL][NCH], d[UNROLL][NCH];
    };

    __device__ __forceinline__ Ctx make_ctx(int l, int tile) const {
        Ctx x;
        x.col0 = (tile * LPR + l) * VEC;
        x.col_ok = x.col0 < k;
        const int cc = x.col_ok ? x.col0 : 0;
        x.ccol = c + cc;
        x.gacol = ga + cc;
        x.lcol = lse + cc / Lane::D;
        x.dcol = dl + cc / Lane::D;
#pragma unroll
        for (int i = 0; i < VEC; ++i) x.zr[i] = 0.f;
        return x;
    }
    __device__ __forceinline__ void row_load(Ctx &x, int64_t row, bool ok) const {
        if (ok && x.col_ok) load_vec<float, VEC>(z + row * (int64_t)k + x.col0, x.zr);
    }
    __device__ __forceinline__ void init_zero(State &s) const {
#pragma unroll
        for (int i = 0; i < VEC; ++i) s.acc[i] = 0.f;
    }
    __device__ __forceinline__ void init(const Ctx &, State &s, int64_t, bool) const { init_zero(s); }
    __device__ __forceinline__ void lane_load(const Ctx &, LaneVals &, int64_t) const {}
    __device__ __forceinline__ void fetch(const Ctx &x, Batch &b, int u, int col, int64_t, const LaneVals &, int, int) const {
        load_vec<float, VEC>(x.ccol + (int64_t)col * k, b.cv[u]);
        load_vec<float, VEC>(x.gacol + (int64_t)col * k, b.gv[u]);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            b.l[u][ch] = x.lcol[(int64_t)col * nk + ch];
            b.d[u][ch] = x.dcol[(int64_t)col * nk + ch];
        }
    }
    __device__ __forceinline__ void apply(const Ctx &x, State &s, const Batch &b, int u, bool valid, int64_t, int) const {
        if (!valid) return;
        float sc[NCH], t[NCH];
        Lane::dot(b.cv[u], x.zr, sc);
        Lane::dot(b.gv[u], x.zr, t);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            const float p = expf(sc[ch] / tau - b.l[u][ch]);
            const float r = p * (t[ch] - b.d[u][ch]) / tau;
#pragma unroll
            for (int i = 0; i < DPL; ++i)
                s.acc[ch * DPL + i] = s.acc[ch * DPL + i] + (p * b.gv[u][ch * DPL + i] + r * b.cv[u][ch * DPL + i]);
        }
    }
    __device__ __forceinline__ void chunk_begin(Ctx &, State &, int, int, int, int, int, float *, const LaneVals &) const {}
    __device__ __forceinline__ void batch_end(const Ctx &, State &, int, int, int) const {}
    __device__ __forceinline__ void chunk_end(const Ctx &, State &, int, int) const {}
    __device__ __forceinline__ void row_end(const Ctx &x, const State &s, int64_t row, bool ok) const {
        if (!(ok && x.col_ok)) return;
        const int64_t at = row * (int64_t)k + x.col0;
        float o[VEC];
        load_vec<float, VEC>(ga + at, o);  // a = z + ...: the direct term
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] = o[i] + s.acc[i];
        store_vec<float, VEC>(gz + at, o);
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

struct DisenArgs {
    const int32_t *rowptr, *colind;
    const float *c, *z, *ga, *lse_in, *dl;
    float *out, *nrm, *lse;
    int64_t n, nnz;
    int k, nk, d;
    float tau;
};
enum { kDisenFwd = 0, kDisenBwdC = 1, kDisenBwdZ = 2 };

// One gather per edge in the forward and the g_c pass; two rows and two scalars per edge in the g_z pass.
constexpr int kDisenFwdUnroll = 4, kDisenBwdCUnroll = 4, kDisenBwdZUnroll = 2;

// The geometry of a launch.  vec: the widest of 4 / 2 / 1 floats that the alignment of every table, the row length k and the
// channel width d allow (vec <= d: a channel is whole lanes) -- but d == 2 takes two channels into a 16-byte lane.  A channel
// is gw = d / vec lanes; a row group is lpr >= gw lanes and a column tile lpr * vec columns, a multiple of d: a channel never
// straddles a lane group or a tile.  16-byte lanes pick the group by the row length; the narrow lanes (misaligned tables, odd
// K with d == 2) always take the whole wave.
struct DisenGeo {
    int vec, gw, nch, lpr;
    int64_t tiles;
    int rec_fwd;  // floats of a forward piece record per lane
};
static DisenGeo disen_geometry(int64_t k, int d, int align) {
    DisenGeo g;
    g.vec = 4;
    while (g.vec > 1 && (align % (g.vec * 4) != 0 || k % g.vec != 0 || (g.vec > d && !(g.vec == 4 && d == 2)))) g.vec /= 2;
    g.nch = g.vec > d ? g.vec / d : 1;
    g.gw = g.vec > d ? 1 : d / g.vec;
    g.lpr = kWave;
    if (g.vec == 4) g.lpr = k <= 64 ? 16 : k <= 128 ? 32 : 64;
    g.tiles = (k + (int64_t)g.lpr * g.vec - 1) / ((int64_t)g.lpr * g.vec);
    g.rec_fwd = g.vec + 2 * g.nch;
    return g;
}

template <int VEC, int LPR, int GW, int NCH>
static int launch_disen(const DisenArgs &a, int kind, int64_t tiles, void *ws, size_t wsb, hipStream_t s) {
    static_assert(GW <= LPR, "a channel inside one lane group");
    if (kind == kDisenFwd) {
        DisenFwdOp<VEC, LPR, GW, NCH, kDisenFwdUnroll> op{a.c, a.z, a.out, a.nrm, a.lse, a.k, a.nk, a.tau};
        return launch_rowreduce(op, a.rowptr, a.colind, a.n, a.nnz, tiles, ws, wsb, s);
    }
    if (kind == kDisenBwdC) {
        DisenBwdCOp<VEC, LPR, GW, NCH, kDisenBwdCUnroll> op{a.c, a.z, a.ga, a.lse_in, a.dl, a.out, a.k, a.nk, a.tau};
        return launch_rowreduce(op, a.rowptr, a.colind, a.n, a.nnz, tiles, ws, wsb, s);
    }
    DisenBwdZOp<VEC, LPR, GW, NCH, kDisenBwdZUnroll> op{a.c, a.z, a.ga, a.lse_in, a.dl, a.out, a.k, a.nk, a.tau};
    return launch_rowreduce(op, a.rowptr, a.colind, a.n, a.nnz, tiles, ws, wsb, s);
}

template <int VEC, int GW, int NCH>
static int disen_lpr(const DisenArgs &a, int kind, const DisenGeo &g, void *ws, size_t wsb, hipStream_t s) {
    if constexpr (VEC == 4) {
        if (g.lpr == 16) return launch_disen<VEC, 16, GW, NCH>(a, kind, g.tiles, ws, wsb, s);
        if (g.lpr == 32) return launch_disen<VEC, 32, GW, NCH>(a, kind, g.tiles, ws, wsb, s);
    }
    if (g.lpr == 64) return launch_disen<VEC, 64, GW, NCH>(a, kind, g.tiles, ws, wsb, s);
    return COGDL_HIP_ERANGE;
}

template <int VEC>
static int disen_gw(const DisenArgs &a, int kind, const DisenGeo &g, void *ws, size_t wsb, hipStream_t s) {
    if constexpr (VEC == 4) {
        if (g.nch == 2 && g.gw == 1) return disen_lpr<4, 1, 2>(a, kind, g, ws, wsb, s);
    }
    if (g.nch != 1) return COGDL_HIP_ERANGE;
    switch (g.gw) {  // d = VEC * gw in {2, .., 64}
        case 1:
            if constexpr (VEC >= 2) return disen_lpr<VEC, 1, 1>(a, kind, g, ws, wsb, s);
            break;
        case 2: return disen_lpr<VEC, 2, 1>(a, kind, g, ws, wsb, s);
        case 4: return disen_lpr<VEC, 4, 1>(a, kind, g, ws, wsb, s);
        case 8: return disen_lpr<VEC, 8, 1>(a, kind, g, ws, wsb, s);
        case 16: return disen_lpr<VEC, 16, 1>(a, kind, g, ws, wsb, s);
        case 32:
            if constexpr (VEC <= 2) return disen_lpr<VEC, 32, 1>(a, kind, g, ws, wsb, s);
            break;
        case 64:
            if constexpr (VEC == 1) return disen_lpr<VEC, 64, 1>(a, kind, g, ws, wsb, s);
            break;
    }
    return COGDL_HIP_ERANGE;
}

static bool disen_width_ok(int64_t d) { return d == 2 || d == 4 || d == 8 || d == 16 || d == 32 || d == 64; }

static int disen_dispatch(const DisenArgs &a, int kind, void *ws, size_t wsb, hipStream_t s) {
    uintptr_t v = 0;
    for (const void *p : {(const void *)a.c, (const void *)a.z, (const void *)a.ga, (const void *)a.out})
        v |= reinterpret_cast<uintptr_t>(p);
    uintptr_t w = v;
    for (const void *p : {(const void *)a.lse_in, (const void *)a.dl, (const void *)a.nrm, (const void *)a.lse})
        w |= reinterpret_cast<uintptr_t>(p);
    if (w % 4 != 0) return COGDL_HIP_EALIGN;
    const int align = (v % 16 == 0) ? 16 : (v % 8 == 0) ? 8 : 4;
    const DisenGeo g = disen_geometry(a.k, a.d, align);
    // (the workspace was sized for the widest record of the three vector widths: disen_workspace_bytes)
    switch (g.vec) {
        case 4: return disen_gw<4>(a, kind, g, ws, wsb, s);
        case 2: return disen_gw<2>(a, kind, g, ws, wsb, s);
        default: return disen_gw<1>(a, kind, g, ws, wsb, s);
    }
}

// The largest piece record over the geometries a call may get (the vector width follows the pointers' alignment).
static size_t disen_workspace_bytes(int64_t nnz, int64_t nk, int64_t d, bool fwd) {
    if (nnz <= 0 || nk <= 0 || !disen_width_ok(d) || nk > 0x7fffffff / d) return 0;
    int64_t stride = 0;
    for (int align : {16, 8, 4}) {
        const DisenGeo g = disen_geometry(nk * d, (int)d, align);
        stride = std::max<int64_t>(stride, g.tiles * g.lpr * (fwd ? g.rec_fwd : g.vec));
    }
    return rowreduce_workspace_bytes(nnz, stride);
}

static int disen_check(int64_t n, int64_t nk, int64_t d, int64_t nnz, float tau) {
    if (n < 0 || nk < 0 || d < 0 || nnz < 0 || !(tau > 0.f)) return COGDL_HIP_EINVAL;
    if (!disen_width_ok(d)) return COGDL_HIP_EUNSUPPORTED;
    if (nk > 0x7fffffff / d || n > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    return COGDL_HIP_OK;
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_disen_route_fwd_workspace_bytes(int64_t nnz, int64_t n_channels, int64_t d) {
    return disen_workspace_bytes(nnz, n_channels, d, true);
}

extern "C" int cogdl_hip_disen_route_fwd(const int32_t *rowptr, const int32_t *colind, const float *c, const float *z,
                                         float tau, float *out, float *nrm, float *lse, int64_t n, int64_t n_channels,
                                         int64_t d, int64_t nnz, void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = disen_check(n, n_channels, d, nnz, tau);
    if (rc != COGDL_HIP_OK) return rc;
    if (n == 0 || n_channels == 0) return COGDL_HIP_OK;
    if (!rowptr || !c || !z || !out || !nrm || (nnz > 0 && !colind)) return COGDL_HIP_EINVAL;
    DisenArgs a{};
    a.rowptr = rowptr, a.colind = colind, a.c = c, a.z = z, a.out = out, a.nrm = nrm, a.lse = lse;
    a.n = n, a.nnz = nnz, a.k = (int)(n_channels * d), a.nk = (int)n_channels, a.d = (int)d, a.tau = tau;
    return disen_dispatch(a, kDisenFwd, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t cogdl_hip_disen_route_bwd_c_workspace_bytes(int64_t nnz, int64_t n_channels, int64_t d) {
    return disen_workspace_bytes(nnz, n_channels, d, false);
}

static int disen_bwd(int kind, const int32_t *ptr, const int32_t *ind, const float *c, const float *z, const float *ga,
                     const float *lse, const float *dl, float tau, float *grad, int64_t n, int64_t nk, int64_t d, int64_t nnz,
                     void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = disen_check(n, nk, d, nnz, tau);
    if (rc != COGDL_HIP_OK) return rc;
    if (n == 0 || nk == 0) return COGDL_HIP_OK;
    if (!ptr || !c || !z || !ga || !lse || !dl || !grad || (nnz > 0 && !ind)) return COGDL_HIP_EINVAL;
    DisenArgs a{};
    a.rowptr = ptr, a.colind = ind, a.c = c, a.z = z, a.ga = ga, a.lse_in = lse, a.dl = dl, a.out = grad;
    a.n = n, a.nnz = nnz, a.k = (int)(nk * d), a.nk = (int)nk, a.d = (int)d, a.tau = tau;
    return disen_dispatch(a, kind, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int cogdl_hip_disen_route_bwd_c(const int32_t *rowptr, const int32_t *colind, const float *c, const float *z,
                                           const float *ga, const float *lse, const float *dl, float tau, float *grad_c,
                                           int64_t n, int64_t n_channels, int64_t d, int64_t nnz, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    return disen_bwd(kDisenBwdC, rowptr, colind, c, z, ga, lse, dl, tau, grad_c, n, n_channels, d, nnz, workspace,
                     workspace_bytes, stream);
}

extern "C" size_t cogdl_hip_disen_route_bwd_z_workspace_bytes(int64_t nnz, int64_t n_channels, int64_t d) {
    return disen_workspace_bytes(nnz, n_channels, d, false);
}

extern "C" int cogdl_hip_disen_route_bwd_z(const int32_t *srcptr, const int32_t *dst_sorted, const float *c, const float *z,
                                           const float *ga, const float *lse, const float *dl, float tau, float *grad_z,
                                           int64_t n, int64_t n_channels, int64_t d, int64_t nnz, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    return disen_bwd(kDisenBwdZ, srcptr, dst_sorted, c, z, ga, lse, dl, tau, grad_z, n, n_channels, d, nnz, workspace,
                     workspace_bytes, stream);
}
