// polyfilter.hip -- one step of a polynomial graph filter as ONE launch: csr_spmm's row sum with the three-term recurrence's
// linear combination and the filter's running sum folded into the row's final store.
//     t[i,:]   = sum_e val[e] * x[col[e],:]            (csr_spmm's sum, in csr_spmm's order)
//     y        = a * (dst_scale[i] * t) + b * x[i,:] + c1 * z1[i,:] + c2 * z2[i,:]
//     out[i,:] = y;   acc[i,:] += d * y
// This is what the spectral propagation of ProNE and the heat-kernel / PPR / Gaussian filters around it iterate
// (cogdl/utils/prone_utils.py:26-176: a Chebyshev recurrence on an [N, F] matrix; unfused, every sparse product is followed
// by 2-5 elementwise passes over [N, F] tensors).  The functor IS csr_spmm's (spmm_op.h: SpmmOp, EXACT, no epilogue) with
// another row_end, launched with the geometry spmm_auto picks for csr_spmm at this width and the alignment of the least
// aligned of x / out / z1 / z2 / acc: the t of every row up to the exact-row bound is the t cogdl_hip_csr_spmm computes for the
// same operands, bit for bit; a long row's too while z1 / z2 / acc are at least as aligned as x / out (the same geometry: the
// engine's long-row path only merges states, and the combine kernel finishes a long row through the same row_end) -- a less
// aligned z1 / z2 / acc narrows the lanes, the pieces of a long row are cut per lane group, and its sum is re-associated.
// Every product and every sum of the epilogue is a separately rounded fp32 operation, left to right as written
// (-ffp-contract=off, no fmaf); an absent operand is never read and its term is skipped, not multiplied by zero.  fp32
// only; no XCD plan, no sweep layout.
#include "spmm_op.h"

namespace cogdl {

struct FilterEpilogue {
    const float *dst_scale;  // [n] or NULL
    const float *z1, *z2;    // [n, k] or NULL (each may be `out`: a lane reads its columns before it writes them)
    float *acc;              // [n, k] or NULL
    float a, b, c1, c2, d;
};

template <int VEC_, int LPR_, int WMODE>
struct FilterOp : SpmmOp<float, VEC_, LPR_, kDefaultUnroll, WMODE, true> {
    using Base = SpmmOp<float, VEC_, LPR_, kDefaultUnroll, WMODE, true>;
    static constexpr int VEC = VEC_;
    FilterEpilogue f;

    __device__ __forceinline__ void row_end(const typename Base::Ctx &c, const typename Base::State &s, int64_t row, bool ok) const {
        if (!(ok && c.col_ok)) return;
        const int64_t off = row * (int64_t)this->k + c.col0;
        float y[VEC];
        const float ds = f.dst_scale ? f.dst_scale[row] : 1.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) y[i] = f.a * (f.dst_scale ? ds * s.acc[i] : s.acc[i]);
        float v[VEC];
        if (f.b != 0.f) {
            load_vec<float, VEC>(this->x + off, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = y[i] + f.b * v[i];
        }
        if (f.z1) {
            load_vec<float, VEC>(f.z1 + off, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = y[i] + f.c1 * v[i];
        }
        if (f.z2) {
            load_vec<float, VEC>(f.z2 + off, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) y[i] = y[i] + f.c2 * v[i];
        }
        store_vec<float, VEC>(this->out + off, y);
        if (f.acc) {
            load_vec<float, VEC>(f.acc + off, v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] = v[i] + f.d * y[i];
            store_vec<float, VEC>(f.acc + off, v);
        }
    }
};

struct FilterArgs {
    const int32_t *rowptr, *colind;
    const float *val, *x;
    float *out;
    int64_t n, nnz;
    int k;
    FilterEpilogue f;
};

template <int VEC, int LPR, int WMODE>
static int launch_filter(const FilterArgs &a, void *ws, size_t wsb, hipStream_t s) {
    const int64_t tiles = ((int64_t)a.k + (int64_t)LPR * VEC - 1) / ((int64_t)LPR * VEC);
    FilterOp<VEC, LPR, WMODE> op{{a.val, nullptr, a.x, a.out, a.k, a.k, 0, nullptr, {}}, a.f};
    return launch_rowreduce(op, a.rowptr, a.colind, a.n, a.nnz, tiles, ws, wsb, s);
}

template <int VEC, int WMODE>
static int filter_lpr(const FilterArgs &a, int lpr, void *ws, size_t wsb, hipStream_t s) {
    switch (lpr) {  // (the lane groups of dispatch_lpr_u for csr_spmm, the group of 20 included)
        case 4: return launch_filter<VEC, 4, WMODE>(a, ws, wsb, s);
        case 8: return launch_filter<VEC, 8, WMODE>(a, ws, wsb, s);
        case 16: return launch_filter<VEC, 16, WMODE>(a, ws, wsb, s);
        case 20: return launch_filter<VEC, 20, WMODE>(a, ws, wsb, s);
        case 32: return launch_filter<VEC, 32, WMODE>(a, ws, wsb, s);
        default: return launch_filter<VEC, 64, WMODE>(a, ws, wsb, s);
    }
}

template <int WMODE>
static int filter_auto(const FilterArgs &a, void *ws, size_t wsb, hipStream_t s) {
    // csr_spmm's own rule (spmm_op.h: spmm_auto with narrow groups, no plan) for the least aligned of EVERY table a lane
    // touches with load_vec / store_vec: x and out, and z1 / z2 / acc where present (NULL is aligned to anything).  An
    // operand that starts mid-allocation narrows the lanes.  A row up to the exact-row bound is one sequential sum at every
    // width; the pieces of a longer row follow the number of lane groups (rowreduce.h), so only there can the width show.
    const int align = std::min(pointer_alignment(a.x, a.out), std::min(pointer_alignment(a.f.z1, a.f.z2), pointer_alignment(a.f.acc, nullptr)));
    const RowGeometry g = spmm_geometry(a.k, a.k, (int)sizeof(float), align, true, false);
    switch (g.vec) {
        case 4: return filter_lpr<4, WMODE>(a, g.lpr, ws, wsb, s);
        case 2: return filter_lpr<2, WMODE>(a, g.lpr, ws, wsb, s);
        default: return filter_lpr<1, WMODE>(a, g.lpr, ws, wsb, s);
    }
}

static bool overlaps(const void *p, const void *q, size_t bytes) {
    if (!p || !q) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + bytes && b < a + bytes;
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_csr_filter_step(const int32_t *rowptr, const int32_t *colind, const void *val, const void *x, void *out,
                                         int64_t n, int64_t k, int64_t nnz, int dtype, float a, float b, const void *z1, float c1,
                                         const void *z2, float c2, const float *dst_scale, void *acc, float d, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    if (n < 0 || k < 0 || nnz < 0) return COGDL_HIP_EINVAL;
    if (n == 0 || k == 0) return COGDL_HIP_OK;
    if (!rowptr || !x || !out || (nnz > 0 && !colind)) return COGDL_HIP_EINVAL;
    if (k > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    if (dtype != COGDL_HIP_F32) return COGDL_HIP_EUNSUPPORTED;
    const size_t bytes = (size_t)n * (size_t)k * sizeof(float);
    if (overlaps(out, x, bytes) || overlaps(acc, x, bytes) || overlaps(out, acc, bytes)) return COGDL_HIP_EINVAL;
    // out may BE z1 or z2 (same-lane read before write); a shifted overlap would be read after another lane wrote it
    if ((z1 != out && overlaps(out, z1, bytes)) || (z2 != out && overlaps(out, z2, bytes))) return COGDL_HIP_EINVAL;
    if ((z1 != acc && overlaps(acc, z1, bytes)) || (z2 != acc && overlaps(acc, z2, bytes))) return COGDL_HIP_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(out, 4) || !aligned_to(val, 4) || !aligned_to(dst_scale, 4) || !aligned_to(z1, 4) ||
        !aligned_to(z2, 4) || !aligned_to(acc, 4))
        return COGDL_HIP_EALIGN;
    FilterArgs fa{rowptr, colind, (const float *)val, (const float *)x, (float *)out, n, nnz, (int)k,
                  FilterEpilogue{dst_scale, (const float *)z1, (const float *)z2, (float *)acc, a, b, c1, c2, d}};
    hipStream_t s = (hipStream_t)stream;
    return val ? filter_auto<1>(fa, workspace, workspace_bytes, s) : filter_auto<0>(fa, workspace, workspace_bytes, s);
}
