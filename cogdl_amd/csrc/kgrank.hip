// kgrank.hip -- all-entity ranking for knowledge-graph link prediction: for every query row q[i] the number of candidate rows of
// table[N, D] that score above, or equal to, the row of its target -- the rank of the target without a [M, N] score matrix,
// a sort or a read-back per triple (cogdl/wrappers/model_wrapper/link_prediction/triple_link_prediction_mw.py:84-132,
// cogdl/utils/link_prediction_utils.py:187-205).  The score of a pair of rows and the counting rule are kgrank_law.h's.
//
// Four launches on the caller's stream, no atomics on floats, the counters are integers: equal results from run to run.
//   1. kg_rank_target_kernel   one thread per query: st[i] = s(q[i], table[target[i]]) into the workspace (NaN for a target
//                              outside [0, N): nothing is counted for it), counts[i] = 0.
//   2. the sweep               grid (query tiles of 64, entity slices).  A workgroup keeps its 64 queries' counters in
//                              registers while it walks its slice in entity tiles; k is walked in LDS slabs and never split:
//                              one accumulator per (query, candidate) sees every k in ascending order.
//        dot        v_mfma_f32_32x32x2_f32: A = 32 candidate rows of a wave, B = 32 queries, so a lane owns ONE query column
//                   (two with the second B tile) and 16 candidates in its accumulator registers -- three counters per query
//                   per lane.  128 candidates x 64 queries per step, slabs of 64 k, [row][k] LDS tiles with a row stride of
//                   66 words (operand reads touch 64 distinct banks, as in linear_fwd.hip).
//        l1 / cl2   VALU, 64 x 64 per step from [k][row] LDS tiles, a 4 x 4 register tile per thread, slabs of 32 k (cl2: 32
//                   real and the 32 matching imaginary columns).
//      At the end of its slice a workgroup adds its counters into counts with integer atomics (LDS first, then global).
//   3. kg_rank_filter_kernel   one thread per filter entry: the entry's score under the same law, taken out of the bucket it
//                              was counted in.  Lists are sorted per query at this boundary (include/cogdl_hip.h), so a
//                              duplicate is an entry equal to its predecessor and is passed over.
// Every global read is bounds-checked against M, N, D and filt_len; ids that are out of range are passed over, so malformed
// index arrays give wrong numbers, never an access outside the operands.
#include "common.h"
#include "kgrank_law.h"

namespace cogdl {
namespace kg = cogdl_kgrank;

typedef float kg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kKgQT = 64;             // queries per workgroup
constexpr int kKgDotET = 128;         // candidates per step, dot (4 waves x 32)
constexpr int kKgDotKC = 64;          // k slab, dot
constexpr int kKgDotStride = kKgDotKC + 2;
constexpr int kKgVET = 64;            // candidates per step, l1 / cl2
constexpr int kKgVKC = 32;            // k slab, l1 / cl2
constexpr int kKgVStride = kKgVET + 1;
constexpr int kKgWantGroups = 2048;   // workgroups a launch aims for

static int64_t kg_slice_entities(int64_t M, int64_t N, int kind) {
    const int64_t tile = kind == kg::kDot ? kKgDotET : kKgVET;
    const int64_t q_tiles = std::max<int64_t>(1, (M + kKgQT - 1) / kKgQT);
    const int64_t want = std::max<int64_t>(1, kKgWantGroups / q_tiles);
    const int64_t per = (std::max<int64_t>(N, 1) + want - 1) / want;
    int64_t len = (per + tile - 1) / tile * tile;
    // (gridDim.y holds the slices)
    while ((N + len - 1) / len > 65535) len *= 2;
    return len;
}

__global__ void kg_rank_target_kernel(const float *__restrict__ q, const float *__restrict__ table,
                                      const int32_t *__restrict__ target, int64_t M, int64_t N, int64_t D, int kind,
                                      float gamma, float *__restrict__ st, int32_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int64_t t = target[i];
    float s = __builtin_nanf("");
    if (t >= 0 && t < N) s = kg::score(kind, gamma, q + i * D, table + t * D, D);
    st[i] = s;
    counts[3 * i] = 0;
    counts[3 * i + 1] = 0;
    counts[3 * i + 2] = 0;
}

// rows [row0, row0 + ROWS) x columns [k0, k0 + KC) of a row-major [n_rows, D] matrix -> dst, zero where the matrix ends
// (rows at and beyond row_end, columns at and beyond k_end).  TRANSPOSED: dst[k][row] with `stride` words per k, else
// dst[row][k] with `stride` words per row.
template <int ROWS, int KC, bool TRANSPOSED>
__device__ __forceinline__ void kg_stage(const float *__restrict__ src, int64_t row0, int64_t row_end, int64_t D, int64_t k0,
                                         int64_t k_end, float *dst, int stride) {
    for (int idx = threadIdx.x; idx < ROWS * KC; idx += 256) {
        const int r = idx / KC, c = idx % KC;
        const int64_t row = row0 + r, k = k0 + c;
        const float v = (row < row_end && k < k_end) ? src[row * D + k] : 0.0f;
        dst[TRANSPOSED ? c * stride + r : r * stride + c] = v;
    }
}

__device__ __forceinline__ void kg_count(float s, float st, int64_t e, int64_t t, int (&cnt)[3]) {
    const int b = kg::bucket(s, st, e, t);
    cnt[0] += b == 0;
    cnt[1] += b == 1;
    cnt[2] += b == 2;
}

// the workgroup's counters (LDS, [kKgQT][3]) into counts
__device__ __forceinline__ void kg_flush(const int *lds_cnt, int64_t q0, int64_t M, int32_t *__restrict__ counts) {
    for (int idx = threadIdx.x; idx < kKgQT * 3; idx += 256) {
        const int64_t i = q0 + idx / 3;
        const int v = lds_cnt[idx];
        if (i < M && v) atomicAdd(&counts[3 * i + idx % 3], v);
    }
}

__global__ __launch_bounds__(256) void kg_rank_dot_kernel(const float *__restrict__ q, const float *__restrict__ table,
                                                          const int32_t *__restrict__ target, const float *__restrict__ st,
                                                          int64_t M, int64_t N, int64_t D, int64_t slice_len,
                                                          int32_t *__restrict__ counts) {
    __shared__ float qs[kKgQT * kKgDotStride];
    __shared__ float ts[kKgDotET * kKgDotStride];
    __shared__ int lds_cnt[kKgQT * 3];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31;
    const int64_t q0 = (int64_t)blockIdx.x * kKgQT;
    const int64_t e_begin = (int64_t)blockIdx.y * slice_len, e_end = min(N, e_begin + slice_len);
    for (int idx = threadIdx.x; idx < kKgQT * 3; idx += 256) lds_cnt[idx] = 0;
    // this lane's two queries: columns j and 32 + j of the workgroup's tile
    int64_t my_t[2];
    float my_st[2];
    int cnt[2][3] = {{0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int64_t i = q0 + 32 * a + j;
        my_t[a] = i < M ? (int64_t)target[i] : -1;
        my_st[a] = i < M ? st[i] : __builtin_nanf("");
    }
    for (int64_t e_blk = e_begin; e_blk < e_end; e_blk += kKgDotET) {
        kg_f32x16 acc[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][r] = 0.0f;
        for (int64_t k0 = 0; k0 < D; k0 += kKgDotKC) {
            __syncthreads();  // the previous slab's operand reads are done
            kg_stage<kKgQT, kKgDotKC, false>(q, q0, M, D, k0, D, qs, kKgDotStride);
            kg_stage<kKgDotET, kKgDotKC, false>(table, e_blk, e_end, D, k0, D, ts, kKgDotStride);
            __syncthreads();
            const int kc = (int)min((int64_t)kKgDotKC, D - k0);
            const int pairs = (kc + 1) >> 1;  // an odd end is one zero column: fmaf(0, 0, acc) = acc
            const float *a_row = ts + (32 * wave + j) * kKgDotStride + half;  // A[i = j][k = half]: candidate rows
            const float *b_row0 = qs + j * kKgDotStride + half;               // B[k = half][n = j]: query columns
            const float *b_row1 = qs + (32 + j) * kKgDotStride + half;
            for (int p = 0; p < pairs; ++p) {
                const float av = a_row[2 * p], b0 = b_row0[2 * p], b1 = b_row1[2 * p];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
            }
        }
        // C/D map of the 32x32 MFMA: register r holds row (r & 3) + 8 (r >> 2) + 4 half, the lane's column is j
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t e = e_blk + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (e < e_end) {
#pragma unroll
                for (int a = 0; a < 2; ++a) kg_count(acc[a][r], my_st[a], e, my_t[a], cnt[a]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (cnt[a][c]) atomicAdd(&lds_cnt[(32 * a + j) * 3 + c], cnt[a][c]);
    __syncthreads();
    kg_flush(lds_cnt, q0, M, counts);
}

template <int KIND>
__global__ __launch_bounds__(256) void kg_rank_valu_kernel(const float *__restrict__ q, const float *__restrict__ table,
                                                           const int32_t *__restrict__ target, const float *__restrict__ st,
                                                           int64_t M, int64_t N, int64_t D, float gamma, int64_t slice_len,
                                                           int32_t *__restrict__ counts) {
    constexpr int kParts = KIND == kg::kCl2 ? 2 : 1;  // real and imaginary slab
    __shared__ float qs[kParts][kKgVKC * kKgVStride];
    __shared__ float ts[kParts][kKgVKC * kKgVStride];
    __shared__ int lds_cnt[kKgQT * 3];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // candidates tx + 16 b, queries ty + 16 a
    const int64_t q0 = (int64_t)blockIdx.x * kKgQT;
    const int64_t e_begin = (int64_t)blockIdx.y * slice_len, e_end = min(N, e_begin + slice_len);
    const int64_t kdim = KIND == kg::kCl2 ? D / 2 : D;  // the k the sum runs over
    for (int idx = threadIdx.x; idx < kKgQT * 3; idx += 256) lds_cnt[idx] = 0;
    int64_t my_t[4];
    float my_st[4];
    int cnt[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t i = q0 + ty + 16 * a;
        my_t[a] = i < M ? (int64_t)target[i] : -1;
        my_st[a] = i < M ? st[i] : __builtin_nanf("");
        cnt[a][0] = cnt[a][1] = cnt[a][2] = 0;
    }
    for (int64_t e_blk = e_begin; e_blk < e_end; e_blk += kKgVET) {
        float acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
        for (int64_t k0 = 0; k0 < kdim; k0 += kKgVKC) {
            __syncthreads();
#pragma unroll
            for (int part = 0; part < kParts; ++part) {
                kg_stage<kKgQT, kKgVKC, true>(q, q0, M, D, part * kdim + k0, (part + 1) * kdim, qs[part], kKgVStride);
                kg_stage<kKgVET, kKgVKC, true>(table, e_blk, e_end, D, part * kdim + k0, (part + 1) * kdim, ts[part], kKgVStride);
            }
            __syncthreads();
            const int kc = (int)min((int64_t)kKgVKC, kdim - k0);
            for (int kk = 0; kk < kc; ++kk) {
                float qv[kParts][4], tv[kParts][4];
#pragma unroll
                for (int part = 0; part < kParts; ++part)
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        qv[part][a] = qs[part][kk * kKgVStride + ty + 16 * a];
                        tv[part][a] = ts[part][kk * kKgVStride + tx + 16 * a];
                    }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if constexpr (KIND == kg::kCl2)
                            acc[a][b] = kg::cl2_step(acc[a][b], qv[0][a], qv[1][a], tv[0][b], tv[1][b]);
                        else
                            acc[a][b] = kg::l1_step(acc[a][b], qv[0][a], tv[0][b]);
                    }
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t e = e_blk + tx + 16 * b;
            if (e < e_end) {
#pragma unroll
                for (int a = 0; a < 4; ++a) kg_count(kg::finish(KIND, gamma, acc[a][b]), my_st[a], e, my_t[a], cnt[a]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (cnt[a][c]) atomicAdd(&lds_cnt[(ty + 16 * a) * 3 + c], cnt[a][c]);
    __syncthreads();
    kg_flush(lds_cnt, q0, M, counts);
}

__global__ void kg_rank_filter_kernel(const float *__restrict__ q, const float *__restrict__ table,
                                      const int32_t *__restrict__ target, const float *__restrict__ st,
                                      const int32_t *__restrict__ filt_ptr, const int32_t *__restrict__ filt_idx,
                                      int64_t filt_len, int64_t M, int64_t N, int64_t D, int kind, float gamma,
                                      int32_t *__restrict__ counts) {
    const int64_t jx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (jx >= filt_len) return;
    // the query that owns entry jx: the first i with filt_ptr[i + 1] > jx
    int64_t lo = 0, hi = M;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)filt_ptr[mid + 1] <= jx) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= M) return;
    const int64_t i = lo, e = filt_idx[jx], t = target[i];
    if (e < 0 || e >= N || t < 0 || t >= N || e == t) return;
    if (jx > 0 && jx > (int64_t)filt_ptr[i] && (int64_t)filt_idx[jx - 1] == e) return;  // a duplicate of its predecessor
    const float s = kg::score(kind, gamma, q + i * D, table + e * D, D);
    const int b = kg::bucket(s, st[i], e, t);
    if (b >= 0) atomicSub(&counts[3 * i + b], 1);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_kg_rank_workspace_bytes(int64_t M, int64_t N, int64_t D, int kind) {
    (void)N, (void)D, (void)kind;
    return M > 0 ? (size_t)M * sizeof(float) : 0;
}

extern "C" int64_t cogdl_hip_kg_rank_slice_entities(int64_t M, int64_t N, int64_t D, int kind) {
    (void)D;
    if (kg::sizes_status(M, N, 0, kind, 0) != 0) return 0;
    return kg_slice_entities(M, N, kind);
}

extern "C" int cogdl_hip_kg_rank(const float *q, const float *table, const int32_t *target, int64_t M, int64_t N, int64_t D,
                                 int kind, float gamma, const int32_t *filt_ptr, const int32_t *filt_idx, int64_t filt_len,
                                 int32_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = kg::sizes_status(M, N, D, kind, filt_len);
    if (rc != 0) return rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (M == 0) return COGDL_HIP_OK;
    if (!target || !counts || (D > 0 && (!q || (N > 0 && !table)))) return COGDL_HIP_EINVAL;
    if (filt_len > 0 && (!filt_ptr || !filt_idx)) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 4) || !aligned_to(table, 4) || !aligned_to(target, 4) || !aligned_to(counts, 4) ||
        !aligned_to(filt_ptr, 4) || !aligned_to(filt_idx, 4) || !aligned_to(workspace, 4))
        return COGDL_HIP_EALIGN;
    if (!workspace || workspace_bytes < cogdl_hip_kg_rank_workspace_bytes(M, N, D, kind)) return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *st = (float *)workspace;
    hipLaunchKernelGGL(kg_rank_target_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, q, table, target, M, N, D, kind,
                       gamma, st, counts);
    int status = launch_status();
    if (status != COGDL_HIP_OK) return status;
    if (N > 0) {
        const int64_t slice_len = kg_slice_entities(M, N, kind);
        const dim3 grid((unsigned)((M + kKgQT - 1) / kKgQT), (unsigned)((N + slice_len - 1) / slice_len));
        if (kind == kg::kDot)
            hipLaunchKernelGGL(kg_rank_dot_kernel, grid, dim3(256), 0, s, q, table, target, st, M, N, D, slice_len, counts);
        else if (kind == kg::kL1)
            hipLaunchKernelGGL(kg_rank_valu_kernel<kg::kL1>, grid, dim3(256), 0, s, q, table, target, st, M, N, D, gamma,
                               slice_len, counts);
        else
            hipLaunchKernelGGL(kg_rank_valu_kernel<kg::kCl2>, grid, dim3(256), 0, s, q, table, target, st, M, N, D, gamma,
                               slice_len, counts);
        status = launch_status();
        if (status != COGDL_HIP_OK) return status;
    }
    if (filt_len > 0 && N > 0) {
        hipLaunchKernelGGL(kg_rank_filter_kernel, dim3((unsigned)((filt_len + 255) / 256)), dim3(256), 0, s, q, table, target, st,
                           filt_ptr, filt_idx, filt_len, M, N, D, kind, gamma, counts);
        status = launch_status();
    }
    return status;
}
