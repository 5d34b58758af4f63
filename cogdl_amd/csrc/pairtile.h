// pairtile.h -- the 64 x 64 fp32 score tile of two row-major [rows, d] operands, shared by the dense pairwise kernels
// (contrast.hip: log-sum-exp; recon.hip: inner-product decoder loss).  A workgroup of 256 threads stages 64 rows of either side in
// LDS for all of d as [row][k] with a stride of DP + 2 words (DP = 64, 128 or 256, the smallest that holds d), and its four waves
// take the four 32 x 32 blocks of the tile from v_mfma_f32_32x32x2_f32.
#pragma once
#include "common.h"

namespace cogdl {

typedef float pl_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPlTile = 64;                   // rows of either side per step

// rows [row0, row0 + 64) x columns [0, dk) of a row-major [rows, d] matrix -> dst[row][k], zero where the matrix ends.
// A wave stages rows wave, wave + 4, ...: consecutive lanes read consecutive words.
template <int DP>
__device__ __forceinline__ void pl_stage(const float *__restrict__ src, int64_t row0, int64_t rows, int d, int dk, int vec,
                                         float *dst) {
    constexpr int S = DP + 2;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (vec) {  // d % 4 == 0, 16-byte aligned rows
        const int nv = d >> 2;
        for (int r = wave; r < kPlTile; r += 4) {
            const int64_t row = row0 + r;
            for (int v = lane; v < nv; v += kWave) {
                float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (row < rows) x = *reinterpret_cast<const float4 *>(src + row * d + 4 * v);
                float2 *p = reinterpret_cast<float2 *>(dst + r * S + 4 * v);  // (S is even: 8-byte aligned)
                p[0] = make_float2(x.x, x.y);
                p[1] = make_float2(x.z, x.w);
            }
        }
    } else {
        for (int r = wave; r < kPlTile; r += 4) {
            const int64_t row = row0 + r;
            for (int c = lane; c < dk; c += kWave) dst[r * S + c] = (row < rows && c < d) ? src[row * d + c] : 0.0f;
        }
    }
}

// The wave's 32 x 32 block of scores: register r = <owned row 32 oh + j, other row 32 th + 4 half + (r & 3) + 8 (r >> 2)>.
template <int DP>
__device__ __forceinline__ void pl_scores(const float *xs, const float *ys, int dk, int oh, int th, int j, int half,
                                          float (&s)[16]) {
    constexpr int S = DP + 2;
    pl_f32x16 a0, a1;
#pragma unroll
    for (int r = 0; r < 16; ++r) a0[r] = a1[r] = 0.0f;
    const float *ap = ys + (32 * th + j) * S + 2 * half;  // A[i = j][k]: rows of the other tile
    const float *bp = xs + (32 * oh + j) * S + 2 * half;  // B[k][n = j]: owned rows
    for (int kk = 0; kk < dk; kk += 4) {
        const float2 av = *reinterpret_cast<const float2 *>(ap + kk), bv = *reinterpret_cast<const float2 *>(bp + kk);
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, a1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = a0[r] + a1[r];
}

}  // namespace cogdl
