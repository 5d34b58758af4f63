// actq.hip -- activation compression on the device: group-wise stochastic quantisation to 1 / 2 / 4 / 8 bits and back, the
// ReLU whose saved state is one bit per element, and the dropout that saves nothing (the keep bits are regenerated from
// (seed, call)).  The law -- groups, bounds, draws, codes, packing, every float32 expression -- is actq_law.h's, the same the
// host twin (host_actq.cpp) follows: all outputs are equal bit for bit.
//
// Geometry.  A wave handles a TILE of 256 consecutive elements at a time and walks the tiles grid-stride with 64-bit element
// indices; four waves per workgroup, no LDS, no atomics, every store an ordinary vector store of a value the lane computed.
//   actq_quantize_kernel    lane l holds elements 4 l .. 4 l + 3 of the tile (one 16-byte load).  A group of 64 / 128 / 256
//                           elements is an aligned run of WIDTH = 16 / 32 / 64 lanes: min, max and the NaN flag go through a
//                           butterfly of log2(WIDTH) lane exchanges.  One Philox call gives the lane's four draws.  A lane's
//                           four codes are 4 b bits; the 8 / b lanes of a 32-bit word OR their shifted pieces together by
//                           lane exchanges and the first of them stores the dword.  The first lane of a group stores (mn, step).
//   actq_dequantize_kernel  the lane's four codes lie in one word and one group: one dword load (shared by the 8 / b lanes of
//                           the word), one 8-byte metadata load, one 16-byte store.
//   relu_mask_kernel        lane l holds elements l, 64 + l, 128 + l, 192 + l of the tile: four coalesced dword loads, and
//                           each __ballot is one finished 64-bit mask word, stored by one lane.
//   mask_apply_kernel       the same mapping; the mask word is a wave-uniform load.
//   drop_apply_kernel       the quantiser's mapping: one Philox call per float4.
// VEC = false (an operand that is not 16-byte aligned: a view that starts mid-allocation) replaces the 16-byte accesses by four
// dword accesses; the element-to-lane mapping, hence every result, is the same.
#include "common.h"
#include "actq_law.h"

namespace cogdl {
namespace aq = cogdl_actq;

constexpr int kAqThreads = 256;
constexpr int kAqWaves = kAqThreads / kWave;
constexpr int64_t kAqMaxBlocks = 4096;

// elements i0 .. i0 + 3; those at or beyond n read as 0
template <bool VEC>
__device__ __forceinline__ void aq_load4(const float *__restrict__ x, int64_t i0, int64_t n, float (&v)[4]) {
    if (VEC && i0 + 3 < n) {
        const float4 t = *reinterpret_cast<const float4 *>(x + i0);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? x[i0 + k] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void aq_store4(float *__restrict__ y, int64_t i0, int64_t n, const float (&v)[4]) {
    if (VEC && i0 + 3 < n) {
        *reinterpret_cast<float4 *>(y + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) y[i0 + k] = v[k];
    }
}

template <int WIDTH, bool VEC>
__global__ __launch_bounds__(kAqThreads) void actq_quantize_kernel(const float *__restrict__ x, int64_t n, int bits, uint64_t seed,
                                                                   uint64_t call, uint32_t *__restrict__ codes,
                                                                   float *__restrict__ meta) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t tiles = (n + aq::kTile - 1) / aq::kTile, groups = (n + 4 * WIDTH - 1) / (4 * WIDTH);
    const int64_t words = (n * bits + 31) / 32;
    const int P = 8 / bits;  // lanes per code word
    for (int64_t t = (int64_t)blockIdx.x * kAqWaves + wave; t < tiles; t += (int64_t)gridDim.x * kAqWaves) {  // wave-uniform
        const int64_t base = t * aq::kTile, i0 = base + 4 * lane;
        float v[4];
        aq_load4<VEC>(x, i0, n, v);
        aq::Bounds b = aq::empty_bounds();
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) aq::take(b, v[k]);
#pragma unroll
        for (int s = WIDTH / 2; s > 0; s >>= 1) {
            const aq::Bounds o = {__shfl_xor(b.mn, s, kWave), __shfl_xor(b.mx, s, kWave), __shfl_xor(b.bad, s, kWave)};
            b = aq::combine(b, o);
        }
        const aq::Quant q = aq::make_quant(b, bits);
        const cogdl_walk::Draw d = aq::draw4(seed, call, (uint64_t)i0 >> 2);
        uint32_t mine = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) mine |= aq::code_of(q, v[k], aq::word_of(d, k)) << (bits * k);
        uint32_t word = mine << (4 * bits * (lane & (P - 1)));
        for (int s = 1; s < P; s <<= 1) word |= __shfl_xor(word, s, kWave);  // (P is wave-uniform: every lane takes part)
        if ((lane & (P - 1)) == 0) {
            const int64_t wi = base / 32 * bits + lane / P;
            if (wi < words) codes[wi] = word;
        }
        if ((lane & (WIDTH - 1)) == 0) {
            const int64_t g = i0 / (4 * WIDTH);
            if (g < groups) reinterpret_cast<float2 *>(meta)[g] = make_float2(q.mn, q.step);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kAqThreads) void actq_dequantize_kernel(const uint32_t *__restrict__ codes, const float *__restrict__ meta,
                                                                     int64_t n, int bits, int group, float *__restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t tiles = (n + aq::kTile - 1) / aq::kTile;
    const int per = 32 / bits;
    const uint32_t low = (1u << bits) - 1u;
    for (int64_t t = (int64_t)blockIdx.x * kAqWaves + wave; t < tiles; t += (int64_t)gridDim.x * kAqWaves) {
        const int64_t i0 = t * aq::kTile + 4 * lane;
        if (i0 >= n) continue;
        // i0 is a multiple of 4 and per >= 4: the four codes share a word; group is a multiple of 4: they share a group
        const uint32_t word = codes[i0 / per] >> (bits * (int)(i0 % per));
        const float2 m = reinterpret_cast<const float2 *>(meta)[i0 / group];
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = aq::dequant(m.x, m.y, (word >> (bits * k)) & low);
        aq_store4<VEC>(out, i0, n, v);
    }
}

__global__ __launch_bounds__(kAqThreads) void relu_mask_kernel(const float *__restrict__ x, int64_t n, float *__restrict__ y,
                                                               unsigned long long *__restrict__ mask) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t tiles = (n + aq::kTile - 1) / aq::kTile, words = (n + 63) / 64;
    for (int64_t t = (int64_t)blockIdx.x * kAqWaves + wave; t < tiles; t += (int64_t)gridDim.x * kAqWaves) {  // wave-uniform
        const int64_t base = t * aq::kTile;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + 64 * k + lane;
            v[k] = i < n ? x[i] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + 64 * k + lane;
            const unsigned long long bits = __ballot(v[k] > 0.0f);  // (outside a divergent branch: all 64 lanes vote)
            if (i < n) y[i] = aq::relu_of(v[k]);
            if (lane == k && base / 64 + k < words) mask[base / 64 + k] = bits;
        }
    }
}

__global__ __launch_bounds__(kAqThreads) void mask_apply_kernel(const float *__restrict__ g, const unsigned long long *__restrict__ mask,
                                                                int64_t n, float *__restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t tiles = (n + aq::kTile - 1) / aq::kTile;
    for (int64_t t = (int64_t)blockIdx.x * kAqWaves + wave; t < tiles; t += (int64_t)gridDim.x * kAqWaves) {
        const int64_t base = t * aq::kTile;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + 64 * k + lane;
            if (i < n) out[i] = ((mask[i >> 6] >> lane) & 1ull) ? g[i] : 0.0f;  // (i >> 6 <= (n - 1) / 64: inside the mask)
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kAqThreads) void drop_apply_kernel(const float *__restrict__ x, int64_t n, uint64_t seed, uint64_t call,
                                                                uint32_t thresh, float scale, float *__restrict__ y) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t tiles = (n + aq::kTile - 1) / aq::kTile;
    for (int64_t t = (int64_t)blockIdx.x * kAqWaves + wave; t < tiles; t += (int64_t)gridDim.x * kAqWaves) {
        const int64_t i0 = t * aq::kTile + 4 * lane;
        if (i0 >= n) continue;
        float v[4];
        aq_load4<VEC>(x, i0, n, v);
        const cogdl_walk::Draw d = aq::draw4(seed, call, (uint64_t)i0 >> 2);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = aq::drop_of(v[k], aq::word_of(d, k), thresh, scale);
        aq_store4<VEC>(y, i0, n, v);
    }
}

static dim3 aq_grid(int64_t n) {
    const int64_t tiles = (n + aq::kTile - 1) / aq::kTile;
    return dim3((unsigned)std::min<int64_t>((tiles + kAqWaves - 1) / kAqWaves, kAqMaxBlocks));
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_actq_quantize(const float *x, int64_t n, int bits, int group, uint64_t seed, uint64_t call,
                                       uint32_t *codes, float *meta, void *stream) {
    if (aq::sizes_status(n, bits, group)) return COGDL_HIP_EINVAL;
    if (n == 0) return COGDL_HIP_OK;
    if (!x || !codes || !meta) return COGDL_HIP_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(codes, 4) || !aligned_to(meta, 8)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = aq_grid(n), block(kAqThreads);
    const bool vec = aligned_to(x, 16);
#define COGDL_AQ_LAUNCH(WIDTH)                                                                                                     \
    do {                                                                                                                           \
        if (vec)                                                                                                                   \
            hipLaunchKernelGGL((actq_quantize_kernel<WIDTH, true>), grid, block, 0, s, x, n, bits, seed, call, codes, meta);        \
        else                                                                                                                       \
            hipLaunchKernelGGL((actq_quantize_kernel<WIDTH, false>), grid, block, 0, s, x, n, bits, seed, call, codes, meta);       \
    } while (0)
    if (group == 64) COGDL_AQ_LAUNCH(16);
    else if (group == 128) COGDL_AQ_LAUNCH(32);
    else COGDL_AQ_LAUNCH(64);
#undef COGDL_AQ_LAUNCH
    return launch_status();
}

extern "C" int cogdl_hip_actq_dequantize(const uint32_t *codes, const float *meta, int64_t n, int bits, int group, float *out,
                                         void *stream) {
    if (aq::sizes_status(n, bits, group)) return COGDL_HIP_EINVAL;
    if (n == 0) return COGDL_HIP_OK;
    if (!codes || !meta || !out) return COGDL_HIP_EINVAL;
    if (!aligned_to(out, 4) || !aligned_to(codes, 4) || !aligned_to(meta, 8)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (aligned_to(out, 16))
        hipLaunchKernelGGL(actq_dequantize_kernel<true>, aq_grid(n), dim3(kAqThreads), 0, s, codes, meta, n, bits, group, out);
    else
        hipLaunchKernelGGL(actq_dequantize_kernel<false>, aq_grid(n), dim3(kAqThreads), 0, s, codes, meta, n, bits, group, out);
    return launch_status();
}

extern "C" int cogdl_hip_relu_mask(const float *x, int64_t n, float *y, uint64_t *mask, void *stream) {
    if (n < 0) return COGDL_HIP_EINVAL;
    if (n == 0) return COGDL_HIP_OK;
    if (!x || !y || !mask) return COGDL_HIP_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(mask, 8)) return COGDL_HIP_EALIGN;
    hipLaunchKernelGGL(relu_mask_kernel, aq_grid(n), dim3(kAqThreads), 0, (hipStream_t)stream, x, n, y,
                       reinterpret_cast<unsigned long long *>(mask));
    return launch_status();
}

extern "C" int cogdl_hip_mask_apply(const float *g, const uint64_t *mask, int64_t n, float *out, void *stream) {
    if (n < 0) return COGDL_HIP_EINVAL;
    if (n == 0) return COGDL_HIP_OK;
    if (!g || !out || !mask) return COGDL_HIP_EINVAL;
    if (!aligned_to(g, 4) || !aligned_to(out, 4) || !aligned_to(mask, 8)) return COGDL_HIP_EALIGN;
    hipLaunchKernelGGL(mask_apply_kernel, aq_grid(n), dim3(kAqThreads), 0, (hipStream_t)stream, g,
                       reinterpret_cast<const unsigned long long *>(mask), n, out);
    return launch_status();
}

extern "C" int cogdl_hip_drop_apply(const float *x, int64_t n, uint64_t seed, uint64_t call, uint32_t thresh, float scale, float *y,
                                    void *stream) {
    if (n < 0 || thresh > 65536u) return COGDL_HIP_EINVAL;
    if (n == 0) return COGDL_HIP_OK;
    if (!x || !y) return COGDL_HIP_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(y, 4)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (aligned_to(x, 16) && aligned_to(y, 16))
        hipLaunchKernelGGL(drop_apply_kernel<true>, aq_grid(n), dim3(kAqThreads), 0, s, x, n, seed, call, thresh, scale, y);
    else
        hipLaunchKernelGGL(drop_apply_kernel<false>, aq_grid(n), dim3(kAqThreads), 0, s, x, n, seed, call, thresh, scale, y);
    return launch_status();
}
