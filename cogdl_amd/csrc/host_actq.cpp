// host_actq.cpp -- the host twin of csrc/actq.hip: group-wise stochastic quantisation, the packed ReLU mask and the
// regenerated dropout.  Bounds, draws, codes and every float32 expression are actq_law.h's, the same the kernels follow, so
// for equal inputs every output byte is the GPU's.  OpenMP over tiles of 256 elements (whole groups, whole code words, whole
// mask words); the result does not depend on the number of threads.  No HIP.
#include <cstdint>

#include "../../include/cogdl_host.h"
#include "actq_law.h"

namespace aq = cogdl_actq;

extern "C" int cogdl_host_actq_quantize(const float *x, int64_t n, int bits, int group, uint64_t seed, uint64_t call,
                                        uint32_t *codes, float *meta) {
    if (aq::sizes_status(n, bits, group)) return COGDL_HOST_EINVAL;
    if (n == 0) return COGDL_HOST_OK;
    if (!x || !codes || !meta) return COGDL_HOST_EINVAL;
    const int64_t tiles = (n + aq::kTile - 1) / aq::kTile;
    const int per = 32 / bits;
#pragma omp parallel for schedule(static)
    for (int64_t t = 0; t < tiles; ++t) {
        const int64_t base = t * aq::kTile, end = base + aq::kTile < n ? base + aq::kTile : n;
        for (int64_t g0 = base; g0 < end; g0 += group) {
            const int64_t g1 = g0 + group < n ? g0 + group : n;
            aq::Bounds b = aq::empty_bounds();
            for (int64_t i = g0; i < g1; ++i) aq::take(b, x[i]);
            const aq::Quant q = aq::make_quant(b, bits);
            meta[2 * (g0 / group)] = q.mn;
            meta[2 * (g0 / group) + 1] = q.step;
            for (int64_t w0 = g0; w0 < g1; w0 += per) {  // (g0 is a multiple of 64: a word never straddles two groups)
                uint32_t word = 0;
                for (int k = 0; k < per && w0 + k < g1; ++k) {
                    const int64_t i = w0 + k;
                    const cogdl_walk::Draw d = aq::draw4(seed, call, (uint64_t)i >> 2);
                    word |= aq::code_of(q, x[i], aq::word_of(d, (int)(i & 3))) << (bits * k);
                }
                codes[w0 / per] = word;
            }
        }
    }
    return COGDL_HOST_OK;
}

extern "C" int cogdl_host_actq_dequantize(const uint32_t *codes, const float *meta, int64_t n, int bits, int group, float *out) {
    if (aq::sizes_status(n, bits, group)) return COGDL_HOST_EINVAL;
    if (n == 0) return COGDL_HOST_OK;
    if (!codes || !meta || !out) return COGDL_HOST_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        const int64_t g = i / group;
        out[i] = aq::dequant(meta[2 * g], meta[2 * g + 1], aq::extract_code(codes, i, bits));
    }
    return COGDL_HOST_OK;
}

extern "C" int cogdl_host_relu_mask(const float *x, int64_t n, float *y, uint64_t *mask) {
    if (n < 0) return COGDL_HOST_EINVAL;
    if (n == 0) return COGDL_HOST_OK;
    if (!x || !y || !mask) return COGDL_HOST_EINVAL;
    const int64_t words = aq::num_mask_words(n);
#pragma omp parallel for schedule(static)
    for (int64_t w = 0; w < words; ++w) {
        uint64_t bits = 0;
        for (int k = 0; k < 64 && w * 64 + k < n; ++k) {
            const float v = x[w * 64 + k];
            bits |= (uint64_t)(v > 0.0f ? 1 : 0) << k;
            y[w * 64 + k] = aq::relu_of(v);
        }
        mask[w] = bits;
    }
    return COGDL_HOST_OK;
}

extern "C" int cogdl_host_mask_apply(const float *g, const uint64_t *mask, int64_t n, float *out) {
    if (n < 0) return COGDL_HOST_EINVAL;
    if (n == 0) return COGDL_HOST_OK;
    if (!g || !out || !mask) return COGDL_HOST_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) out[i] = ((mask[i >> 6] >> (i & 63)) & 1u) ? g[i] : 0.0f;
    return COGDL_HOST_OK;
}

extern "C" int cogdl_host_drop_apply(const float *x, int64_t n, uint64_t seed, uint64_t call, uint32_t thresh, float scale,
                                     float *y) {
    if (n < 0 || thresh > 65536u) return COGDL_HOST_EINVAL;
    if (n == 0) return COGDL_HOST_OK;
    if (!x || !y) return COGDL_HOST_EINVAL;
    const int64_t quads = (n + 3) / 4;
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < quads; ++q) {
        const cogdl_walk::Draw d = aq::draw4(seed, call, (uint64_t)q);
        for (int k = 0; k < 4 && 4 * q + k < n; ++k) y[4 * q + k] = aq::drop_of(x[4 * q + k], aq::word_of(d, k), thresh, scale);
    }
    return COGDL_HOST_OK;
}
