// host_kgscore.cpp -- the host twin of csrc/kgscore.hip: sampled triple scores and their two gradients for knowledge-graph
// embedding training.  Scores, partial derivatives and the order of every sum are kgscore_law.h's, the same the kernels follow,
// so for equal inputs scores, grad_q and grad_table are the GPU's bit for bit.  OpenMP over the query rows (over the entities
// for grad_table); the result does not depend on the number of threads.  No HIP.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/cogdl_host.h"
#include "kgscore_law.h"

namespace ks = cogdl_kgscore;
namespace kgl = cogdl_kgrank;

static int ks_sizes(int64_t B, int64_t K, int64_t N, int64_t D, int kind) {
    const int rc = ks::sizes_status(B, K, N, D, kind);
    return rc == 0 ? COGDL_HOST_OK : (rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE);
}

extern "C" int cogdl_host_kg_score(const float *q, const float *table, const int32_t *idx, int64_t B, int64_t K, int64_t N,
                                   int64_t D, int kind, float gamma, float *scores) {
    const int rc = ks_sizes(B, K, N, D, kind);
    if (rc != COGDL_HOST_OK) return rc;
    if (B == 0 || K == 0) return COGDL_HOST_OK;
    if (!idx || !scores || (D > 0 && (!q || (N > 0 && !table)))) return COGDL_HOST_EINVAL;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t b = 0; b < B; ++b) {
        for (int64_t j = 0; j < K; ++j) {
            const int64_t e = idx[b * K + j];
            scores[b * K + j] = (e < 0 || e >= N) ? std::numeric_limits<float>::quiet_NaN()
                                                  : ks::score(kind, gamma, q + b * D, table + e * D, D);
        }
    }
    return COGDL_HOST_OK;
}

// acc_a[k] (and acc_b[k], cl2's imaginary column) += g * partial for every term k of one pair of rows
template <bool WRT_Q>
static inline void ks_add_row(int kind, const float *qrow, const float *trow, float g, int64_t terms, int64_t half, float *acc) {
    for (int64_t k = 0; k < terms; ++k) {
        const float q_b = kind == kgl::kCl2 ? qrow[k + half] : 0.0f, t_b = kind == kgl::kCl2 ? trow[k + half] : 0.0f;
        float da, db;
        if (WRT_Q) ks::partial_q(kind, qrow[k], q_b, trow[k], t_b, &da, &db);
        else ks::partial_t(kind, qrow[k], q_b, trow[k], t_b, &da, &db);
        acc[k] = ks::add_contribution(acc[k], g, da);
        if (kind == kgl::kCl2) acc[k + half] = ks::add_contribution(acc[k + half], g, db);
    }
}

extern "C" int cogdl_host_kg_score_grad_q(const float *q, const float *table, const int32_t *idx, const float *g, int64_t B,
                                          int64_t K, int64_t N, int64_t D, int kind, float *grad_q) {
    const int rc = ks_sizes(B, K, N, D, kind);
    if (rc != COGDL_HOST_OK) return rc;
    if (B == 0 || D == 0) return COGDL_HOST_OK;
    if (!q || !grad_q || (K > 0 && (!idx || !g || (N > 0 && !table)))) return COGDL_HOST_EINVAL;
    const int64_t terms = ks::terms_of(kind, D), half = D / 2;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t b = 0; b < B; ++b) {
        float *out = grad_q + b * D;
        for (int64_t k = 0; k < D; ++k) out[k] = 0.0f;
        for (int64_t j = 0; j < K; ++j) {
            const int64_t e = idx[b * K + j];
            if (e < 0 || e >= N) continue;
            ks_add_row<true>(kind, q + b * D, table + e * D, g[b * K + j], terms, half, out);
        }
    }
    return COGDL_HOST_OK;
}

extern "C" int cogdl_host_kg_score_grad_table(const float *q, const float *table, const float *g, const int32_t *occ_ptr,
                                              const int32_t *occ_pos, int64_t B, int64_t K, int64_t N, int64_t D, int kind,
                                              float *grad_table) {
    const int rc = ks_sizes(B, K, N, D, kind);
    if (rc != COGDL_HOST_OK) return rc;
    if (N == 0 || D == 0) return COGDL_HOST_OK;
    if (!table || !grad_table || !occ_ptr || (B * K > 0 && (!q || !g || !occ_pos))) return COGDL_HOST_EINVAL;
    const int64_t terms = ks::terms_of(kind, D), half = D / 2, BK = B * K;
#pragma omp parallel
    {
        std::vector<float> part((size_t)D);
#pragma omp for schedule(dynamic, 16)
        for (int64_t e = 0; e < N; ++e) {
            float *out = grad_table + e * D;
            for (int64_t k = 0; k < D; ++k) out[k] = 0.0f;
            int64_t lo = occ_ptr[e], hi = occ_ptr[e + 1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > BK ? BK : hi;
            for (int64_t c0 = lo; c0 < hi; c0 += ks::kChunk) {
                const int64_t c1 = c0 + ks::kChunk < hi ? c0 + ks::kChunk : hi;
                for (int64_t k = 0; k < D; ++k) part[k] = 0.0f;
                for (int64_t i = c0; i < c1; ++i) {
                    const int64_t p = occ_pos[i];
                    if (p < 0 || p >= BK) continue;
                    ks_add_row<false>(kind, q + (p / K) * D, table + e * D, g[p], terms, half, part.data());
                }
                for (int64_t k = 0; k < D; ++k) out[k] = out[k] + part[k];
            }
        }
    }
    return COGDL_HOST_OK;
}
