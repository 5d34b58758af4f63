// host_kgrank.cpp -- the host twin of csrc/kgrank.hip: all-entity ranking counts for knowledge-graph link prediction.  The
// score of a pair of rows, the buckets and the treatment of filter lists are kgrank_law.h's, the same the kernels follow, so
// for equal inputs all three counts of every query are the GPU's.  OpenMP over the queries; the result does not depend on the
// number of threads.  No HIP.
#include <cmath>
#include <cstdint>

#include "../../include/cogdl_host.h"
#include "kgrank_law.h"

namespace kg = cogdl_kgrank;

extern "C" int cogdl_host_kg_rank(const float *q, const float *table, const int32_t *target, int64_t M, int64_t N, int64_t D,
                                  int kind, float gamma, const int32_t *filt_ptr, const int32_t *filt_idx, int64_t filt_len,
                                  int32_t *counts) {
    const int rc = kg::sizes_status(M, N, D, kind, filt_len);
    if (rc != 0) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    if (M == 0) return COGDL_HOST_OK;
    if (!target || !counts || (D > 0 && (!q || (N > 0 && !table)))) return COGDL_HOST_EINVAL;
    if (filt_len > 0 && (!filt_ptr || !filt_idx)) return COGDL_HOST_EINVAL;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t i = 0; i < M; ++i) {
        int32_t c[3] = {0, 0, 0};
        const int64_t t = target[i];
        if (t >= 0 && t < N) {
            const float *qi = q + i * D;
            const float st = kg::score(kind, gamma, qi, table + t * D, D);
            for (int64_t e = 0; e < N; ++e) {
                const int b = kg::bucket(kg::score(kind, gamma, qi, table + e * D, D), st, e, t);
                if (b >= 0) ++c[b];
            }
            if (filt_len > 0) {
                int64_t lo = filt_ptr[i], hi = filt_ptr[i + 1];
                lo = lo < 0 ? 0 : lo;
                hi = hi > filt_len ? filt_len : hi;
                for (int64_t j = lo; j < hi; ++j) {
                    const int64_t e = filt_idx[j];
                    if (e < 0 || e >= N || e == t) continue;
                    if (j > lo && filt_idx[j - 1] == e) continue;  // a duplicate of its predecessor
                    const int b = kg::bucket(kg::score(kind, gamma, qi, table + e * D, D), st, e, t);
                    if (b >= 0) --c[b];
                }
            }
        }
        counts[3 * i] = c[0];
        counts[3 * i + 1] = c[1];
        counts[3 * i + 2] = c[2];
    }
    return COGDL_HOST_OK;
}
