// host_kgsample.cpp -- the host twin of csrc/kgsample.hip: one training batch of a knowledge-graph embedding model (positives,
// filtered negatives, subsampling weights).  Rows, draws and the lookup are kgsample_law.h's, the same the kernel follows, so
// for equal inputs positive, negative, weight and the status word are the GPU's bit for bit.  OpenMP over the rows of the
// batch; the result does not depend on the number of threads.  No HIP.
#include <cstdint>

#include "../../include/cogdl_host.h"
#include "kgsample_law.h"

namespace kgs = cogdl_kgsample;

template <typename IndexT>
static int kgs_batch(const int32_t *triples, const float *weight_tab, const int32_t *group, const int32_t *list_ptr,
                     const int32_t *list_idx, int64_t T, int64_t G, int64_t list_len, const int32_t *order, int64_t B, int64_t K,
                     int64_t N, uint64_t seed, uint32_t tag, uint64_t first_sid, int64_t *positive, IndexT *negative,
                     float *weight) {
    int flags = 0;
#pragma omp parallel for schedule(static) reduction(| : flags)
    for (int64_t b = 0; b < B; ++b) {
        const kgs::Row row = kgs::resolve_row(order, b, group, list_ptr, T, G, list_len, N);
        IndexT *neg = negative + b * K;
        if (row.err) {
            flags |= row.err;
            for (int c = 0; c < 3; ++c) positive[b * 3 + c] = -1;
            weight[b] = 0.0f;
            for (int64_t j = 0; j < K; ++j) neg[j] = (IndexT)-1;
            continue;
        }
        for (int c = 0; c < 3; ++c) positive[b * 3 + c] = (int64_t)triples[(int64_t)row.t * 3 + c];
        weight[b] = weight_tab[row.t];
        const int32_t *a = list_idx + row.lo;
        const uint64_t sid = first_sid + (uint64_t)b;
        for (int64_t j = 0; j < K; ++j)
            neg[j] = (IndexT)kgs::negative_of(kgs::draw_word(seed, tag, sid, j), row.M, row.L, [a](int32_t i) { return a[i] - i; });
    }
    return flags;
}

extern "C" int cogdl_host_kg_train_batch(const int32_t *triples, const float *weight_tab, const int32_t *group,
                                         const int32_t *list_ptr, const int32_t *list_idx, int64_t T, int64_t G, int64_t list_len,
                                         const int32_t *order, int64_t B, int64_t K, int64_t N, uint64_t seed, uint32_t tag,
                                         uint64_t first_sid, int index64, int64_t *positive, void *negative, float *weight,
                                         int *status) {
    const int rc = kgs::sizes_status(T, G, list_len, B, K, N);
    if (rc != 0) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    if (!status) return COGDL_HOST_EINVAL;
    *status = 0;
    if (B == 0) return COGDL_HOST_OK;
    if (!order || !positive || !weight || !list_ptr || (K > 0 && !negative)) return COGDL_HOST_EINVAL;
    if (T > 0 && (!triples || !weight_tab || !group)) return COGDL_HOST_EINVAL;
    if (list_len > 0 && !list_idx) return COGDL_HOST_EINVAL;
    *status = index64 ? kgs_batch(triples, weight_tab, group, list_ptr, list_idx, T, G, list_len, order, B, K, N, seed, tag,
                                  first_sid, positive, (int64_t *)negative, weight)
                      : kgs_batch(triples, weight_tab, group, list_ptr, list_idx, T, G, list_len, order, B, K, N, seed, tag,
                                  first_sid, positive, (int32_t *)negative, weight);
    return COGDL_HOST_OK;
}
