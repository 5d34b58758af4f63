// kgsample.hip -- one training batch of a knowledge-graph embedding model, made on the device: for each of B positives named
// by `order`, the triple, its subsampling weight and K negatives drawn uniformly from the entities that are not true for it
// (the reference does this on the host, one positive at a time: np.random.randint + np.in1d in a rejection loop, three tensors
// per positive, a collate of 1024 of them and a copy to the device; cogdl/datasets/kg_data.py:98-135).  The law is
// kgsample_law.h's: every negative is a pure function of (seed, tag, sid, j) and the positive's true list -- no rejection
// loop, no data-dependent trip count beyond the binary search's ceil(log2(L + 1)).
//
//   kg_train_batch_kernel  one wave per positive, four waves per workgroup.  The wave resolves its row once (triple id, group,
//                          list bounds: wave-uniform), stages a list of at most kLdsList ids in its own LDS slice as a[i] - i,
//                          and its lanes stride over pairs of negatives: one Philox call gives the words of j = 2 p and
//                          2 p + 1, each is scaled to [0, M) and looked up by one upper-bound search -- in LDS, or, for a
//                          longer list, in global memory (the lists of a dataset are a few MB: L2 hits).
// Integer work and a few KB of traffic per row: the launch is latency-bound, the geometry only has to keep the searches of a
// wave in flight together.  No atomics; every store is an ordinary store of a value the lane computed.  The status word is
// raised by a plain read-or-write (common.h: raise_flags).  A refused row (kgsample_law.h: Refusals) is written as -1 and
// indexes nothing.
#include "common.h"
#include "kgsample_law.h"

namespace cogdl {
namespace kgs = cogdl_kgsample;

constexpr int kKgsThreads = 256;
constexpr int kKgsWaves = kKgsThreads / kWave;

template <typename IndexT>
__global__ __launch_bounds__(kKgsThreads) void kg_train_batch_kernel(
    const int32_t *__restrict__ triples, const float *__restrict__ weight_tab, const int32_t *__restrict__ group,
    const int32_t *__restrict__ list_ptr, const int32_t *__restrict__ list_idx, int64_t T, int64_t G, int64_t list_len,
    const int32_t *__restrict__ order, int64_t B, int64_t K, int64_t N, uint64_t seed, uint32_t tag, uint64_t first_sid,
    int64_t *__restrict__ positive, IndexT *__restrict__ negative, float *__restrict__ weight, int *__restrict__ status) {
    __shared__ int32_t kgs_gap[kKgsWaves][kgs::kLdsList];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * kKgsWaves + wave;  // wave-uniform
    const bool live = b < B;
    kgs::Row row = {0, 0, 0, 0, 0};
    if (live) row = kgs::resolve_row(order, b, group, list_ptr, T, G, list_len, N);
    const bool draw = live && row.err == 0;
    const bool staged = draw && row.L <= kgs::kLdsList;
    const int32_t *a = list_idx + row.lo;  // [0, L): inside list_idx (resolve_row)
    if (staged) {
        for (int32_t i = lane; i < row.L; i += kWave) kgs_gap[wave][i] = a[i] - i;
    }
    __syncthreads();  // (every wave of the workgroup arrives here: nothing above returns)
    if (!live) return;
    IndexT *neg = negative + b * K;
    if (!draw) {
        if (lane < 3) positive[b * 3 + lane] = -1;
        if (lane == 0) weight[b] = 0.0f;
        for (int64_t j = lane; j < K; j += kWave) neg[j] = (IndexT)-1;
        if (lane == 0) raise_flags(status, row.err);
        return;
    }
    if (lane < 3) positive[b * 3 + lane] = (int64_t)triples[(int64_t)row.t * 3 + lane];
    if (lane == 0) weight[b] = weight_tab[row.t];
    const uint64_t sid = first_sid + (uint64_t)b;
    const int64_t pairs = (K + 1) >> 1;
    const int32_t *gaps = kgs_gap[wave];
    for (int64_t p = lane; p < pairs; p += kWave) {
        uint64_t w0, w1;
        kgs::draw_pair(seed, tag, sid, p, &w0, &w1);
        int64_t n0, n1;
        if (staged) {
            n0 = kgs::negative_of(w0, row.M, row.L, [gaps](int32_t i) { return gaps[i]; });
            n1 = kgs::negative_of(w1, row.M, row.L, [gaps](int32_t i) { return gaps[i]; });
        } else {
            n0 = kgs::negative_of(w0, row.M, row.L, [a](int32_t i) { return a[i] - i; });
            n1 = kgs::negative_of(w1, row.M, row.L, [a](int32_t i) { return a[i] - i; });
        }
        neg[2 * p] = (IndexT)n0;
        if (2 * p + 1 < K) neg[2 * p + 1] = (IndexT)n1;
    }
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_kg_train_batch(const int32_t *triples, const float *weight_tab, const int32_t *group,
                                        const int32_t *list_ptr, const int32_t *list_idx, int64_t T, int64_t G, int64_t list_len,
                                        const int32_t *order, int64_t B, int64_t K, int64_t N, uint64_t seed, uint32_t tag,
                                        uint64_t first_sid, int index64, int64_t *positive, void *negative, float *weight,
                                        int *status, void *stream) {
    const int rc = kgs::sizes_status(T, G, list_len, B, K, N);
    if (rc != 0) return rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (!status) return COGDL_HIP_EINVAL;
    if (!aligned_to(status, 4)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int cleared = clear_flags_async(status, s);
    if (cleared != COGDL_HIP_OK || B == 0) return cleared;
    if (!order || !positive || !weight || !list_ptr || (K > 0 && !negative)) return COGDL_HIP_EINVAL;
    if (T > 0 && (!triples || !weight_tab || !group)) return COGDL_HIP_EINVAL;
    if (list_len > 0 && !list_idx) return COGDL_HIP_EINVAL;
    if (!aligned_to(triples, 4) || !aligned_to(weight_tab, 4) || !aligned_to(group, 4) || !aligned_to(list_ptr, 4) ||
        !aligned_to(list_idx, 4) || !aligned_to(order, 4) || !aligned_to(positive, 8) || !aligned_to(negative, index64 ? 8 : 4) ||
        !aligned_to(weight, 4))
        return COGDL_HIP_EALIGN;
    const dim3 grid((unsigned)((B + kKgsWaves - 1) / kKgsWaves)), block(kKgsThreads);
    if (index64)
        hipLaunchKernelGGL(kg_train_batch_kernel<int64_t>, grid, block, 0, s, triples, weight_tab, group, list_ptr, list_idx, T, G,
                           list_len, order, B, K, N, seed, tag, first_sid, positive, (int64_t *)negative, weight, status);
    else
        hipLaunchKernelGGL(kg_train_batch_kernel<int32_t>, grid, block, 0, s, triples, weight_tab, group, list_ptr, list_idx, T, G,
                           list_len, order, B, K, N, seed, tag, first_sid, positive, (int32_t *)negative, weight, status);
    return launch_status();
}
