// line.hip -- edge-sampled skip-gram training with negative sampling for gfx950: the trainer of the LINE model (orders 1 and
// 2) on an edge table that is already on the device.  The law (draws, order of updates, every rounding) is line_law.h, which
// the host twin (host_line.cpp) includes too.
//
// Shape.  One wave64 runs a contiguous range of samples.  The draws are counter-based, so any lane can compute any draw: per
// group of 64 samples, lane l draws the edge (one binary search over ecum), the orientation, the learning rate and the K
// negatives (K binary searches over ncum, advanced in lockstep so that their loads are in flight together) of sample
// base + l, and works out which negatives are skipped (equal to u or v) and which repeat an earlier one.  The group's
// samples then run one after the other: the values travel from lane i to the whole wave by readlane, lane l owns the elements
// d = l, l + 64, .. of every row, emb[u] and err stay in registers for the sample, the dot product is a per-lane sum plus a
// shuffle butterfly, and the sigmoid is a table in LDS.  Up to D = 64 the loads of all the sample's distinct target rows are
// issued together, before the first dot product (the law reads emb[u] once per sample, so distinct targets do not depend on
// each other; wider rows would take the K + 1 row buffers out of the register file); a repeated target is read again after
// the wave's own update of it has completed.
//
// Two modes, one kernel.
//   workers == 1   one launch of ONE wave that runs samples 0 .. S - 1 in order and waits for its own updates after every
//                  sample: the tables equal the host twin's, bit for bit.  Slow by construction.
//   workers != 1   launches of at most samples_in_flight consecutive samples, in sample order.  The samples of one launch run
//                  concurrently and update the tables without locks (Hogwild); within a sample the law holds.
//
// Coherence.  Table rows are read and updated through sgns_step.h, under the rules stated at its head ("Coherence"), with the
// memory-side atomic add as the only row update.  This kernel keeps its own loop over the targets (unrolled, with prefetch
// slots and the skip / repeat masks) and so its own wait before the re-read of a repeated target; samples go in launches of
// samples_in_flight and not in one persistent grid because the kernel boundary bounds how stale another XCD's copy can be.
// Error flags are raised by a validation pass that runs first in the stream; the training kernels read the word and leave
// the tables untouched when it is non-zero.  Ids are bounds-checked again where they are used: nothing is read out of bounds.
#include "common.h"

#include "line_law.h"
#include "sgns_step.h"

namespace cogdl {

namespace ln = cogdl_line;

constexpr int kLineBlock = 256;  // 4 waves per workgroup
constexpr int kLineWaves = kLineBlock / kWave;
constexpr int kLineMaxWaves = 4096;               // waves of one launch of the throughput mode: 16 per CU
constexpr int64_t kLineSamplesInFlight = 262144;  // samples per launch of the throughput mode (profiles/line_bench.txt)
constexpr int kLineTargets = ln::kMaxNegative + 1;

struct LineJob {
    const int64_t *eu, *ev, *ecum;
    int64_t M, V;
    const uint32_t *ncum;
    const float *exp_table;
    int D, K;
    int64_t S;
    double alpha;
    uint64_t seed;
    float *emb, *tgt;  // tgt: emb (order 1) or ctx (order 2)
    const int *flags;
};

// Wave w of the grid runs the samples [s0 + w * per, s0 + (w + 1) * per) below s0 + n.  ORDERED: wait for the sample's
// updates before the next sample begins (the serial mode).  PREFETCH: hold all K + 1 target rows in registers.  Four waves
// per SIMD (at most 128 registers: the compiler takes 170 when left alone, which admits two): a wave's samples are a chain
// of load and atomic latencies, and the rate grows with the waves a CU can switch between (profiles/line_bench.txt).
template <int KD, bool PREFETCH, bool ORDERED>
__global__ __launch_bounds__(kLineBlock, 4) void line_train_kernel(LineJob J, int64_t s0, int64_t n, int64_t per) {
    __shared__ float exp_lds[cogdl_sgns::kExpTable];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (!stage_exp_table(exp_lds, J.exp_table, J.flags)) return;  // a bad id or table: touch nothing
    const int D = J.D, K = J.K, B = cogdl_sgns::butterfly_width(D);
    const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    const int64_t first = s0 + w * per, stop = s0 + n;
    const int64_t last = first + per < stop ? first + per : stop;
    for (int64_t base = first; base < last; base += kWave) {
        const int cnt = last - base < kWave ? (int)(last - base) : kWave;
        // ---- the draws of sample base + lane
        int32_t u_l = -1, v_l = -1, neg[ln::kMaxNegative];
        float lr_l = 0.0f;
        uint32_t skip_l = 0, dup_l = 0;  // bit k: target k is skipped / repeats an earlier target of the sample
#pragma unroll
        for (int d = 0; d < ln::kMaxNegative; ++d) neg[d] = 0;
        if (lane < cnt) {
            const int64_t s = base + lane;
            bool swapped;
            const int64_t e = ln::draw_edge(J.seed, s, J.ecum, J.M, swapped);
            const int64_t a = J.eu[e], b = J.ev[e];
            if ((uint64_t)a < (uint64_t)J.V && (uint64_t)b < (uint64_t)J.V) {
                u_l = (int32_t)(swapped ? b : a);
                v_l = (int32_t)(swapped ? a : b);
            }
            lr_l = ln::learning_rate(J.alpha, s, J.S);
            // ln::draw_negative for d = 1..K, the K searches advanced in lockstep
            uint32_t key[ln::kMaxNegative];
            int32_t hi[ln::kMaxNegative];
#pragma unroll
            for (int d = 0; d < ln::kMaxNegative; ++d) {
                key[d] = 0;
                hi[d] = 0;
                if (d < K) {
                    key[d] = ln::negative_key(J.seed, s, d + 1, J.ncum, J.V);
                    hi[d] = (int32_t)(J.V - 1);
                }
            }
            bool more = true;
            while (more) {
                more = false;
#pragma unroll
                for (int d = 0; d < ln::kMaxNegative; ++d)
                    if (neg[d] < hi[d]) {
                        const int32_t mid = neg[d] + ((hi[d] - neg[d]) >> 1);
                        if (J.ncum[mid] > key[d]) hi[d] = mid;
                        else neg[d] = mid + 1;
                        more |= neg[d] < hi[d];
                    }
            }
#pragma unroll
            for (int d = 0; d < ln::kMaxNegative; ++d)
                if (d < K) {
                    if (neg[d] == u_l || neg[d] == v_l) skip_l |= 2u << d;
                    else {
                        bool dup = false;
#pragma unroll
                        for (int q = 0; q < d; ++q) dup |= neg[q] == neg[d];  // (a skipped q differs from this one)
                        if (dup) dup_l |= 2u << d;
                    }
                }
        }
        // ---- the samples of the group, in order
        for (int i = 0; i < cnt; ++i) {
            const int32_t u = __builtin_amdgcn_readlane(u_l, i), v = __builtin_amdgcn_readlane(v_l, i);
            if (u < 0) continue;  // (an endpoint outside [0, V): the validation pass has flagged it)
            const float lr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lr_l), i));
            const uint32_t skip = (uint32_t)__builtin_amdgcn_readlane((int)skip_l, i);
            const uint32_t dup = (uint32_t)__builtin_amdgcn_readlane((int)dup_l, i);
            float *xrow = J.emb + (int64_t)u * D + lane;
            float x[KD], err[KD] = {};
            load_row<KD>(x, xrow, lane, D);
            float y[PREFETCH ? kLineTargets : 1][KD];
            if constexpr (PREFETCH) {
#pragma unroll
                for (int k = 0; k < kLineTargets; ++k)
                    if (k <= K && !(((skip | dup) >> k) & 1u)) {
                        const int32_t t = k == 0 ? v : __builtin_amdgcn_readlane(neg[k == 0 ? 0 : k - 1], i);
                        load_row<KD>(y[k], J.tgt + (int64_t)t * D + lane, lane, D);
                    }
            }
#pragma unroll
            for (int k = 0; k < kLineTargets; ++k) {
                if (k > K || ((skip >> k) & 1u)) continue;  // (no early exit: the loop is unrolled, k is a constant below)
                const int slot = PREFETCH ? k : 0;
                const int32_t t = k == 0 ? v : __builtin_amdgcn_readlane(neg[k == 0 ? 0 : k - 1], i);
                float *yrow = J.tgt + (int64_t)t * D + lane;
                const bool again = (dup >> k) & 1u;
                if (!PREFETCH || again) {
                    if (again) wait_own_updates();  // a target this sample has already updated
                    load_row<KD>(y[slot], yrow, lane, D);
                }
                const float f = wave_dot<KD>(x, y[slot], lane, D, B);
                update_target<KD, ln::Saturate, false>(f, x, y[slot], yrow, err, k == 0 ? 1.0f : 0.0f, lr, exp_lds, lane, D);
            }
#pragma unroll
            for (int q = 0; q < KD; ++q)
                if (lane + q * kWave < D) row_add<false>(xrow + q * kWave, x[q], err[q]);
            if constexpr (ORDERED) wait_own_updates();
        }
    }
}

__global__ void line_check_kernel(const int64_t *__restrict__ eu, const int64_t *__restrict__ ev, const int64_t *__restrict__ ecum,
                                  int64_t M, const uint32_t *__restrict__ ncum, int64_t V, int *__restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int err = cogdl_sgns::noise_table_flags(ncum, V, first, stride, ln::kBadNodeTable);
    for (int64_t k = first; k < M; k += stride) {
        if ((uint64_t)eu[k] >= (uint64_t)V || (uint64_t)ev[k] >= (uint64_t)V) err |= ln::kBadEndpoint;
        if (ecum) {
            if (k > 0 && ecum[k] < ecum[k - 1]) err |= ln::kBadEdgeTable;
            if (k == 0 && ecum[k] < 0) err |= ln::kBadEdgeTable;
            if (k == M - 1 && (ecum[k] < 1 || ecum[k] > ln::kEdgeTotalMax)) err |= ln::kBadEdgeTable;
        }
    }
    raise_flags(flags, err);
}

// PREFETCH up to D = 64 (one element per lane)
static void line_launch(bool ordered, unsigned blocks, unsigned threads, hipStream_t s, const LineJob &J, int64_t s0, int64_t n,
                        int64_t per) {
    with_row_width(J.D, ordered, [&](auto kd, auto ord) {
        constexpr int KD = decltype(kd)::value;
        hipLaunchKernelGGL((line_train_kernel<KD, KD == 1, decltype(ord)::value>), dim3(blocks), dim3(threads), 0, s, J, s0, n, per);
    });
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_line_train(const int64_t *eu, const int64_t *ev, const int64_t *ecum, int64_t M, int64_t V,
                                    const uint32_t *ncum, const float *exp_table, int D, int negative, int order, int64_t S,
                                    double alpha, uint64_t seed, int workers, int64_t samples_in_flight, float *emb, float *ctx,
                                    int *flags, void *stream) {
    const int rc = ln::args_status(M, V, D, negative, order, S, alpha);
    if (rc) return rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (!eu || !ev || !ncum || !exp_table || !emb || (order == 2 && !ctx) || !flags || workers < 0 || samples_in_flight < 0)
        return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cleared = clear_flags_async(flags, s);
    if (cleared != COGDL_HIP_OK) return cleared;
    const int64_t n_check = std::max<int64_t>(M, V);
    hipLaunchKernelGGL(line_check_kernel, dim3((unsigned)std::min<int64_t>((n_check + 255) / 256, 8192)), dim3(256), 0, s, eu, ev,
                       ecum, M, ncum, V, flags);
    int st = launch_status();
    if (st != COGDL_HIP_OK || S == 0) return st;
    const LineJob J = {eu, ev, ecum, M, V, ncum, exp_table, D, negative, S, alpha, seed, emb, order == 1 ? emb : ctx, flags};
    if (workers == 1) {  // one wave, every sample in order
        line_launch(true, 1u, (unsigned)kWave, s, J, 0, S, S);
        return launch_status();
    }
    return launch_chunks(S, samples_in_flight > 0 ? samples_in_flight : kLineSamplesInFlight, [&](int64_t s0, int64_t n) {
        const int64_t per = (n + kLineMaxWaves - 1) / kLineMaxWaves, waves = (n + per - 1) / per;
        line_launch(false, (unsigned)((waves + kLineWaves - 1) / kLineWaves), (unsigned)kLineBlock, s, J, s0, n, per);
    });
}
