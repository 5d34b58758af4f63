// sgns.hip -- skip-gram training with negative sampling (SGNS) over rows of token ids for gfx950: the trainer behind
// gensim's Word2Vec(sg=1, negative=K) as the reference's deepwalk / node2vec call it, on walks that are already on the
// device.  The law (draws, order of updates, every rounding) is sgns_law.h, which the host twin (host_sgns.cpp) includes
// too.
//
// Shape.  One wave64 per row of `walks`.  The kept tokens of the row sit in LDS (wave-private), lane l owns the elements
// d = l, l + 64, .. of every embedding row it touches (256 contiguous bytes per wave instruction), the dot product is a
// per-lane sum plus a shuffle butterfly, and the sigmoid is a table in LDS.  Lanes 1..K draw and binary-search the K
// negatives of a pair in parallel.
//
// Two modes, one kernel.
//   workers == 1   one launch of ONE wave that runs every epoch and every row in order: the tables equal the host twin's,
//                  bit for bit.  Slow by construction (one wave of 1024 CUs' worth).
//   workers != 1   per epoch, launches of at most rows_in_flight rows, in row order.  Rows of one launch run concurrently
//                  and update the tables without locks (Hogwild); within a row the law holds.
//
// Coherence.  Rows of syn0 and syn1 are read and updated by the wave-level step of sgns_step.h, under the rules stated at
// its head ("Coherence"); this kernel adds the wait for the wave's own updates at the end of every pair (the input row of a
// pair is the input row of the next centres' pairs), takes the row-update variant from tuning key 17 (kTuneSgnsVariant), and
// sends rows in launches of rows_in_flight, not in one persistent grid, because the kernel boundary is what bounds how
// stale another XCD's copy of a row can be.
// Error flags are raised by a validation pass that runs first in the stream (ids >= V, a cum that runs backwards); the
// training kernels read the word and leave the tables untouched when it is non-zero.  Ids are bounds-checked again where
// they are used: nothing is read out of bounds.
#include "common.h"

#include "sgns_law.h"
#include "sgns_step.h"

namespace cogdl {

namespace sg = cogdl_sgns;

constexpr int kSgnsBlock = 256;                    // 4 waves = 4 rows per workgroup
constexpr int kSgnsWaves = kSgnsBlock / kWave;
constexpr int kSgnsRowsInFlight = 8192;            // rows per launch of the throughput mode (profiles/sgns_bench.txt)

struct SgnsJob {
    const int64_t *walks;
    int64_t W, L, V;
    int D, window, K;
    int64_t epochs;
    double alpha, min_alpha;
    const uint32_t *keep, *cum;
    const float *exp_table;
    uint64_t seed;
    float *syn0, *syn1;
    const int *flags;
};

__device__ __forceinline__ void sgns_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rows row0 + (global wave index) + k * (waves of the grid) below row0 + n_rows, for the epochs [e0, e1).
template <int KD, bool STORES>
__global__ __launch_bounds__(kSgnsBlock) void sgns_train_kernel(SgnsJob J, int64_t row0, int64_t n_rows, int64_t e0, int64_t e1) {
    __shared__ float exp_lds[sg::kExpTable];
    __shared__ int32_t tok_lds[kSgnsWaves][sg::kMaxLength];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (!stage_exp_table(exp_lds, J.exp_table, J.flags)) return;  // a bad id or table: touch nothing
    int32_t *s = tok_lds[wave];
    const int D = J.D, B = sg::butterfly_width(D);
    const int L = (int)J.L;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t e = e0; e < e1; ++e) {
        for (int64_t w = row0 + (int64_t)blockIdx.x * (blockDim.x >> 6) + wave; w < row0 + n_rows; w += n_waves) {
            const float lr = sg::learning_rate(J.alpha, J.min_alpha, e, w, J.W, J.epochs);
            // the kept tokens, compacted in order
            int n = 0;
            sgns_lds_sync();  // (the previous row's readers of s are done)
            for (int p0 = 0; p0 < L; p0 += kWave) {
                const int p = p0 + lane;
                int64_t id = -1;
                if (p < L) id = J.walks[w * J.L + p];
                bool kept = false;
                if (id >= 0 && id < J.V) kept = sg::keep_token(J.seed, w, e, p, J.keep[id]);
                const uint64_t mask = __ballot(kept);
                if (kept) s[n + __popcll(mask & (((uint64_t)1 << lane) - 1))] = (int32_t)id;
                n += __popcll(mask);
            }
            sgns_lds_sync();
            for (int i = 0; i < n; ++i) {
                const int span = J.window - sg::window_shrink(J.seed, w, e, i, J.window);
                const int j0 = i - span < 0 ? 0 : i - span, j1 = i + span > n - 1 ? n - 1 : i + span;
                const int32_t centre = s[i];
                for (int j = j0; j <= j1; ++j) {
                    if (j == i) continue;
                    const int32_t in = s[j];
                    // lane k holds target k: the centre, then the K negatives (-1: skipped)
                    int32_t tl = -1;
                    if (lane == 0) tl = centre;
                    else if (lane <= J.K) {
                        tl = (int32_t)sg::draw_negative(J.seed, w, e, i, j, lane, J.cum, J.V);
                        if (tl == centre) tl = -1;
                    }
                    float *xrow = J.syn0 + (int64_t)in * D + lane;
                    float x[KD], neu[KD] = {};
                    load_row<KD>(x, xrow, lane, D);
                    update_lane_targets<KD, sg::Skip, STORES>(tl, J.K, x, neu, J.syn1, lr, exp_lds, lane, D, B);
#pragma unroll
                    for (int q = 0; q < KD; ++q)
                        if (lane + q * kWave < D) row_add<STORES>(xrow + q * kWave, x[q], neu[q]);
                    wait_own_updates();
                }
            }
        }
    }
}

__global__ void sgns_check_kernel(const int64_t *__restrict__ walks, int64_t n_tokens, const uint32_t *__restrict__ cum, int64_t V,
                                  int *__restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int err = sg::noise_table_flags(cum, V, first, stride, sg::kBadTable);
    for (int64_t k = first; k < n_tokens; k += stride) err |= walks[k] >= V ? sg::kBadId : 0;
    raise_flags(flags, err);
}

__global__ void sgns_init_kernel(float *__restrict__ syn0, float *__restrict__ syn1, int64_t V, int D, uint64_t seed) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, total = V * D;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += stride) {
        syn0[k] = sg::init_value(seed, k / D, (int)(k % D), D);
        syn1[k] = 0.0f;
    }
}

static void sgns_launch(unsigned blocks, unsigned threads, hipStream_t s, const SgnsJob &J, int64_t row0, int64_t n_rows, int64_t e0,
                        int64_t e1) {
    with_row_width(J.D, g_tuning[kTuneSgnsVariant] == 1, [&](auto kd, auto stores) {
        hipLaunchKernelGGL((sgns_train_kernel<decltype(kd)::value, decltype(stores)::value>), dim3(blocks), dim3(threads), 0, s, J, row0,
                           n_rows, e0, e1);
    });
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_sgns_init(float *syn0, float *syn1, int64_t V, int D, uint64_t seed, void *stream) {
    if (V < 0 || D < 1 || D > sg::kMaxDim || (V > 0 && (!syn0 || !syn1))) return COGDL_HIP_EINVAL;
    if (V == 0) return COGDL_HIP_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((V * D + 255) / 256, 8192);
    hipLaunchKernelGGL(sgns_init_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, syn0, syn1, V, D, seed);
    return launch_status();
}

extern "C" int cogdl_hip_sgns_train(const int64_t *walks, int64_t W, int64_t L, int64_t V, int D, int window, int negative,
                                    int64_t epochs, double alpha, double min_alpha, const uint32_t *keep, const uint32_t *cum,
                                    const float *exp_table, uint64_t seed, int workers, int64_t rows_in_flight, float *syn0,
                                    float *syn1, int *flags, void *stream) {
    const int rc = sg::args_status(W, L, V, D, window, negative, epochs, alpha, min_alpha);
    if (rc) return rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (!keep || !cum || !exp_table || !syn0 || !syn1 || !flags || (W > 0 && !walks) || workers < 0 || rows_in_flight < 0)
        return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cleared = clear_flags_async(flags, s);
    if (cleared != COGDL_HIP_OK) return cleared;
    const int64_t n_check = std::max<int64_t>(W * L, V);
    hipLaunchKernelGGL(sgns_check_kernel, dim3((unsigned)std::min<int64_t>((n_check + 255) / 256, 8192)), dim3(256), 0, s, walks,
                       W * L, cum, V, flags);
    int st = launch_status();
    if (st != COGDL_HIP_OK || W == 0) return st;
    const SgnsJob J = {walks, W, L, V, D, window, negative, epochs, alpha, min_alpha, keep, cum, exp_table, seed, syn0, syn1, flags};
    if (workers == 1) {  // one wave, every epoch and row in order
        sgns_launch(1u, (unsigned)kWave, s, J, 0, W, 0, epochs);
        return launch_status();
    }
    const int64_t chunk = rows_in_flight > 0 ? rows_in_flight : kSgnsRowsInFlight;
    for (int64_t ep = 0; ep < epochs && st == COGDL_HIP_OK; ++ep)
        st = launch_chunks(W, chunk, [&](int64_t row0, int64_t n_rows) {
            sgns_launch((unsigned)((n_rows + kSgnsWaves - 1) / kSgnsWaves), (unsigned)kSgnsBlock, s, J, row0, n_rows, ep, ep + 1);
        });
    return st;
}
