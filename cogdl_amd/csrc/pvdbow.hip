// pvdbow.hip -- PV-DBOW training over ragged documents for gfx950: the trainer behind gensim's Doc2Vec(dm=0, negative=K) as
// the reference's Graph2Vec calls it (cogdl/models/emb/graph2vec.py:99-109), on documents that are already on the device.
// The law (draws, order of updates, every rounding) is pvdbow_law.h on top of sgns_law.h; the host twin (host_pvdbow.cpp)
// includes both.
//
// Shape.  One wave64 per document.  dv[g] belongs to its wave alone: lane l keeps the elements d = l, l + 64, .. (at most 8)
// in VGPRs for the whole document and stores them once at its end.  Only syn1 rows are shared between waves; they are read
// and updated by the wave-level step of sgns_step.h, under the rules stated at its head ("Coherence"), with the update
// variant of kTuneSgnsVariant, and the wave waits for its own updates at the end of every position.
// Token ids are read 64 at a time, `keep` is decided per lane and the kept positions are walked off a ballot in ascending
// order; lanes 1..K draw and binary-search the K negatives of a position in parallel.
//
// Two modes, one kernel, as in sgns.hip.
//   workers == 1   one launch of ONE wave that runs every epoch and every document in order: the tables equal the host
//                  twin's, bit for bit.
//   workers != 1   per epoch, launches of at most docs_in_flight documents, in document order.  The kernel boundary bounds
//                  how stale a syn1 row can be; dv rows are exact either way (one writer).
// One wave per document makes a batch with one very long document uneven; that is not addressed here.
// Error flags are raised by a validation pass that runs first in the stream; the training kernels read the word and leave
// the tables untouched when it is non-zero.  Ids are bounds-checked again where they are used.
#include "common.h"

#include "pvdbow_law.h"
#include "sgns_step.h"

namespace cogdl {

namespace sg = cogdl_sgns;
namespace pv = cogdl_pvdbow;

constexpr int kPvBlock = 256;  // 4 waves = 4 documents per workgroup
constexpr int kPvWaves = kPvBlock / kWave;
constexpr int kPvDocsInFlight = 8192;

struct PvJob {
    const int64_t *doc_ptr, *words;
    int64_t G, T, V;
    int D, K;
    int64_t epochs;
    double alpha, min_alpha;
    const uint32_t *keep, *cum;
    const float *exp_table;
    uint64_t seed;
    float *dv, *syn1;
    const int *flags;
};

// Documents doc0 + (global wave index) + k * (waves of the grid) below doc0 + n_docs, for the epochs [e0, e1).
template <int KD, bool STORES>
__global__ __launch_bounds__(kPvBlock) void pvdbow_train_kernel(PvJob J, int64_t doc0, int64_t n_docs, int64_t e0, int64_t e1) {
    __shared__ float exp_lds[sg::kExpTable];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (!stage_exp_table(exp_lds, J.exp_table, J.flags)) return;  // a bad id, table or doc_ptr: touch nothing
    const int D = J.D, B = sg::butterfly_width(D);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t e = e0; e < e1; ++e) {
        for (int64_t g = doc0 + (int64_t)blockIdx.x * (blockDim.x >> 6) + wave; g < doc0 + n_docs; g += n_waves) {
            const float lr = sg::learning_rate(J.alpha, J.min_alpha, e, g, J.G, J.epochs);
            const int64_t beg = J.doc_ptr[g], end = J.doc_ptr[g + 1];  // (validated: 0 <= beg <= end <= T)
            if (beg >= end) continue;
            float *xrow = J.dv + g * D + lane;
            float x[KD];
            load_row<KD>(x, xrow, lane, D);
            for (int64_t p0 = beg; p0 < end; p0 += kWave) {
                const int64_t q = p0 + lane;
                int64_t id = -1;
                if (q < end) id = J.words[q];
                bool kept = false;
                if (id >= 0 && id < J.V) kept = pv::keep_position(J.seed, g, e, (uint32_t)(q - beg), J.keep[id]);
                uint64_t mask = __ballot(kept);
                const int32_t id32 = kept ? (int32_t)id : -1;
                while (mask) {
                    const int b = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const int32_t word = __builtin_amdgcn_readlane(id32, b);
                    const uint32_t pos = (uint32_t)(p0 - beg) + (uint32_t)b;
                    // lane k holds target k: the word, then the K negatives (-1: skipped)
                    int32_t tl = -1;
                    if (lane == 0) tl = word;
                    else if (lane <= J.K) {
                        tl = (int32_t)pv::draw_negative(J.seed, g, e, pos, lane, J.cum, J.V);
                        if (tl == word) tl = -1;
                    }
                    float neu[KD] = {};
                    update_lane_targets<KD, sg::Skip, STORES>(tl, J.K, x, neu, J.syn1, lr, exp_lds, lane, D, B);
#pragma unroll
                    for (int c = 0; c < KD; ++c) x[c] = x[c] + neu[c];
                    wait_own_updates();
                }
            }
#pragma unroll
            for (int k = 0; k < KD; ++k)
                if (lane + k * kWave < D) __hip_atomic_store(xrow + k * kWave, x[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            wait_own_updates();
        }
    }
}

__global__ void pvdbow_check_kernel(const int64_t *__restrict__ doc_ptr, int64_t G, const int64_t *__restrict__ words, int64_t T,
                                    const uint32_t *__restrict__ cum, int64_t V, int *__restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int err = sg::noise_table_flags(cum, V, first, stride, pv::kBadTable);
    for (int64_t k = first; k < T; k += stride) err |= words[k] >= V ? pv::kBadId : 0;
    for (int64_t g = first; g <= G; g += stride) {
        const int64_t a = doc_ptr[g];
        if (a < 0 || a > T) err |= pv::kBadPtr;
        if (g < G && doc_ptr[g + 1] < a) err |= pv::kBadPtr;
    }
    raise_flags(flags, err);
}

__global__ void pvdbow_init_kernel(float *__restrict__ dv, int64_t G, float *__restrict__ syn1, int64_t V, int D, uint64_t seed) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t k = first; k < G * D; k += stride) dv[k] = pv::init_value(seed, k / D, (int)(k % D), D);
    for (int64_t k = first; k < V * D; k += stride) syn1[k] = 0.0f;
}

static void pvdbow_launch(unsigned blocks, unsigned threads, hipStream_t s, const PvJob &J, int64_t doc0, int64_t n_docs, int64_t e0,
                          int64_t e1) {
    with_row_width(J.D, g_tuning[kTuneSgnsVariant] == 1, [&](auto kd, auto stores) {
        hipLaunchKernelGGL((pvdbow_train_kernel<decltype(kd)::value, decltype(stores)::value>), dim3(blocks), dim3(threads), 0, s, J,
                           doc0, n_docs, e0, e1);
    });
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_pvdbow_init(float *dv, int64_t G, float *syn1, int64_t V, int D, uint64_t seed, void *stream) {
    if (G < 0 || V < 0 || D < 1 || D > sg::kMaxDim || (G > 0 && !dv) || (V > 0 && !syn1)) return COGDL_HIP_EINVAL;
    const int64_t n = std::max<int64_t>(G, V) * D;
    if (n == 0) return COGDL_HIP_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(pvdbow_init_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dv, G, syn1, V, D, seed);
    return launch_status();
}

extern "C" int cogdl_hip_pvdbow_train(const int64_t *doc_ptr, int64_t G, const int64_t *words, int64_t T, int64_t V, int D,
                                      int negative, int64_t epochs, double alpha, double min_alpha, const uint32_t *keep,
                                      const uint32_t *cum, const float *exp_table, uint64_t seed, int workers,
                                      int64_t docs_in_flight, float *dv, float *syn1, int *flags, void *stream) {
    const int rc = pv::args_status(G, T, V, D, negative, epochs, alpha, min_alpha);
    if (rc) return rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (!doc_ptr || !keep || !cum || !exp_table || !syn1 || !flags || (G > 0 && !dv) || (T > 0 && !words) || workers < 0 ||
        docs_in_flight < 0)
        return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cleared = clear_flags_async(flags, s);
    if (cleared != COGDL_HIP_OK) return cleared;
    const int64_t n_check = std::max<int64_t>(std::max<int64_t>(T, V), G + 1);
    hipLaunchKernelGGL(pvdbow_check_kernel, dim3((unsigned)std::min<int64_t>((n_check + 255) / 256, 8192)), dim3(256), 0, s, doc_ptr, G,
                       words, T, cum, V, flags);
    int st = launch_status();
    if (st != COGDL_HIP_OK || G == 0) return st;
    const PvJob J = {doc_ptr, words, G, T, V, D, negative, epochs, alpha, min_alpha, keep, cum, exp_table, seed, dv, syn1, flags};
    if (workers == 1) {  // one wave, every epoch and document in order
        pvdbow_launch(1u, (unsigned)kWave, s, J, 0, G, 0, epochs);
        return launch_status();
    }
    const int64_t chunk = docs_in_flight > 0 ? docs_in_flight : kPvDocsInFlight;
    for (int64_t ep = 0; ep < epochs && st == COGDL_HIP_OK; ++ep)
        st = launch_chunks(G, chunk, [&](int64_t doc0, int64_t n_docs) {
            pvdbow_launch((unsigned)((n_docs + kPvWaves - 1) / kPvWaves), (unsigned)kPvBlock, s, J, doc0, n_docs, ep, ep + 1);
        });
    return st;
}
