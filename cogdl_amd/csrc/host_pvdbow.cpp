// host_pvdbow.cpp -- the host twin of csrc/pvdbow.hip: PV-DBOW training over ragged documents.  The draws, the order of the
// updates and every rounding are pvdbow_law.h's (on top of sgns_law.h), so with workers == 1 (strictly sequential) the two
// tables equal the GPU's serial mode bit for bit.  workers != 1 runs the documents of an epoch under OpenMP without locks
// (Hogwild on syn1; a dv row has one writer): fast, not reproducible.  The target step and the loop over documents are
// sgns_host.h's, the host side of the wave-level step whose memory rules csrc/sgns_step.h states.  No HIP.
#include <cstdint>
#include <vector>

#include "../../include/cogdl_host.h"
#include "pvdbow_law.h"
#include "sgns_host.h"

namespace {
namespace sg = cogdl_sgns;
namespace pv = cogdl_pvdbow;

struct Job {
    const int64_t *doc_ptr, *words;
    int64_t G, T, V;
    int D, K;
    int64_t epochs;
    double alpha, min_alpha;
    const uint32_t *keep, *cum;
    const float *exp_table;
    uint64_t seed;
    float *dv, *syn1;
    int B;  // butterfly width
};

void train_doc(const Job &J, int64_t e, int64_t g, std::vector<float> &scratch) {
    float *__restrict__ neu = scratch.data();
    const float lr = sg::learning_rate(J.alpha, J.min_alpha, e, g, J.G, J.epochs);
    const int64_t beg = J.doc_ptr[g], end = J.doc_ptr[g + 1];
    const int D = J.D;
    float *__restrict__ x = J.dv + g * D;  // (dv and syn1 are different tables)
    for (int64_t q = beg; q < end; ++q) {
        const int64_t word = J.words[q];
        if (word < 0 || word >= J.V) continue;
        const uint32_t pos = (uint32_t)(q - beg);
        if (!pv::keep_position(J.seed, g, e, pos, J.keep[word])) continue;
        for (int d = 0; d < D; ++d) neu[d] = 0.0f;
        for (int k = 0; k <= J.K; ++k) {
            int64_t t = word;
            if (k > 0) {
                t = pv::draw_negative(J.seed, g, e, pos, k, J.cum, J.V);
                if (t == word) continue;
            }
            sg::apply_target<sg::Skip>(x, J.syn1 + t * D, neu, D, J.B, k == 0 ? 1.0f : 0.0f, lr, J.exp_table);
        }
        for (int d = 0; d < D; ++d) x[d] = x[d] + neu[d];
    }
}

}  // namespace

extern "C" {

int cogdl_host_pvdbow_init(float *dv, int64_t G, float *syn1, int64_t V, int D, uint64_t seed) {
    if (G < 0 || V < 0 || D < 1 || D > sg::kMaxDim || (G > 0 && !dv) || (V > 0 && !syn1)) return COGDL_HOST_EINVAL;
#pragma omp parallel for schedule(static) if (G * D >= 65536)
    for (int64_t g = 0; g < G; ++g)
        for (int d = 0; d < D; ++d) dv[g * D + d] = pv::init_value(seed, g, d, D);
    for (int64_t k = 0; k < V * D; ++k) syn1[k] = 0.0f;
    return COGDL_HOST_OK;
}

int cogdl_host_pvdbow_train(const int64_t *doc_ptr, int64_t G, const int64_t *words, int64_t T, int64_t V, int D, int negative,
                            int64_t epochs, double alpha, double min_alpha, const uint32_t *keep, const uint32_t *cum,
                            const float *exp_table, uint64_t seed, int workers, float *dv, float *syn1, int *flags) {
    const int rc = pv::args_status(G, T, V, D, negative, epochs, alpha, min_alpha);
    if (rc) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    if (!doc_ptr || !keep || !cum || !exp_table || !syn1 || !flags || (G > 0 && !dv) || (T > 0 && !words) || workers < 0)
        return COGDL_HOST_EINVAL;
    int bad = sg::noise_table_flags(cum, V, 0, 1, pv::kBadTable);
#pragma omp parallel for schedule(static) reduction(| : bad) if (T >= 65536)
    for (int64_t k = 0; k < T; ++k) bad |= words[k] >= V ? pv::kBadId : 0;
    for (int64_t g = 0; g <= G; ++g) {
        const int64_t a = doc_ptr[g];
        if (a < 0 || a > T) bad |= pv::kBadPtr;
        if (g < G && doc_ptr[g + 1] < a) bad |= pv::kBadPtr;
    }
    *flags = bad;
    if (bad || G == 0) return COGDL_HOST_OK;  // (nothing was touched)
    const Job J = {doc_ptr, words, G, T, V, D, negative, epochs, alpha, min_alpha, keep, cum, exp_table, seed, dv, syn1,
                   sg::butterfly_width(D)};
    for (int64_t e = 0; e < epochs; ++e)
        sg::parallel_for(
            workers, G, 16, [&] { return std::vector<float>((size_t)D); },
            [&](int64_t g, std::vector<float> &neu) { train_doc(J, e, g, neu); });
    return COGDL_HOST_OK;
}

}  // extern "C"
