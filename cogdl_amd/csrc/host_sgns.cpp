// host_sgns.cpp -- the host twin of csrc/sgns.hip: skip-gram training with negative sampling over rows of token ids.  The
// draws, the order of the updates and every rounding are sgns_law.h's, so with workers == 1 (strictly sequential) the two
// tables equal the GPU's serial mode bit for bit.  workers != 1 runs the rows of an epoch under OpenMP without locks
// (Hogwild): fast, not reproducible.  The target step, the trace and the loop over rows are sgns_host.h's, the host side of
// the wave-level step whose memory rules csrc/sgns_step.h states (they concern the GPU alone).  No HIP.
#include <cstdint>
#include <vector>

#include "../../include/cogdl_host.h"
#include "sgns_host.h"

namespace {
namespace sg = cogdl_sgns;

struct Job {
    const int64_t *walks;
    int64_t W, L, V;
    int D, window, K;
    int64_t epochs;
    double alpha, min_alpha;
    const uint32_t *keep, *cum;
    const float *exp_table;
    uint64_t seed;
    float *syn0, *syn1;
    int B;  // butterfly width
};

struct Scratch {
    std::vector<int32_t> s;  // the kept tokens of the row
    std::vector<float> neu;
};

void train_row(const Job &J, int64_t e, int64_t w, Scratch &scratch, sg::Trace &trace) {
    int32_t *s = scratch.s.data();
    float *__restrict__ neu = scratch.neu.data();
    const float lr = sg::learning_rate(J.alpha, J.min_alpha, e, w, J.W, J.epochs);
    int n = 0;
    for (int p = 0; p < (int)J.L; ++p) {
        const int64_t id = J.walks[w * J.L + p];
        if (id < 0 || id >= J.V) continue;
        if (sg::keep_token(J.seed, w, e, p, J.keep[id])) s[n++] = (int32_t)id;
    }
    const int D = J.D;
    for (int i = 0; i < n; ++i) {
        const int span = J.window - sg::window_shrink(J.seed, w, e, i, J.window);
        const int j0 = i - span < 0 ? 0 : i - span, j1 = i + span > n - 1 ? n - 1 : i + span;
        const int64_t centre = s[i];
        for (int j = j0; j <= j1; ++j) {
            if (j == i) continue;
            const int64_t in = s[j];
            float *__restrict__ x = J.syn0 + in * D;  // (syn0 and syn1 are different tables)
            for (int d = 0; d < D; ++d) neu[d] = 0.0f;
            for (int k = 0; k <= J.K; ++k) {
                int64_t t = centre;
                if (k > 0) {
                    t = sg::draw_negative(J.seed, w, e, i, j, k, J.cum, J.V);
                    if (t == centre) continue;
                }
                const float label = k == 0 ? 1.0f : 0.0f;
                if (sg::apply_target<sg::Skip>(x, J.syn1 + t * D, neu, D, J.B, label, lr, J.exp_table))
                    trace.add(e, w, in, t, label, lr);
            }
            for (int d = 0; d < D; ++d) x[d] = x[d] + neu[d];
        }
    }
}

}  // namespace

extern "C" {

int cogdl_host_sgns_init(float *syn0, float *syn1, int64_t V, int D, uint64_t seed) {
    if (V < 0 || D < 1 || D > sg::kMaxDim || (V > 0 && (!syn0 || !syn1))) return COGDL_HOST_EINVAL;
#pragma omp parallel for schedule(static) if (V * D >= 65536)
    for (int64_t v = 0; v < V; ++v)
        for (int d = 0; d < D; ++d) {
            syn0[v * D + d] = sg::init_value(seed, v, d, D);
            syn1[v * D + d] = 0.0f;
        }
    return COGDL_HOST_OK;
}

int cogdl_host_sgns_train(const int64_t *walks, int64_t W, int64_t L, int64_t V, int D, int window, int negative,
                          int64_t epochs, double alpha, double min_alpha, const uint32_t *keep, const uint32_t *cum,
                          const float *exp_table, uint64_t seed, int workers, float *syn0, float *syn1, int *flags,
                          double *trace, int64_t trace_cap, int64_t *trace_n) {
    const int rc = sg::args_status(W, L, V, D, window, negative, epochs, alpha, min_alpha);
    if (rc) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    if (!keep || !cum || !exp_table || !syn0 || !syn1 || !flags || (W > 0 && !walks) || workers < 0) return COGDL_HOST_EINVAL;
    if (trace && (trace_cap < 0 || !trace_n || workers != 1)) return COGDL_HOST_EINVAL;
    if (trace_n) *trace_n = 0;
    int bad = sg::noise_table_flags(cum, V, 0, 1, sg::kBadTable);
#pragma omp parallel for schedule(static) reduction(| : bad) if (W * L >= 65536)
    for (int64_t k = 0; k < W * L; ++k) bad |= walks[k] >= V ? sg::kBadId : 0;
    *flags = bad;
    if (bad || W == 0) return COGDL_HOST_OK;  // (nothing was touched)
    const Job J = {walks, W, L, V, D, window, negative, epochs, alpha, min_alpha, keep, cum, exp_table, seed, syn0, syn1,
                   sg::butterfly_width(D)};
    sg::Trace tr = {trace, trace_cap, 0};
    for (int64_t e = 0; e < epochs; ++e)
        sg::parallel_for(
            workers, W, 16, [&] { return Scratch{std::vector<int32_t>((size_t)L), std::vector<float>((size_t)D)}; },
            [&](int64_t w, Scratch &scratch) { train_row(J, e, w, scratch, tr); });
    if (trace_n) *trace_n = tr.n;
    return COGDL_HOST_OK;
}

}  // extern "C"
