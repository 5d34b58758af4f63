// host_line.cpp -- the host twin of csrc/line.hip: edge-sampled skip-gram training (LINE, orders 1 and 2).  The draws, the
// order of the updates and every rounding are line_law.h's (on top of sgns_law.h), so with workers == 1 (strictly
// sequential) the tables equal the GPU's serial mode bit for bit.  workers != 1 runs the samples under OpenMP without locks
// (Hogwild): fast, not reproducible.  The target step, the trace and the loop over samples are sgns_host.h's, the host side
// of the wave-level step whose memory rules csrc/sgns_step.h states.  No HIP.
#include <cstdint>
#include <vector>

#include "../../include/cogdl_host.h"
#include "line_law.h"
#include "sgns_host.h"

namespace {
namespace sg = cogdl_sgns;
namespace ln = cogdl_line;

struct Job {
    const int64_t *eu, *ev, *ecum;
    int64_t M, V;
    const uint32_t *ncum;
    const float *exp_table;
    int D, K;
    int64_t S;
    double alpha;
    uint64_t seed;
    float *emb, *tgt;  // tgt: emb (order 1) or ctx (order 2)
    int B;             // butterfly width
};

// x and err are scratch rows of D floats (x is the sample's copy of emb[u]: in order 1 a target row can be emb[u] itself)
struct Scratch {
    std::vector<float> x, err;
};

void train_sample(const Job &J, int64_t s, Scratch &scratch, sg::Trace &trace) {
    float *x = scratch.x.data(), *err = scratch.err.data();
    bool swapped;
    const int64_t e = ln::draw_edge(J.seed, s, J.ecum, J.M, swapped);
    int64_t u = J.eu[e], v = J.ev[e];
    if ((uint64_t)u >= (uint64_t)J.V || (uint64_t)v >= (uint64_t)J.V) return;  // (the validation pass has flagged it)
    if (swapped) {
        const int64_t k = u;
        u = v, v = k;
    }
    const float lr = ln::learning_rate(J.alpha, s, J.S);
    const int D = J.D;
    float *xrow = J.emb + u * D;
    for (int d = 0; d < D; ++d) x[d] = xrow[d], err[d] = 0.0f;
    for (int k = 0; k <= J.K; ++k) {
        int64_t t = v;
        if (k > 0) {
            t = ln::draw_negative(J.seed, s, k, J.ncum, J.V);
            if (t == u || t == v) continue;
        }
        const float label = k == 0 ? 1.0f : 0.0f;
        if (sg::apply_target<ln::Saturate>(x, J.tgt + t * D, err, D, J.B, label, lr, J.exp_table))
            trace.add(s, u, t, label, lr);
    }
    for (int d = 0; d < D; ++d) xrow[d] = xrow[d] + err[d];
}

}  // namespace

extern "C" int cogdl_host_line_train(const int64_t *eu, const int64_t *ev, const int64_t *ecum, int64_t M, int64_t V,
                                     const uint32_t *ncum, const float *exp_table, int D, int negative, int order, int64_t S,
                                     double alpha, uint64_t seed, int workers, float *emb, float *ctx, int *flags, double *trace,
                                     int64_t trace_cap, int64_t *trace_n) {
    const int rc = ln::args_status(M, V, D, negative, order, S, alpha);
    if (rc) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    if (!eu || !ev || !ncum || !exp_table || !emb || (order == 2 && !ctx) || !flags || workers < 0) return COGDL_HOST_EINVAL;
    if (trace && (trace_cap < 0 || !trace_n || workers != 1)) return COGDL_HOST_EINVAL;
    if (trace_n) *trace_n = 0;
    int bad = sg::noise_table_flags(ncum, V, 0, 1, ln::kBadNodeTable);
    if (ecum) {
        for (int64_t k = 1; k < M; ++k) bad |= ecum[k] < ecum[k - 1] ? ln::kBadEdgeTable : 0;
        bad |= ecum[0] < 0 || ecum[M - 1] < 1 || ecum[M - 1] > ln::kEdgeTotalMax ? ln::kBadEdgeTable : 0;
    }
#pragma omp parallel for schedule(static) reduction(| : bad) if (M >= 65536)
    for (int64_t k = 0; k < M; ++k)
        bad |= (uint64_t)eu[k] >= (uint64_t)V || (uint64_t)ev[k] >= (uint64_t)V ? ln::kBadEndpoint : 0;
    *flags = bad;
    if (bad || S == 0) return COGDL_HOST_OK;  // (nothing was touched)
    const Job J = {eu, ev, ecum, M, V, ncum, exp_table, D, negative, S, alpha, seed, emb, order == 1 ? emb : ctx, sg::butterfly_width(D)};
    sg::Trace tr = {trace, trace_cap, 0};
    sg::parallel_for(
        workers, S, 256, [&] { return Scratch{std::vector<float>((size_t)D), std::vector<float>((size_t)D)}; },
        [&](int64_t s, Scratch &scratch) { train_sample(J, s, scratch, tr); });
    if (trace_n) *trace_n = tr.n;
    return COGDL_HOST_OK;
}
