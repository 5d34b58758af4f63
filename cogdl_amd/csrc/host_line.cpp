// host_line.cpp -- the host twin of csrc/line.hip: edge-sampled skip-gram training (LINE, orders 1 and 2).  The draws, the
// order of the updates and every rounding are line_law.h's (on top of sgns_law.h), so with workers == 1 (strictly
// sequential) the tables equal the GPU's serial mode bit for bit.  workers != 1 runs the samples under OpenMP without locks
// (Hogwild): fast, not reproducible.  No HIP.
#include <cstdint>
#include <vector>

#include "../../include/cogdl_host.h"
#include "line_law.h"

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

struct Trace {
    double *rec;
    int64_t cap, n;
};

// the dot product in sgns_law.h's order: lane sums over d % 64, then the butterfly's lower half
inline float dot(const float *a, const float *b, int D, int B) {
    float p[sg::kLanes];
    const int m = D < sg::kLanes ? D : sg::kLanes;
    for (int l = 0; l < m; ++l) p[l] = 0.0f + a[l] * b[l];
    for (int l = m; l < B; ++l) p[l] = 0.0f;
    for (int d = sg::kLanes; d < D; ++d) p[d & (sg::kLanes - 1)] = p[d & (sg::kLanes - 1)] + a[d] * b[d];
    for (int s = B >> 1; s > 0; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
    return p[0];
}

// x and err are scratch rows of D floats (x is the sample's copy of emb[u]: in order 1 a target row can be emb[u] itself)
void train_sample(const Job &J, int64_t s, float *x, float *err, Trace *trace) {
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
        float *y = J.tgt + t * D;
        const float f = dot(x, y, D, J.B);
        if (!ln::applies(f)) continue;
        const float label = k == 0 ? 1.0f : 0.0f;
        const float g = ln::gradient(f, label, lr, J.exp_table);
        for (int d = 0; d < D; ++d) {
            err[d] = err[d] + g * y[d];
            y[d] = y[d] + g * x[d];
        }
        if (trace) {
            if (trace->n < trace->cap) {
                double *r = trace->rec + trace->n * 5;
                r[0] = (double)s, r[1] = (double)u, r[2] = (double)t, r[3] = (double)label, r[4] = (double)lr;
            }
            ++trace->n;
        }
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
    int bad = 0;
    for (int64_t v = 1; v < V; ++v) bad |= ncum[v] < ncum[v - 1] ? ln::kBadNodeTable : 0;
    bad |= ncum[V - 1] == 0 ? ln::kBadNodeTable : 0;
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
    if (workers == 1) {
        Trace tr = {trace, trace_cap, 0};
        std::vector<float> x((size_t)D), err((size_t)D);
        for (int64_t s = 0; s < S; ++s) train_sample(J, s, x.data(), err.data(), trace ? &tr : nullptr);
        if (trace_n) *trace_n = tr.n;
        return COGDL_HOST_OK;
    }
    if (workers > 1) {
#pragma omp parallel num_threads(workers)
        {
            std::vector<float> x((size_t)D), err((size_t)D);
#pragma omp for schedule(dynamic, 256)
            for (int64_t s = 0; s < S; ++s) train_sample(J, s, x.data(), err.data(), nullptr);
        }
    } else {
#pragma omp parallel
        {
            std::vector<float> x((size_t)D), err((size_t)D);
#pragma omp for schedule(dynamic, 256)
            for (int64_t s = 0; s < S; ++s) train_sample(J, s, x.data(), err.data(), nullptr);
        }
    }
    return COGDL_HOST_OK;
}
