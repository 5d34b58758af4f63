// host_ppr.cpp -- the host twin of csrc/ppr.hip: top-k personalised PageRank by synchronous forward-push rounds in fixed
// point.  The arithmetic, the push rule and the output order are ppr_fixed.h's, the same functions the kernel runs, so for
// equal inputs both return the same arrays.  OpenMP over the sources; each thread owns one open-addressed table that it
// cleans through its touched list after every source.  No HIP.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/cogdl_host.h"
#include "ppr_fixed.h"

namespace {
namespace pp = cogdl_ppr;

struct Table {
    std::vector<int64_t> keys;
    std::vector<uint64_t> r, p, shares;
    std::vector<uint32_t> touched, cur, next;
    uint64_t mask = 0;

    explicit Table(const pp::Params &P) : keys(P.cap, -1), r(P.cap, 0), p(P.cap, 0), mask((uint64_t)P.cap - 1) {
        touched.reserve(P.max_touched);
    }

    // slot of v, inserted if new; -1 when the table's load limit is reached
    int64_t slot_of(int64_t v, const pp::Params &P) {
        uint64_t h = pp::hash_id(v) & mask;
        for (int64_t probe = 0; probe < P.cap; ++probe, h = (h + 1) & mask) {
            if (keys[h] == v) return (int64_t)h;
            if (keys[h] == -1) {
                if ((int64_t)touched.size() >= P.max_touched) return -1;
                keys[h] = v;
                touched.push_back((uint32_t)h);
                return (int64_t)h;
            }
        }
        return -1;
    }

    void clean() {
        for (uint32_t h : touched) {
            keys[h] = -1;
            r[h] = 0;
            p[h] = 0;
        }
        touched.clear();
        cur.clear();
        next.clear();
    }
};

// One source: fills row `i` of the outputs, returns the error bits.
int one_source(const pp::Graph &g, const pp::Params &P, Table &t, int64_t s, int64_t topk, int64_t *nbr, float *val,
               int32_t *count, int32_t *stats) {
    int err = 0;
    int64_t rounds = 0;
    std::vector<std::pair<uint64_t, int64_t>> best;
    if (!pp::valid_id(g, s)) {
        err = pp::kBadSource;
    } else {
        const int64_t s0 = t.slot_of(s, P);
        t.r[s0] = P.r0;
        t.cur.push_back((uint32_t)s0);
        for (; !t.cur.empty() && !err; ++rounds) {
            if (rounds >= P.max_rounds) {
                err |= pp::kRoundCap;
                break;
            }
            const size_t nf = t.cur.size();
            t.shares.resize(nf);
            for (size_t i = 0; i < nf; ++i) {  // phase A: residual -> score, residual cleared, the share of the round
                const uint32_t h = t.cur[i];
                int64_t lo, hi;
                if (!pp::row_of(g, t.keys[h], lo, hi)) err |= pp::kBadRowPtr;
                const uint64_t res = t.r[h];
                t.r[h] = 0;
                t.p[h] += res;
                t.shares[i] = pp::share(res, P.beta, hi - lo);
            }
            if (err) break;
            t.next.clear();
            for (size_t i = 0; i < nf && !err; ++i) {  // phase B: the shares go out
                const uint64_t sh = t.shares[i];
                if (sh == 0) continue;
                int64_t lo, hi;
                pp::row_of(g, t.keys[t.cur[i]], lo, hi);
                for (int64_t j = lo; j < hi; ++j) {
                    const int64_t v = g.indices[j];
                    if (!pp::valid_id(g, v)) {
                        err |= pp::kBadNeighbour;
                        continue;
                    }
                    int64_t vlo, vhi;
                    if (!pp::row_of(g, v, vlo, vhi)) {
                        err |= pp::kBadRowPtr;
                        continue;
                    }
                    const int64_t h = t.slot_of(v, P);
                    if (h < 0) {
                        err |= pp::kTableFull;
                        break;
                    }
                    const uint64_t old = t.r[h];
                    t.r[h] = old + sh;
                    if (pp::crossed(old, old + sh, P.thr, vhi - vlo)) t.next.push_back((uint32_t)h);
                }
            }
            t.cur.swap(t.next);
        }
    }
    int64_t n = 0;
    if (!err) {
        best.reserve(t.touched.size());
        for (uint32_t h : t.touched)
            if (t.p[h] > 0) best.emplace_back(t.p[h], t.keys[h]);
        n = std::min<int64_t>(topk, (int64_t)best.size());
        std::partial_sort(best.begin(), best.begin() + n, best.end(),
                          [](const std::pair<uint64_t, int64_t> &a, const std::pair<uint64_t, int64_t> &b) {
                              return pp::before(a.first, a.second, b.first, b.second);
                          });
    }
    for (int64_t j = 0; j < topk; ++j) {
        nbr[j] = j < n ? best[j].second : -1;
        val[j] = j < n ? pp::to_f32(best[j].first) : 0.0f;
    }
    *count = (int32_t)n;
    if (stats) {
        stats[0] = (int32_t)rounds;
        stats[1] = (int32_t)t.touched.size();
    }
    t.clean();
    return err;
}

}  // namespace

extern "C" {

int cogdl_host_ppr_plan(int64_t num_nodes, int64_t num_edges, int64_t max_source_degree, double alpha, double eps,
                        int64_t *out) {
    if (!out) return COGDL_HOST_EINVAL;
    pp::Params P;
    const int rc = pp::make_params(alpha, eps, num_nodes, num_edges, max_source_degree, &P);
    if (rc != 0) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    out[0] = P.budget;
    out[1] = P.cap;
    out[2] = P.max_rounds;
    out[3] = P.cap <= pp::kLdsCap ? 1 : 0;
    return COGDL_HOST_OK;
}

int cogdl_host_ppr_topk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                        const int64_t *sources, int64_t n_sources, int64_t max_source_degree, double alpha, double eps,
                        int64_t topk, int64_t *nbr, float *val, int32_t *count, int32_t *stats, int *flags) {
    if (num_nodes < 0 || num_edges < 0 || n_sources < 0 || topk < 1 || !flags) return COGDL_HOST_EINVAL;
    if (n_sources > 0 && (!indptr || !sources || !nbr || !val || !count)) return COGDL_HOST_EINVAL;
    if (num_edges > 0 && !indices) return COGDL_HOST_EINVAL;
    pp::Params P;
    const int rc = pp::make_params(alpha, eps, num_nodes, num_edges, max_source_degree, &P);
    if (rc != 0) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    const pp::Graph g = {indptr, indices, num_nodes, num_edges};
    int all = 0;
#pragma omp parallel reduction(| : all) if (n_sources >= 8)
    {
        Table t(P);
#pragma omp for schedule(dynamic, 4)
        for (int64_t i = 0; i < n_sources; ++i)
            all |= one_source(g, P, t, sources[i], topk, nbr + i * topk, val + i * topk, count + i, stats ? stats + 2 * i : nullptr);
    }
    *flags = all;
    return COGDL_HOST_OK;
}

}  // extern "C"
