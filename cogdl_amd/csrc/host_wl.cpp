// host_wl.cpp -- the host twin of csrc/wl.hip: Weisfeiler-Lehman subtree relabelling on a batch of graphs, by the law of
// wl_law.h.  Signatures are compared outright (the table below is keyed by a hash but every hit is verified against the
// stored representative, and a miss probes on), so the result does not depend on the hash; nodes are numbered in one serial
// pass in id order, the rows are gathered and sorted under OpenMP (order-free).  hash_bits < 128 emulates the GPU's
// truncated hash: where two different signatures of a round share a truncated hash the GPU's verification raises
// kCollision, and so does this twin.  No HIP.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/cogdl_host.h"
#include "wl_law.h"

namespace {
namespace wl = cogdl_wl;

struct Trunc {
    uint64_t lo, hi;
    int32_t label;
    bool operator<(const Trunc &o) const { return hi != o.hi ? hi < o.hi : lo != o.lo ? lo < o.lo : label < o.label; }
};

}  // namespace

extern "C" {

int cogdl_host_wl_max_degree(void) { return wl::kMaxDegree; }

int cogdl_host_wl_labels(const int32_t *indptr, const int32_t *indices, const int64_t *label0, int64_t N, int64_t E,
                         int64_t rounds, int hash_bits, uint64_t salt, int32_t *labels, int64_t *classes, int *flags) {
    const int rc = wl::args_status(N, E, rounds, hash_bits);
    if (rc) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    if (!indptr || !flags || !classes || (E > 0 && !indices) || (N > 0 && (!label0 || !labels))) return COGDL_HOST_EINVAL;
    for (int64_t r = 0; r <= rounds; ++r) classes[r] = 0;
    int bad = 0;
    if (indptr[0] != 0 || indptr[N] != E) bad |= wl::kBadPtr;
    for (int64_t v = 0; v < N; ++v) {
        const int64_t deg = (int64_t)indptr[v + 1] - indptr[v];
        if (deg < 0 || indptr[v] < 0 || indptr[v] > E) bad |= wl::kBadPtr;
        else if (deg > wl::kMaxDegree) bad |= wl::kRowTooLong;
    }
    if (!(bad & wl::kBadPtr))
        for (int64_t k = 0; k < E; ++k) bad |= (indices[k] < 0 || indices[k] >= N) ? wl::kBadIndex : 0;
    *flags = bad;
    if (bad || N == 0) return COGDL_HOST_OK;

    const int64_t slots = wl::table_slots(N);
    std::vector<int32_t> sorted((size_t)E), table((size_t)slots);
    std::vector<wl::Hash> hash((size_t)N);
    std::vector<Trunc> trunc;
    for (int64_t r = 0; r <= rounds; ++r) {
        const int32_t *prev = r > 0 ? labels + (r - 1) * N : nullptr;
        int32_t *next = labels + r * N;
#pragma omp parallel for schedule(dynamic, 256) if (N + E >= 65536)
        for (int64_t v = 0; v < N; ++v) {
            if (r == 0) {
                hash[v] = wl::finish(salt, label0[v], 0, 0, 0, 128);
                continue;
            }
            const int32_t a = indptr[v], b = indptr[v + 1];
            for (int32_t k = a; k < b; ++k) sorted[k] = prev[indices[k]];
            std::sort(sorted.begin() + a, sorted.begin() + b);
            uint64_t s0 = 0, s1 = 0;
            for (int32_t k = a; k < b; ++k) {
                s0 += wl::element(salt, 0, k - a, sorted[k]);
                s1 += wl::element(salt, 1, k - a, sorted[k]);
            }
            hash[v] = wl::finish(salt, prev[v], b - a, s0, s1, 128);
        }
        std::fill(table.begin(), table.end(), -1);
        int32_t n_classes = 0;
        for (int64_t v = 0; v < N; ++v) {  // serial, in id order: a class is numbered where its first node is met
            uint64_t slot = hash[v].lo & (uint64_t)(slots - 1);
            for (;;) {  // (at most N of the >= 2 N slots are ever taken: an empty one is always reached)
                const int32_t u = table[slot];
                if (u < 0) {
                    table[slot] = (int32_t)v;
                    next[v] = n_classes++;
                    break;
                }
                bool same;
                if (r == 0) same = label0[u] == label0[v];
                else {
                    const int32_t au = indptr[u], av = indptr[v], du = indptr[u + 1] - au, dv = indptr[v + 1] - av;
                    same = prev[u] == prev[v] && du == dv && std::equal(sorted.begin() + av, sorted.begin() + av + dv, sorted.begin() + au);
                }
                if (same) {
                    next[v] = next[u];
                    break;
                }
                slot = (slot + 1) & (uint64_t)(slots - 1);
            }
        }
        classes[r] = n_classes;
        if (hash_bits < 128) {  // would the GPU's truncated hash have merged two classes?
            trunc.resize((size_t)N);
            for (int64_t v = 0; v < N; ++v) {
                const wl::Hash t = wl::truncate(hash[v], hash_bits);
                trunc[v] = {t.lo, t.hi, next[v]};
            }
            std::sort(trunc.begin(), trunc.end());
            for (int64_t v = 1; v < N; ++v)
                if (trunc[v].lo == trunc[v - 1].lo && trunc[v].hi == trunc[v - 1].hi && trunc[v].label != trunc[v - 1].label) {
                    *flags = wl::kCollision;
                    return COGDL_HOST_OK;
                }
        }
    }
    return COGDL_HOST_OK;
}

}  // extern "C"
