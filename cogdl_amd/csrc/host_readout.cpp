// host_readout.cpp -- the host twin of csrc/readout.hip: segment sum / mean / max pooling over a sorted batch vector and
// sort-pool, forward and backward.  The order of the additions, the comparisons and the sort order are readout_law.h's, the
// same the kernels follow, so for equal inputs both return the same bytes.  OpenMP over graphs (or rows); the result does
// not depend on the number of threads.  No HIP.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/cogdl_host.h"
#include "readout_law.h"

namespace {
namespace ro = cogdl_readout;

struct Seg {
    int64_t lo, hi;
};
inline Seg segment_of(const int32_t *ptr, int64_t g, int64_t N) {
    const int64_t lo = ro::clamp_row(ptr[g], 0, N);
    return {lo, ro::clamp_row(ptr[g + 1], lo, N)};
}

inline int sizes_rc(int64_t N, int64_t B, int64_t F, int64_t k) {
    const int rc = ro::sizes_status(N, B, F, k);
    return rc == 0 ? COGDL_HOST_OK : (rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE);
}

// One graph, one mode: `ways` accumulators per column (1 for a segment inside the exact bound), combined in way order.
template <int MODE>
void pool_graph(const float *x, int64_t N, int64_t F, Seg s, float *out, int32_t *argmax, std::vector<float> &v,
                std::vector<int32_t> &a) {
    const int64_t n = s.hi - s.lo;
    const int ways = n > ro::kExactNodes ? ro::kWays : 1;
    std::fill(v.begin(), v.begin() + ways * F, MODE == ro::kMax ? -INFINITY : 0.0f);
    std::fill(a.begin(), a.begin() + ways * F, (int32_t)s.lo);
    for (int64_t j = 0; j < n; ++j) {
        const float *row = x + (s.lo + j) * F;
        float *acc = v.data() + (ways == 1 ? 0 : ro::way_of(j)) * F;
        int32_t *arg = a.data() + (ways == 1 ? 0 : ro::way_of(j)) * F;
        for (int64_t f = 0; f < F; ++f) {
            if (MODE == ro::kMax) {
                if (row[f] > acc[f]) {
                    acc[f] = row[f];
                    arg[f] = (int32_t)(s.lo + j);
                }
            } else {
                acc[f] = acc[f] + row[f];
            }
        }
    }
    for (int64_t f = 0; f < F; ++f) {
        float r = v[f];
        int32_t ra = a[f];
        for (int w = 1; w < ways; ++w) {
            if (MODE == ro::kMax) {
                if (ro::better(v[w * F + f], a[w * F + f], r, ra)) {
                    r = v[w * F + f];
                    ra = a[w * F + f];
                }
            } else {
                r = r + v[w * F + f];
            }
        }
        out[f] = n == 0 ? 0.0f : (MODE == ro::kMean ? r / (float)n : r);
        if (MODE == ro::kMax) argmax[f] = n == 0 ? -1 : ra;
    }
}

}  // namespace

extern "C" {

int cogdl_host_segment_exact_nodes(void) { return ro::kExactNodes; }

int cogdl_host_segment_ptr(const int64_t *batch, int64_t N, int64_t B, int32_t *ptr, int *flag) {
    const int rc = sizes_rc(N, B, 1, 1);
    if (rc) return rc;
    if (N == 0 || B == 0) return COGDL_HOST_OK;
    if (!batch || !ptr || !flag) return COGDL_HOST_EINVAL;
    int bad = 0;
    for (int64_t i = 0; i <= N; ++i) {
        const int64_t prev = i > 0 ? batch[i - 1] : -1, cur = i < N ? batch[i] : B;
        if (i < N && (cur < 0 || cur >= B || cur < prev)) bad = 1;
        const int64_t first = ro::clamp_row(prev, -1, B) + 1, last = ro::clamp_row(cur, -1, B);
        for (int64_t g = first; g <= last; ++g) ptr[g] = (int32_t)i;
    }
    *flag = bad;
    return COGDL_HOST_OK;
}

int cogdl_host_segment_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int mode, float *out,
                                int32_t *argmax) {
    const int rc = sizes_rc(N, B, F, 1);
    if (rc) return rc;
    if (mode < ro::kSum || mode > ro::kMax) return COGDL_HOST_EINVAL;
    if (N == 0 || B == 0) return COGDL_HOST_OK;
    if (!x || !ptr || !out || (mode == ro::kMax && !argmax)) return COGDL_HOST_EINVAL;
#pragma omp parallel
    {
        std::vector<float> v((size_t)(ro::kWays * F));
        std::vector<int32_t> a((size_t)(ro::kWays * F));
#pragma omp for schedule(dynamic, 16)
        for (int64_t g = 0; g < B; ++g) {
            const Seg s = segment_of(ptr, g, N);
            int32_t *am = argmax ? argmax + g * F : nullptr;
            if (mode == ro::kSum) pool_graph<ro::kSum>(x, N, F, s, out + g * F, am, v, a);
            else if (mode == ro::kMean) pool_graph<ro::kMean>(x, N, F, s, out + g * F, am, v, a);
            else pool_graph<ro::kMax>(x, N, F, s, out + g * F, am, v, a);
        }
    }
    return COGDL_HOST_OK;
}

int cogdl_host_segment_pool_bwd(const float *grad, const int32_t *ptr, const int64_t *batch, const int32_t *argmax, int64_t N,
                                int64_t B, int64_t F, int mode, float *grad_x) {
    const int rc = sizes_rc(N, B, F, 1);
    if (rc) return rc;
    if (mode < ro::kSum || mode > ro::kMax) return COGDL_HOST_EINVAL;
    if (N == 0) return COGDL_HOST_OK;
    if (!ptr || !grad_x || (B > 0 && !grad) || (mode == ro::kMax && !argmax)) return COGDL_HOST_EINVAL;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < N; ++i) {
        float *o = grad_x + i * F;
        int64_t g = batch ? batch[i] : (std::upper_bound(ptr, ptr + B + 1, i, [](int64_t v, int32_t p) { return v < (int64_t)p; }) - ptr) - 1;
        Seg s = {0, 0};
        if (g >= 0 && g < B) s = segment_of(ptr, g, N);
        if (s.hi <= s.lo) {
            std::fill(o, o + F, 0.0f);
            continue;
        }
        const float *gr = grad + g * F;
        for (int64_t f = 0; f < F; ++f) {
            if (mode == ro::kSum) o[f] = gr[f];
            else if (mode == ro::kMean) o[f] = gr[f] / (float)(s.hi - s.lo);
            else o[f] = (int64_t)argmax[g * F + f] == i ? gr[f] : 0.0f;
        }
    }
    return COGDL_HOST_OK;
}

int cogdl_host_sort_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int64_t k, int64_t key_col,
                             float *out, int32_t *idx) {
    const int rc = sizes_rc(N, B, F, k);
    if (rc) return rc;
    if (key_col < 0 || key_col >= F) return COGDL_HOST_EINVAL;
    if (B * k > 0x7fffffff) return COGDL_HOST_ERANGE;
    if (B == 0) return COGDL_HOST_OK;
    if (!ptr || !out || !idx || (N > 0 && !x)) return COGDL_HOST_EINVAL;
#pragma omp parallel
    {
        std::vector<uint64_t> w;
#pragma omp for schedule(dynamic, 4)
        for (int64_t g = 0; g < B; ++g) {
            const Seg s = segment_of(ptr, g, N);
            const int64_t n = s.hi - s.lo, kk = std::min(n, k);
            w.resize((size_t)n);
            for (int64_t t = 0; t < n; ++t) w[t] = ro::word(x[(s.lo + t) * F + key_col], t);
            std::partial_sort(w.begin(), w.begin() + kk, w.end());  // (the words are distinct: any sort gives this order)
            for (int64_t j = 0; j < k; ++j) {
                float *o = out + (g * k + j) * F;
                if (j < kk) {
                    const int64_t src = s.lo + (int64_t)(uint32_t)w[j];
                    idx[g * k + j] = (int32_t)src;
                    memcpy(o, x + src * F, sizeof(float) * (size_t)F);
                } else {
                    idx[g * k + j] = -1;
                    std::fill(o, o + F, 0.0f);
                }
            }
        }
    }
    return COGDL_HOST_OK;
}

int cogdl_host_sort_pool_bwd(const float *grad, const int32_t *idx, int64_t N, int64_t B, int64_t F, int64_t k, float *grad_x) {
    const int rc = sizes_rc(N, B, F, k);
    if (rc) return rc;
    if (B * k > 0x7fffffff) return COGDL_HOST_ERANGE;
    if (N == 0) return COGDL_HOST_OK;
    if (!grad_x || (B > 0 && (!grad || !idx))) return COGDL_HOST_EINVAL;
    std::fill(grad_x, grad_x + N * F, 0.0f);
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < B * k; ++j) {
        const int64_t dst = idx[j];
        if (dst >= 0 && dst < N) memcpy(grad_x + dst * F, grad + j * F, sizeof(float) * (size_t)F);
    }
    return COGDL_HOST_OK;
}

}  // extern "C"
