// kgscore.hip -- sampled triple scoring for knowledge-graph embedding training: the score of query row q[b] against the table
// rows an index matrix idx[B, K] names, and its two gradients, without a [B, K, D] gather (the reference's KGEModel.forward,
// cogdl/models/emb/knowledge_base.py:52-101, index_selects that copy and broadcasts three to eight elementwise kernels over
// it; its backward scatters [B K, D] rows with float atomics).  Scores, partial derivatives and the order of every sum are
// kgscore_law.h's.  Bandwidth-bound row gathering, no MFMA, no atomics: equal results from run to run.
//
//   kg_score_kernel        one workgroup of four waves per query row b.  q[b] goes to LDS once; the waves take the j in turn,
//                          a wave reads table[idx[b, j]] with up to kInFlight 16-byte loads per lane in flight, lane l adds the
//                          terms of slot l in ascending k, the butterfly is five + one xor shuffles, lane 0 writes the score.
//   kg_score_grad_q_kernel grid (B, column blocks of 1024 terms).  A thread owns four terms (for cl2: four pairs, eight
//                          columns), holds q[b] of them in registers and one accumulator per column across j = 0 .. K-1.
//   kg_score_grad_table_kernel
//                          grid (N, column blocks).  The same ownership with the table row in registers; the occurrences of
//                          entity e come from the inverted index (occ_ptr, occ_pos: flat positions b K + j ascending), chunks
//                          of 512 are summed from +0 and the partials added in chunk order.  Every row of grad_table is
//                          written, zeros included: no memset precedes the launch.
// The vector instantiations (16-byte loads) run where every row starts on 16 bytes (base address and D % 4; cl2: D % 8, so that
// the imaginary half does too); the scalar ones otherwise.  Terms map to slots and to accumulators alike in both, so the bits
// are equal.  Every global read is bounds-checked: an id outside [0, N) scores NaN and adds nothing, a position outside
// [0, B K) and list bounds outside [0, B K] are passed over or clamped.
#include "common.h"
#include "kgscore_law.h"

namespace cogdl {
namespace ks = cogdl_kgscore;
namespace kgl = cogdl_kgrank;

constexpr int kKsThreads = 256;
constexpr int kKsWaves = kKsThreads / kWave;
constexpr int kKsInFlight = 4;                   // groups of four terms a lane loads before it folds them
constexpr int kKsBlockTerms = kKsThreads * 4;    // terms per workgroup of the two gradient kernels

// four consecutive floats of a row from k on; VEC: one 16-byte load (k + 3 < limit by construction), else guarded scalars
template <bool VEC>
__device__ __forceinline__ void ks_load4(const float *__restrict__ row, int64_t k, int64_t limit, float (&v)[4]) {
    if constexpr (VEC) {
        const float4 x = *reinterpret_cast<const float4 *>(row + k);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = k + c < limit ? row[k + c] : 0.0f;
    }
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(kKsThreads) void kg_score_kernel(const float *__restrict__ q, const float *__restrict__ table,
                                                              const int32_t *__restrict__ idx, int64_t B, int64_t K, int64_t N,
                                                              int64_t D, float gamma, float *__restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) float ks_q[];  // q[b], D floats
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x;
    const float *qb = q + b * D;
    for (int64_t k = threadIdx.x; k < D; k += kKsThreads) ks_q[k] = qb[k];
    __syncthreads();
    const int64_t half = D / 2;
    const int64_t terms = KIND == kgl::kCl2 ? half : D;
    const int64_t groups = (terms + 3) >> 2;
    for (int64_t j = wave; j < K; j += kKsWaves) {
        const int64_t e = idx[b * K + j];  // wave-uniform
        if (e < 0 || e >= N) {
            if (lane == 0) scores[b * K + j] = __builtin_nanf("");
            continue;
        }
        const float *trow = table + e * D;
        float acc = 0.0f;
        for (int64_t g0 = lane; g0 < groups; g0 += (int64_t)kWave * kKsInFlight) {
            float ta[kKsInFlight][4], tb[kKsInFlight][4];
#pragma unroll
            for (int u = 0; u < kKsInFlight; ++u) {
                const int64_t gi = g0 + (int64_t)kWave * u;
                if (gi < groups) {
                    ks_load4<VEC>(trow, 4 * gi, terms, ta[u]);
                    if constexpr (KIND == kgl::kCl2) ks_load4<VEC>(trow + half, 4 * gi, terms, tb[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kKsInFlight; ++u) {
                const int64_t gi = g0 + (int64_t)kWave * u;
                if (gi < groups) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int64_t k = 4 * gi + c;
                        if (VEC || k < terms) {
                            if constexpr (KIND == kgl::kDot) acc = kgl::dot_step(acc, ks_q[k], ta[u][c]);
                            else if constexpr (KIND == kgl::kL1) acc = kgl::l1_step(acc, ks_q[k], ta[u][c]);
                            else acc = kgl::cl2_step(acc, ks_q[k], ks_q[k + half], ta[u][c], tb[u][c]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int off = kWave / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, kWave);
        if (lane == 0) scores[b * K + j] = kgl::finish(KIND, gamma, acc);
    }
}

// the term a thread owns as its c-th: four consecutive ones where rows are read 16 bytes at a time, else strided by the
// workgroup so that neighbouring lanes read neighbouring floats (a sum per element: the ownership changes no bit)
template <bool VEC>
__device__ __forceinline__ int64_t ks_term(int64_t block0, int c) {
    return VEC ? block0 + 4 * (int64_t)threadIdx.x + c : block0 + (int64_t)threadIdx.x + (int64_t)kKsThreads * c;
}

// the thread's four terms of a row: a[c] (and b[c], the imaginary column, for cl2); zero beyond `terms`
template <int KIND, bool VEC>
__device__ __forceinline__ void ks_load_terms(const float *__restrict__ row, int64_t block0, int64_t terms, int64_t half,
                                              float (&a)[4], float (&b)[4]) {
    if constexpr (VEC) {
        const int64_t k = ks_term<true>(block0, 0);
        if (k < terms) {
            ks_load4<true>(row, k, terms, a);
            if constexpr (KIND == kgl::kCl2) ks_load4<true>(row + half, k, terms, b);
            else b[0] = b[1] = b[2] = b[3] = 0.0f;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) a[c] = 0.0f, b[c] = 0.0f;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t k = ks_term<false>(block0, c);
            a[c] = k < terms ? row[k] : 0.0f;
            b[c] = (KIND == kgl::kCl2 && k < terms) ? row[k + half] : 0.0f;
        }
    }
}

template <int KIND, bool VEC>
__device__ __forceinline__ void ks_put_terms(float *__restrict__ row, int64_t block0, int64_t terms, int64_t half,
                                               const float (&a)[4], const float (&b)[4]) {
    if constexpr (VEC) {
        const int64_t k = ks_term<true>(block0, 0);
        if (k < terms) {
            *reinterpret_cast<float4 *>(row + k) = make_float4(a[0], a[1], a[2], a[3]);
            if constexpr (KIND == kgl::kCl2) *reinterpret_cast<float4 *>(row + half + k) = make_float4(b[0], b[1], b[2], b[3]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t k = ks_term<false>(block0, c);
            if (k < terms) {
                row[k] = a[c];
                if constexpr (KIND == kgl::kCl2) row[k + half] = b[c];
            }
        }
    }
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(kKsThreads) void kg_score_grad_q_kernel(const float *__restrict__ q, const float *__restrict__ table,
                                                                     const int32_t *__restrict__ idx, const float *__restrict__ g,
                                                                     int64_t B, int64_t K, int64_t N, int64_t D,
                                                                     float *__restrict__ grad_q) {
    const int64_t b = blockIdx.x, block0 = (int64_t)blockIdx.y * kKsBlockTerms;
    const int64_t half = D / 2;
    const int64_t terms = KIND == kgl::kCl2 ? half : D;
    float qa[4], qb[4], acc_a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc_b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    ks_load_terms<KIND, VEC>(q + b * D, block0, terms, half, qa, qb);
    for (int64_t j0 = 0; j0 < K; j0 += kKsInFlight) {
        float ta[kKsInFlight][4], tb[kKsInFlight][4], gv[kKsInFlight];
        bool ok[kKsInFlight];
#pragma unroll
        for (int u = 0; u < kKsInFlight; ++u) {
            const int64_t j = j0 + u;
            const int64_t e = j < K ? (int64_t)idx[b * K + j] : -1;  // workgroup-uniform
            ok[u] = e >= 0 && e < N;
            gv[u] = ok[u] ? g[b * K + j] : 0.0f;
            ks_load_terms<KIND, VEC>(table + (ok[u] ? e : 0) * D, block0, ok[u] ? terms : 0, half, ta[u], tb[u]);
        }
#pragma unroll
        for (int u = 0; u < kKsInFlight; ++u) {
            if (ok[u]) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float da, db;
                    ks::partial_q(KIND, qa[c], qb[c], ta[u][c], tb[u][c], &da, &db);
                    acc_a[c] = ks::add_contribution(acc_a[c], gv[u], da);
                    if constexpr (KIND == kgl::kCl2) acc_b[c] = ks::add_contribution(acc_b[c], gv[u], db);
                }
            }
        }
    }
    ks_put_terms<KIND, VEC>(grad_q + b * D, block0, terms, half, acc_a, acc_b);
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(kKsThreads) void kg_score_grad_table_kernel(const float *__restrict__ q, const float *__restrict__ table,
                                                                         const float *__restrict__ g,
                                                                         const int32_t *__restrict__ occ_ptr,
                                                                         const int32_t *__restrict__ occ_pos, int64_t B, int64_t K,
                                                                         int64_t N, int64_t D, float *__restrict__ grad_table) {
    const int64_t e = blockIdx.x, block0 = (int64_t)blockIdx.y * kKsBlockTerms;
    const int64_t half = D / 2;
    const int64_t terms = KIND == kgl::kCl2 ? half : D;
    const int64_t BK = B * K;
    float ta[4], tb[4], tot_a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, tot_b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    ks_load_terms<KIND, VEC>(table + e * D, block0, terms, half, ta, tb);
    int64_t lo = occ_ptr[e], hi = occ_ptr[e + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > BK ? BK : hi;
    for (int64_t c0 = lo; c0 < hi; c0 += ks::kChunk) {
        const int64_t c1 = c0 + ks::kChunk < hi ? c0 + ks::kChunk : hi;
        float acc_a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc_b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t i0 = c0; i0 < c1; i0 += kKsInFlight) {
            float qa[kKsInFlight][4], qb[kKsInFlight][4], gv[kKsInFlight];
            bool ok[kKsInFlight];
#pragma unroll
            for (int u = 0; u < kKsInFlight; ++u) {
                const int64_t i = i0 + u;
                const int64_t p = i < c1 ? (int64_t)occ_pos[i] : -1;  // workgroup-uniform
                ok[u] = p >= 0 && p < BK;
                gv[u] = ok[u] ? g[p] : 0.0f;
                ks_load_terms<KIND, VEC>(q + (ok[u] ? p / K : 0) * D, block0, ok[u] ? terms : 0, half, qa[u], qb[u]);
            }
#pragma unroll
            for (int u = 0; u < kKsInFlight; ++u) {
                if (ok[u]) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float da, db;
                        ks::partial_t(KIND, qa[u][c], qb[u][c], ta[c], tb[c], &da, &db);
                        acc_a[c] = ks::add_contribution(acc_a[c], gv[u], da);
                        if constexpr (KIND == kgl::kCl2) acc_b[c] = ks::add_contribution(acc_b[c], gv[u], db);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            tot_a[c] = tot_a[c] + acc_a[c];
            tot_b[c] = tot_b[c] + acc_b[c];
        }
    }
    ks_put_terms<KIND, VEC>(grad_table + e * D, block0, terms, half, tot_a, tot_b);
}

// 16-byte loads where every row of every float operand starts on 16 bytes
static bool ks_vector_ok(int kind, int64_t D, const void *a, const void *b, const void *c) {
    if (D % (kind == kgl::kCl2 ? 8 : 4)) return false;
    return aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(c, 16);
}

template <typename F>
static void ks_dispatch(int kind, bool vec, F &&launch) {
    if (kind == kgl::kDot) vec ? launch.template operator()<kgl::kDot, true>() : launch.template operator()<kgl::kDot, false>();
    else if (kind == kgl::kL1) vec ? launch.template operator()<kgl::kL1, true>() : launch.template operator()<kgl::kL1, false>();
    else vec ? launch.template operator()<kgl::kCl2, true>() : launch.template operator()<kgl::kCl2, false>();
}

static unsigned ks_column_blocks(int kind, int64_t D) {
    const int64_t terms = ks::terms_of(kind, D);
    return (unsigned)std::max<int64_t>(1, (terms + kKsBlockTerms - 1) / kKsBlockTerms);
}

struct KsScoreLaunch {
    const float *q, *table;
    const int32_t *idx;
    int64_t B, K, N, D;
    float gamma;
    float *scores;
    hipStream_t s;
    template <int KIND, bool VEC>
    void operator()() const {
        hipLaunchKernelGGL((kg_score_kernel<KIND, VEC>), dim3((unsigned)B), dim3(kKsThreads), (size_t)D * sizeof(float), s, q, table,
                           idx, B, K, N, D, gamma, scores);
    }
};

struct KsGradQLaunch {
    const float *q, *table;
    const int32_t *idx;
    const float *g;
    int64_t B, K, N, D;
    int kind;
    float *grad_q;
    hipStream_t s;
    template <int KIND, bool VEC>
    void operator()() const {
        hipLaunchKernelGGL((kg_score_grad_q_kernel<KIND, VEC>), dim3((unsigned)B, ks_column_blocks(kind, D)), dim3(kKsThreads), 0, s,
                           q, table, idx, g, B, K, N, D, grad_q);
    }
};

struct KsGradTableLaunch {
    const float *q, *table, *g;
    const int32_t *occ_ptr, *occ_pos;
    int64_t B, K, N, D;
    int kind;
    float *grad_table;
    hipStream_t s;
    template <int KIND, bool VEC>
    void operator()() const {
        hipLaunchKernelGGL((kg_score_grad_table_kernel<KIND, VEC>), dim3((unsigned)N, ks_column_blocks(kind, D)), dim3(kKsThreads),
                           0, s, q, table, g, occ_ptr, occ_pos, B, K, N, D, grad_table);
    }
};

static int ks_sizes(int64_t B, int64_t K, int64_t N, int64_t D, int kind) {
    const int rc = ks::sizes_status(B, K, N, D, kind);
    return rc == 0 ? COGDL_HIP_OK : (rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_kg_score(const float *q, const float *table, const int32_t *idx, int64_t B, int64_t K, int64_t N,
                                  int64_t D, int kind, float gamma, float *scores, void *stream) {
    const int rc = ks_sizes(B, K, N, D, kind);
    if (rc != COGDL_HIP_OK) return rc;
    if (B == 0 || K == 0) return COGDL_HIP_OK;
    if (!idx || !scores || (D > 0 && (!q || (N > 0 && !table)))) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 4) || !aligned_to(table, 4) || !aligned_to(idx, 4) || !aligned_to(scores, 4)) return COGDL_HIP_EALIGN;
    if (D > ks::kMaxD) return COGDL_HIP_ERANGE;
    // (q is copied to LDS by scalars: only the table's rows are read 16 bytes at a time)
    ks_dispatch(kind, ks_vector_ok(kind, D, table, nullptr, nullptr), KsScoreLaunch{q, table, idx, B, K, N, D, gamma, scores,
                                                                                (hipStream_t)stream});
    return launch_status();
}

extern "C" int cogdl_hip_kg_score_grad_q(const float *q, const float *table, const int32_t *idx, const float *g, int64_t B,
                                         int64_t K, int64_t N, int64_t D, int kind, float *grad_q, void *stream) {
    const int rc = ks_sizes(B, K, N, D, kind);
    if (rc != COGDL_HIP_OK) return rc;
    if (B == 0 || D == 0) return COGDL_HIP_OK;
    if (!q || !grad_q || (K > 0 && (!idx || !g || (N > 0 && !table)))) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 4) || !aligned_to(table, 4) || !aligned_to(idx, 4) || !aligned_to(g, 4) || !aligned_to(grad_q, 4))
        return COGDL_HIP_EALIGN;
    if (D > ks::kMaxD) return COGDL_HIP_ERANGE;
    ks_dispatch(kind, ks_vector_ok(kind, D, q, table, grad_q), KsGradQLaunch{q, table, idx, g, B, K, N, D, kind, grad_q,
                                                                              (hipStream_t)stream});
    return launch_status();
}

extern "C" int cogdl_hip_kg_score_grad_table(const float *q, const float *table, const float *g, const int32_t *occ_ptr,
                                             const int32_t *occ_pos, int64_t B, int64_t K, int64_t N, int64_t D, int kind,
                                             float *grad_table, void *stream) {
    const int rc = ks_sizes(B, K, N, D, kind);
    if (rc != COGDL_HIP_OK) return rc;
    if (N == 0 || D == 0) return COGDL_HIP_OK;
    if (!table || !grad_table || !occ_ptr || (B * K > 0 && (!q || !g || !occ_pos))) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 4) || !aligned_to(table, 4) || !aligned_to(g, 4) || !aligned_to(occ_ptr, 4) || !aligned_to(occ_pos, 4) ||
        !aligned_to(grad_table, 4))
        return COGDL_HIP_EALIGN;
    if (D > ks::kMaxD) return COGDL_HIP_ERANGE;
    ks_dispatch(kind, ks_vector_ok(kind, D, q, table, grad_table), KsGradTableLaunch{q, table, g, occ_ptr, occ_pos, B, K, N, D, kind,
                                                                                     grad_table, (hipStream_t)stream});
    return launch_status();
}
