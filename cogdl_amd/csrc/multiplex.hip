// multiplex.hip -- the fused multiplex (typed-edge) attention embedding: GATNE's model step (cogdl/models/emb/gatne.py:221-241)
// without its [B, T, S, T, U] gather.  The reference indexes the type table with the whole neighbour block, keeps the diagonal of
// the result, runs about fifteen small kernels on it and, backward, scatters [B, T, S, T, U] rows with float atomics.  Here the
// forward is one launch, nothing larger than [B, T, U] is written, and no gradient uses an atomic: the order of every float32
// operation is multiplex_law.h's, so results are equal from run to run and do not depend on the launch geometry.
//
//   multiplex_fwd_kernel          one wave (one workgroup of 64 lanes) per sample.  The T U neighbour sums, the T A tanh units,
//                                 the softmax over T and the U-vector m live in LDS; y is 16 registers per lane.  Rows are tiny
//                                 (U = 10, D = 200 at the reference's defaults): the kernel is latency-bound, so it is one launch
//                                 and every id is checked before its row is read.
//   multiplex_bwd_sample_kernel   one wave per sample: g_y [B, D], g_c [B, T, U], g_pre [B, T, A], g_e [B, T].
//   multiplex_bwd_weights_kernel  grad trans_w, grad att_w1, grad att_w2 from the samples of each type in ascending b; a workgroup
//                                 sums eight of the law's chunks of one type's list at once and adds the partials in order.
//   multiplex_bwd_node_kernel     one thread per element of grad node_emb, walking the occurrences of its node in inputs.
//   multiplex_bwd_type_kernel     one thread per element of grad type_emb, walking the neighbour slots that name its (node, type).
// The three list kernels write every element, zeros included: no memset precedes them.  All loads are 4-byte scalars, so tables
// that start mid-allocation are served as they are.
#include "common.h"
#include "multiplex_law.h"

namespace cogdl {
namespace mx = cogdl_multiplex;

constexpr int kMxPerLane = (int)(mx::kMaxD / kWave);  // y values a lane holds
constexpr int kMxThreads = 256;                       // the list kernels

__device__ __forceinline__ float mx_butterfly(float v) {
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, kWave);
    return v;
}

// LDS floats of one wave: c [T U] | pre-activation side [T A] | three T-vectors | one U-vector
static size_t mx_lds_bytes(int64_t T, int64_t U, int64_t A) { return (size_t)(T * U + T * A + 3 * T + U) * sizeof(float); }

__global__ __launch_bounds__(kWave) void multiplex_fwd_kernel(
    const float *__restrict__ node_emb, const float *__restrict__ type_emb, const float *__restrict__ trans_w,
    const float *__restrict__ att_w1, const float *__restrict__ att_w2, const int32_t *__restrict__ neigh,
    const int32_t *__restrict__ inputs, const int32_t *__restrict__ types, int64_t B, int64_t N, int T, int S, int U, int A, int D,
    float *__restrict__ c_out, float *__restrict__ h_out, float *__restrict__ att_out, float *__restrict__ m_out,
    float *__restrict__ nrm_out, float *__restrict__ out) {
    extern __shared__ float mx_lds[];
    float *c = mx_lds, *h = c + T * U, *e = h + T * A, *att = e + T, *m = att + T;
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t x = inputs[b], t = types[b];  // wave-uniform
    const int TS = T * S, TU = T * U, TA = T * A;
    bool ok = x >= 0 && x < N && t >= 0 && t < T;
    if (ok) {
        const int32_t *nb = neigh + x * TS;
        bool good = true;
        for (int k = lane; k < TS; k += kWave) {
            const int64_t n = nb[k];
            good = good && n >= 0 && n < N;
        }
        ok = __all(good) != 0;
    }
    if (!ok) {  // (uniform: the whole wave leaves in front of the first barrier)
        for (int d = lane; d < D; d += kWave) out[b * D + d] = __builtin_nanf("");
        if (lane == 0) nrm_out[b] = -1.0f;
        return;
    }
    for (int idx = lane; idx < TU; idx += kWave) {
        const int i = idx / U, u = idx - i * U;
        const int32_t *nbi = neigh + (x * T + i) * S;
        float acc = 0.0f;
        for (int s = 0; s < S; ++s) {
            const int64_t n = nbi[s];
            acc = acc + type_emb[(n * T + i) * U + u];
        }
        c[idx] = acc;
        c_out[b * TU + idx] = acc;
    }
    __syncthreads();
    for (int idx = lane; idx < TA; idx += kWave) {
        const int i = idx / A, a = idx - i * A;
        float acc = 0.0f;
        for (int u = 0; u < U; ++u) {
            const float p = c[i * U + u] * att_w1[(t * U + u) * A + a];
            acc = acc + p;
        }
        const float hv = tanhf(acc);
        h[idx] = hv;
        h_out[b * TA + idx] = hv;
    }
    __syncthreads();
    if (lane < T) {  // (T lanes, A terms: float64 costs nothing here, and the softmax turns an error of e into one of att)
        double acc = 0.0;
        for (int a = 0; a < A; ++a) {
            const double p = (double)h[lane * A + a] * (double)att_w2[t * A + a];
            acc = acc + p;
        }
        e[lane] = (float)acc;
    }
    __syncthreads();
    if (lane < T) {
        float top = e[0];
        for (int i = 1; i < T; ++i) top = fmaxf(top, e[i]);
        float z = 0.0f;
        for (int i = 0; i < T; ++i) z = z + expf(e[i] - top);
        const float av = expf(e[lane] - top) / z;
        att[lane] = av;
        att_out[b * T + lane] = av;
    }
    __syncthreads();
    if (lane < U) {
        float acc = 0.0f;
        for (int i = 0; i < T; ++i) {
            const float p = att[i] * c[i * U + lane];
            acc = acc + p;
        }
        m[lane] = acc;
        m_out[b * U + lane] = acc;
    }
    __syncthreads();
    float y[kMxPerLane];
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < kMxPerLane; ++k) {
        const int d = lane + kWave * k;
        y[k] = 0.0f;
        if (d < D) {
            float acc = 0.0f;
            for (int u = 0; u < U; ++u) {
                const float p = m[u] * trans_w[(t * U + u) * D + d];
                acc = acc + p;
            }
            y[k] = node_emb[x * D + d] + acc;
            const float sq = y[k] * y[k];
            ss = ss + sq;
        }
    }
    const float nrm = sqrtf(mx_butterfly(ss));
    const float dn = fmaxf(nrm, mx::kEps);
#pragma unroll
    for (int k = 0; k < kMxPerLane; ++k) {
        const int d = lane + kWave * k;
        if (d < D) out[b * D + d] = y[k] / dn;
    }
    if (lane == 0) nrm_out[b] = nrm;
}

__global__ __launch_bounds__(kWave) void multiplex_bwd_sample_kernel(
    const float *__restrict__ trans_w, const float *__restrict__ att_w1, const float *__restrict__ att_w2,
    const int32_t *__restrict__ types, const float *__restrict__ g, const float *__restrict__ out, const float *__restrict__ nrm_s,
    const float *__restrict__ c_s, const float *__restrict__ h_s, const float *__restrict__ att_s, int64_t B, int T, int U, int A,
    int D, float *__restrict__ g_y, float *__restrict__ g_c, float *__restrict__ g_pre, float *__restrict__ g_e) {
    extern __shared__ float mx_lds[];
    float *c = mx_lds, *gpre = c + T * U, *gatt = gpre + T * A, *att = gatt + T, *ge = att + T, *gm = ge + T;
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t t = types[b];
    const float nrm = nrm_s[b];
    const int TU = T * U, TA = T * A;
    if (nrm < 0.0f || t < 0 || t >= T) {  // a sample the forward refused: it contributes to no gradient
        for (int d = lane; d < D; d += kWave) g_y[b * D + d] = 0.0f;
        for (int k = lane; k < TU; k += kWave) g_c[b * TU + k] = 0.0f;
        for (int k = lane; k < TA; k += kWave) g_pre[b * TA + k] = 0.0f;
        if (lane < T) g_e[b * T + lane] = 0.0f;
        return;
    }
    float gy[kMxPerLane], ov[kMxPerLane];
    float dot = 0.0f;
#pragma unroll
    for (int k = 0; k < kMxPerLane; ++k) {
        const int d = lane + kWave * k;
        gy[k] = 0.0f, ov[k] = 0.0f;
        if (d < D) {
            gy[k] = g[b * D + d];
            ov[k] = out[b * D + d];
            const float p = gy[k] * ov[k];
            dot = dot + p;
        }
    }
    dot = mx_butterfly(dot);
    const bool through_norm = !(nrm < mx::kEps);
    const float dn = through_norm ? nrm : mx::kEps;
#pragma unroll
    for (int k = 0; k < kMxPerLane; ++k) {
        const int d = lane + kWave * k;
        if (d < D) {
            float v = gy[k];
            if (through_norm) {
                const float p = ov[k] * dot;
                v = v - p;
            }
            gy[k] = v / dn;
            g_y[b * D + d] = gy[k];
        }
    }
    float gmv = 0.0f;
    for (int u = 0; u < U; ++u) {
        const float *w = trans_w + (t * U + u) * D;
        float part = 0.0f;
#pragma unroll
        for (int k = 0; k < kMxPerLane; ++k) {
            const int d = lane + kWave * k;
            if (d < D) {
                const float p = gy[k] * w[d];
                part = part + p;
            }
        }
        part = mx_butterfly(part);
        if (lane == u) gmv = part;
    }
    if (lane < U) gm[lane] = gmv;
    for (int k = lane; k < TU; k += kWave) c[k] = c_s[b * TU + k];
    if (lane < T) att[lane] = att_s[b * T + lane];
    __syncthreads();
    if (lane < T) {
        float acc = 0.0f;
        for (int u = 0; u < U; ++u) {
            const float p = gm[u] * c[lane * U + u];
            acc = acc + p;
        }
        gatt[lane] = acc;
    }
    __syncthreads();
    if (lane < T) {
        float ds = 0.0f;
        for (int i = 0; i < T; ++i) {
            const float p = att[i] * gatt[i];
            ds = ds + p;
        }
        const float v = att[lane] * (gatt[lane] - ds);
        ge[lane] = v;
        g_e[b * T + lane] = v;
    }
    __syncthreads();
    for (int idx = lane; idx < TA; idx += kWave) {
        const int i = idx / A, a = idx - i * A;
        const float hv = h_s[b * TA + idx];
        const float gh = ge[i] * att_w2[t * A + a];
        const float hh = hv * hv;
        const float v = gh * (1.0f - hh);
        gpre[idx] = v;
        g_pre[b * TA + idx] = v;
    }
    __syncthreads();
    for (int idx = lane; idx < TU; idx += kWave) {
        const int i = idx / U, u = idx - i * U;
        float acc = att[i] * gm[u];
        for (int a = 0; a < A; ++a) {
            const float p = gpre[i * A + a] * att_w1[(t * U + u) * A + a];
            acc = acc + p;
        }
        g_c[b * TU + idx] = acc;
    }
}

// One list of the inverted index, summed as the law says.  `term(pos, acc)` adds the terms of the entry at position `pos`
// (already moved to the list's own origin and range-checked against `limit`) to acc and returns it.
template <typename F>
__device__ __forceinline__ float mx_list_sum(const int32_t *__restrict__ occ_ptr, const int32_t *__restrict__ occ_pos, int64_t key,
                                             int64_t pos_base, int64_t limit, int64_t P, F &&term) {
    int64_t lo = occ_ptr[key], hi = occ_ptr[key + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > P ? P : hi;
    float tot = 0.0f;
    for (int64_t c0 = lo; c0 < hi; c0 += mx::kChunk) {
        const int64_t c1 = c0 + mx::kChunk < hi ? c0 + mx::kChunk : hi;
        float acc = 0.0f;
        for (int64_t i = c0; i < c1; ++i) {
            const int64_t p = (int64_t)occ_pos[i] - pos_base;
            if (p >= 0 && p < limit) acc = term(p, acc);
        }
        tot = tot + acc;
    }
    return tot;
}

// The weight gradients.  grid (blocks of one family of one type, T): blockIdx.y is the type, whose sample list every thread of the
// workgroup walks; blockIdx.x selects kMxWElems consecutive elements of ONE of the three gradients of that type (trans_w first,
// then att_w1, then att_w2: a workgroup never mixes two).  The law's chunks are independent until their partials are added, so
// kMxWSlots of them are summed at once: thread (slot, element) sums chunk `round + slot` of its element, the partials go through
// LDS, and the slot-0 thread adds them in ascending chunk order.  The bits are the law's whatever the geometry.
// occ_ptr points at the list of type 0 (T + 1 bounds are read); positions are pos_base + b.
constexpr int kMxWSlots = 8;
constexpr int kMxWElems = kMxThreads / kMxWSlots;

template <typename F>
__device__ __forceinline__ float mx_chunk_sum(const int32_t *__restrict__ occ_pos, int64_t c0, int64_t c1, int64_t pos_base,
                                              int64_t limit, F &&term) {
    float acc = 0.0f;
    for (int64_t i = c0; i < c1; ++i) {
        const int64_t p = (int64_t)occ_pos[i] - pos_base;
        if (p >= 0 && p < limit) acc = term(p, acc);
    }
    return acc;
}

__global__ __launch_bounds__(kMxThreads) void multiplex_bwd_weights_kernel(
    const float *__restrict__ m_s, const float *__restrict__ g_y, const float *__restrict__ c_s, const float *__restrict__ g_pre,
    const float *__restrict__ g_e, const float *__restrict__ h_s, const int32_t *__restrict__ occ_ptr,
    const int32_t *__restrict__ occ_pos, int64_t pos_base, int64_t P, int64_t B, int T, int U, int A, int D,
    float *__restrict__ g_trans, float *__restrict__ g_w1, float *__restrict__ g_w2) {
    __shared__ float part[kMxWSlots][kMxWElems];
    const int el = threadIdx.x % kMxWElems, slot = threadIdx.x / kMxWElems;
    const int64_t t = blockIdx.y;
    const int n_trans = U * D, n_w1 = U * A, n_w2 = A;  // elements per type
    const int b_trans = (n_trans + kMxWElems - 1) / kMxWElems, b_w1 = (n_w1 + kMxWElems - 1) / kMxWElems;
    int family, e;  // workgroup-uniform family; e: the thread's element inside the type's slice
    if ((int)blockIdx.x < b_trans) family = 0, e = (int)blockIdx.x * kMxWElems + el;
    else if ((int)blockIdx.x < b_trans + b_w1) family = 1, e = ((int)blockIdx.x - b_trans) * kMxWElems + el;
    else family = 2, e = ((int)blockIdx.x - b_trans - b_w1) * kMxWElems + el;
    const int count = family == 0 ? n_trans : (family == 1 ? n_w1 : n_w2);
    float *dst = family == 0 ? g_trans : (family == 1 ? g_w1 : g_w2);
    if (!dst) return;  // (uniform: this gradient was not asked for)
    const bool live = e < count;
    const int width = family == 0 ? D : A;  // trans_w: (u, d); att_w1: (u, a); att_w2: (0, a)
    const int u = live ? e / width : 0, col = live ? e - u * width : 0;
    int64_t lo = occ_ptr[t], hi = occ_ptr[t + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > P ? P : hi;
    const int64_t chunks = hi > lo ? (hi - lo + mx::kChunk - 1) / mx::kChunk : 0;
    float tot = 0.0f;
    for (int64_t round = 0; round < chunks; round += kMxWSlots) {  // (uniform bounds: every thread meets every barrier)
        const int64_t chunk = round + slot;
        float acc = 0.0f;
        if (live && chunk < chunks) {
            const int64_t c0 = lo + chunk * mx::kChunk, c1 = c0 + mx::kChunk < hi ? c0 + mx::kChunk : hi;
            if (family == 0) {
                acc = mx_chunk_sum(occ_pos, c0, c1, pos_base, B, [&](int64_t b, float a_) {
                    const float p = m_s[b * U + u] * g_y[b * D + col];
                    return a_ + p;
                });
            } else if (family == 1) {
                acc = mx_chunk_sum(occ_pos, c0, c1, pos_base, B, [&](int64_t b, float a_) {
                    for (int i = 0; i < T; ++i) {
                        const float p = c_s[(b * T + i) * U + u] * g_pre[(b * T + i) * A + col];
                        a_ = a_ + p;
                    }
                    return a_;
                });
            } else {
                acc = mx_chunk_sum(occ_pos, c0, c1, pos_base, B, [&](int64_t b, float a_) {
                    for (int i = 0; i < T; ++i) {
                        const float p = g_e[b * T + i] * h_s[(b * T + i) * A + col];
                        a_ = a_ + p;
                    }
                    return a_;
                });
            }
        }
        part[slot][el] = acc;
        __syncthreads();
        if (slot == 0) {
            const int64_t left = chunks - round;
            const int n = left < kMxWSlots ? (int)left : kMxWSlots;
            for (int k = 0; k < n; ++k) tot = tot + part[k][el];
        }
        __syncthreads();
    }
    if (slot == 0 && live) dst[t * count + e] = tot;
}

// occ_ptr points at the list of node 0 (N + 1 bounds are read); positions are pos_base + b
__global__ __launch_bounds__(kMxThreads) void multiplex_bwd_node_kernel(const float *__restrict__ g_y,
                                                                        const int32_t *__restrict__ occ_ptr,
                                                                        const int32_t *__restrict__ occ_pos, int64_t pos_base,
                                                                        int64_t P, int64_t B, int64_t N, int D,
                                                                        float *__restrict__ g_node) {
    const int64_t idx = (int64_t)blockIdx.x * kMxThreads + threadIdx.x;
    if (idx >= N * D) return;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    g_node[idx] = mx_list_sum(occ_ptr, occ_pos, n, pos_base, B, P, [&](int64_t b, float acc) { return acc + g_y[b * D + d]; });
}

// occ_ptr points at the list of key 0 = (node 0, type 0) (N T + 1 bounds are read); positions are pos_base + (b T + i) S + s
__global__ __launch_bounds__(kMxThreads) void multiplex_bwd_type_kernel(const float *__restrict__ g_c,
                                                                        const int32_t *__restrict__ occ_ptr,
                                                                        const int32_t *__restrict__ occ_pos, int64_t pos_base,
                                                                        int64_t P, int64_t B, int64_t N, int T, int S, int U,
                                                                        float *__restrict__ g_type) {
    const int64_t idx = (int64_t)blockIdx.x * kMxThreads + threadIdx.x;
    if (idx >= N * T * U) return;
    const int64_t key = idx / U;
    const int u = (int)(idx - key * U);
    g_type[idx] = mx_list_sum(occ_ptr, occ_pos, key, pos_base, B * T * S, P,
                              [&](int64_t p, float acc) { return acc + g_c[(p / S) * U + u]; });
}

static int mx_sizes(int64_t B, int64_t N, int64_t T, int64_t S, int64_t U, int64_t A, int64_t D) {
    const int rc = mx::sizes_status(B, N, T, S, U, A, D);
    return rc == 0 ? COGDL_HIP_OK : (rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE);
}

static bool mx_aligned(std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if (!aligned_to(p, 4)) return false;
    return true;
}

static bool mx_any_null(std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if (!p) return true;
    return false;
}

static unsigned mx_blocks(int64_t elements) { return (unsigned)((elements + kMxThreads - 1) / kMxThreads); }

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_multiplex_fwd(const float *node_emb, const float *type_emb, const float *trans_w, const float *att_w1,
                                       const float *att_w2, const int32_t *neigh, const int32_t *inputs, const int32_t *types,
                                       int64_t B, int64_t N, int64_t T, int64_t S, int64_t U, int64_t A, int64_t D, float *c,
                                       float *h, float *att, float *m, float *nrm, float *out, void *stream) {
    const int rc = mx_sizes(B, N, T, S, U, A, D);
    if (rc != COGDL_HIP_OK) return rc;
    if (B == 0) return COGDL_HIP_OK;
    if (mx_any_null({trans_w, att_w1, att_w2, inputs, types, c, h, att, m, nrm, out})) return COGDL_HIP_EINVAL;
    if (N > 0 && mx_any_null({node_emb, type_emb, neigh})) return COGDL_HIP_EINVAL;
    if (!mx_aligned({node_emb, type_emb, trans_w, att_w1, att_w2, neigh, inputs, types, c, h, att, m, nrm, out}))
        return COGDL_HIP_EALIGN;
    hipLaunchKernelGGL(multiplex_fwd_kernel, dim3((unsigned)B), dim3(kWave), mx_lds_bytes(T, U, A), (hipStream_t)stream, node_emb,
                       type_emb, trans_w, att_w1, att_w2, neigh, inputs, types, B, N, (int)T, (int)S, (int)U, (int)A, (int)D, c, h,
                       att, m, nrm, out);
    return launch_status();
}

extern "C" int cogdl_hip_multiplex_bwd_sample(const float *trans_w, const float *att_w1, const float *att_w2, const int32_t *types,
                                              const float *g, const float *out, const float *nrm, const float *c, const float *h,
                                              const float *att, int64_t B, int64_t T, int64_t U, int64_t A, int64_t D, float *g_y,
                                              float *g_c, float *g_pre, float *g_e, void *stream) {
    const int rc = mx_sizes(B, 0, T, 1, U, A, D);
    if (rc != COGDL_HIP_OK) return rc;
    if (B == 0) return COGDL_HIP_OK;
    if (mx_any_null({trans_w, att_w1, att_w2, types, g, out, nrm, c, h, att, g_y, g_c, g_pre, g_e})) return COGDL_HIP_EINVAL;
    if (!mx_aligned({trans_w, att_w1, att_w2, types, g, out, nrm, c, h, att, g_y, g_c, g_pre, g_e})) return COGDL_HIP_EALIGN;
    hipLaunchKernelGGL(multiplex_bwd_sample_kernel, dim3((unsigned)B), dim3(kWave), mx_lds_bytes(T, U, A), (hipStream_t)stream,
                       trans_w, att_w1, att_w2, types, g, out, nrm, c, h, att, B, (int)T, (int)U, (int)A, (int)D, g_y, g_c, g_pre,
                       g_e);
    return launch_status();
}

extern "C" int cogdl_hip_multiplex_bwd_weights(const float *m, const float *g_y, const float *c, const float *g_pre,
                                               const float *g_e, const float *h, const int32_t *occ_ptr, const int32_t *occ_pos,
                                               int64_t pos_base, int64_t P, int64_t B, int64_t T, int64_t U, int64_t A, int64_t D,
                                               float *g_trans, float *g_w1, float *g_w2, void *stream) {
    const int rc = mx_sizes(B, 0, T, 1, U, A, D);
    if (rc != COGDL_HIP_OK) return rc;
    if (pos_base < 0 || P < 0 || P >= 0x7fffffff) return COGDL_HIP_EINVAL;
    if (!occ_ptr || (P > 0 && !occ_pos)) return COGDL_HIP_EINVAL;
    if (B > 0 && mx_any_null({m, g_y, c, g_pre, g_e, h})) return COGDL_HIP_EINVAL;
    if (!mx_aligned({m, g_y, c, g_pre, g_e, h, occ_ptr, occ_pos, g_trans, g_w1, g_w2})) return COGDL_HIP_EALIGN;
    if (!g_trans && !g_w1 && !g_w2) return COGDL_HIP_OK;
    const auto blocks_of = [](int64_t elements) { return (unsigned)((elements + kMxWElems - 1) / kMxWElems); };
    hipLaunchKernelGGL(multiplex_bwd_weights_kernel, dim3(blocks_of(U * D) + blocks_of(U * A) + blocks_of(A), (unsigned)T),
                       dim3(kMxThreads), 0, (hipStream_t)stream, m, g_y, c, g_pre, g_e, h, occ_ptr, occ_pos, pos_base, P, B, (int)T, (int)U, (int)A,
                       (int)D, g_trans, g_w1, g_w2);
    return launch_status();
}

extern "C" int cogdl_hip_multiplex_bwd_node(const float *g_y, const int32_t *occ_ptr, const int32_t *occ_pos, int64_t pos_base,
                                            int64_t P, int64_t B, int64_t N, int64_t D, float *g_node, void *stream) {
    const int rc = mx_sizes(B, N, 1, 1, 1, 1, D);
    if (rc != COGDL_HIP_OK) return rc;
    if (pos_base < 0 || P < 0 || P >= 0x7fffffff) return COGDL_HIP_EINVAL;
    if (N == 0) return COGDL_HIP_OK;
    if (!occ_ptr || !g_node || (P > 0 && !occ_pos) || (B > 0 && !g_y)) return COGDL_HIP_EINVAL;
    if (!mx_aligned({g_y, occ_ptr, occ_pos, g_node})) return COGDL_HIP_EALIGN;
    if (N * D > (int64_t)0x7fffffff * kMxThreads) return COGDL_HIP_ERANGE;
    hipLaunchKernelGGL(multiplex_bwd_node_kernel, dim3(mx_blocks(N * D)), dim3(kMxThreads), 0, (hipStream_t)stream, g_y, occ_ptr,
                       occ_pos, pos_base, P, B, N, (int)D, g_node);
    return launch_status();
}

extern "C" int cogdl_hip_multiplex_bwd_type(const float *g_c, const int32_t *occ_ptr, const int32_t *occ_pos, int64_t pos_base,
                                            int64_t P, int64_t B, int64_t N, int64_t T, int64_t S, int64_t U, float *g_type,
                                            void *stream) {
    const int rc = mx_sizes(B, N, T, S, U, 1, 1);
    if (rc != COGDL_HIP_OK) return rc;
    if (pos_base < 0 || P < 0 || P >= 0x7fffffff) return COGDL_HIP_EINVAL;
    if (N == 0) return COGDL_HIP_OK;
    if (!occ_ptr || !g_type || (P > 0 && !occ_pos) || (B > 0 && !g_c)) return COGDL_HIP_EINVAL;
    if (!mx_aligned({g_c, occ_ptr, occ_pos, g_type})) return COGDL_HIP_EALIGN;
    hipLaunchKernelGGL(multiplex_bwd_type_kernel, dim3(mx_blocks(N * T * U)), dim3(kMxThreads), 0, (hipStream_t)stream, g_c, occ_ptr,
                       occ_pos, pos_base, P, B, N, (int)T, (int)S, (int)U, g_type);
    return launch_status();
}
