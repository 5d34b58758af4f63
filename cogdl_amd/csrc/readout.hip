// readout.hip -- batched graph readout: x[N, F] node rows + a sorted `batch` vector -> one row (or k rows) per graph.
//   segment_ptr        batch -> ptr[B + 1] (a graph is a contiguous range of rows) and a validity flag
//   segment_pool       sum / mean / max over each range, forward and the gather that is its backward
//   sort_pool          per graph the k rows with the largest key, in descending key order, forward and backward
// The order of every addition and the sort order are readout_law.h's, shared with host_readout.cpp: both return the same
// bytes.  float32 only, no atomics, nothing read back, everything on the caller's stream.
//
// Pooling layout: lanes run along F (coalesced row loads), each lane adds its own column(s) in row order, so the
// association is the sequential one.  A wave is cut into groups of G lanes, G the power of two that covers a row (at most
// 64): narrow rows put 64 / G graphs into one wave, wide rows take several waves per graph.  Eight row loads are in flight
// per lane before the first add.  Rows whose width is a multiple of four floats go as 16-byte lanes.
#include "common.h"
#include "readout_law.h"

#include <initializer_list>

namespace cogdl {
namespace ro = cogdl_readout;

constexpr int kRoBlock = 256;                  // 4 waves
constexpr int kRoWaves = kRoBlock / kWave;
constexpr int kRoInFlight = 8;                 // row loads issued before the adds that consume them
static_assert(kRoWaves == ro::kWays, "the long-segment kernel gives one way to each wave");

struct Seg {
    int64_t lo, hi;
};
__device__ __forceinline__ Seg segment_of(const int32_t *__restrict__ ptr, int64_t g, int64_t N) {
    const int64_t lo = ro::clamp_row(ptr[g], 0, N);
    return {lo, ro::clamp_row(ptr[g + 1], lo, N)};
}

// ---- batch -> ptr ----------------------------------------------------------------------------------------------------
// Item i in [0, N]: every graph id in (batch[i - 1], batch[i]] starts at row i (batch[-1] = -1, batch[N] = B).
__global__ void segment_ptr_kernel(const int64_t *__restrict__ batch, int64_t N, int64_t B, int32_t *__restrict__ ptr,
                                   int *__restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= N; i += stride) {
        const int64_t prev = i > 0 ? batch[i - 1] : -1, cur = i < N ? batch[i] : B;
        if (i < N && (cur < 0 || cur >= B || cur < prev)) bad = true;
        const int64_t first = ro::clamp_row(prev, -1, B) + 1, last = ro::clamp_row(cur, -1, B);
        for (int64_t g = first; g <= last; ++g) ptr[g] = (int32_t)i;
    }
    if (bad) *flag = 1;
}

// ---- pooling, forward ------------------------------------------------------------------------------------------------
template <int VEC, int MODE>
struct Acc {
    float v[VEC];
    int32_t arg[VEC];
    __device__ __forceinline__ void init(int64_t lo) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            v[q] = MODE == ro::kMax ? -INFINITY : 0.0f;
            arg[q] = (int32_t)lo;
        }
    }
    __device__ __forceinline__ void take(const float (&x)[VEC], int64_t row) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            if (MODE == ro::kMax) {
                if (x[q] > v[q]) {
                    v[q] = x[q];
                    arg[q] = (int32_t)row;
                }
            } else {
                v[q] = v[q] + x[q];
            }
        }
    }
    // rows [r0, r1) of the column(s) at `col` in increasing order, kRoInFlight loads ahead of the adds
    __device__ __forceinline__ void rows(const float *__restrict__ col, int64_t F, int64_t r0, int64_t r1) {
        int64_t r = r0;
        for (; r + kRoInFlight <= r1; r += kRoInFlight) {
            float x[kRoInFlight][VEC];
#pragma unroll
            for (int u = 0; u < kRoInFlight; ++u) load_vec<float, VEC>(col + (r + u) * F, x[u]);
#pragma unroll
            for (int u = 0; u < kRoInFlight; ++u) take(x[u], r + u);
        }
        for (; r < r1; ++r) {
            float x[VEC];
            load_vec<float, VEC>(col + r * F, x);
            take(x, r);
        }
    }
    __device__ __forceinline__ void store(float *__restrict__ out, int32_t *__restrict__ argmax, int64_t at, int64_t n) {
        float o[VEC], a[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            o[q] = n == 0 ? 0.0f : (MODE == ro::kMean ? v[q] / (float)n : v[q]);
            a[q] = __int_as_float(n == 0 ? -1 : arg[q]);
        }
        store_vec<float, VEC>(out + at, o);
        if (MODE == ro::kMax) store_vec<float, VEC>(reinterpret_cast<float *>(argmax) + at, a);
    }
};

// C column slots of VEC floats per row; a group of G lanes (power of two) holds one (graph, tile of G slots) item.
template <int VEC, int MODE>
__global__ __launch_bounds__(kRoBlock) void segment_pool_kernel(const float *__restrict__ x, const int32_t *__restrict__ ptr,
                                                                int64_t N, int64_t B, int64_t F, int C, int G, int T,
                                                                float *__restrict__ out, int32_t *__restrict__ argmax) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t item = ((int64_t)blockIdx.x * kRoWaves + wave) * (kWave / G) + lane / G;
    const int64_t g = item / T;
    const int slot = (int)(item % T) * G + (lane & (G - 1));
    if (g >= B || slot >= C) return;
    const Seg s = segment_of(ptr, g, N);
    if (s.hi - s.lo > ro::kExactNodes) return;  // segment_pool_long_kernel's
    Acc<VEC, MODE> acc;
    acc.init(s.lo);
    acc.rows(x + (int64_t)slot * VEC, F, s.lo, s.hi);
    acc.store(out, argmax, g * F + (int64_t)slot * VEC, s.hi - s.lo);
}

// Segments above kExactNodes rows: one workgroup per (graph, tile of 64 slots), wave w is way w of the law.
template <int VEC, int MODE>
__global__ __launch_bounds__(kRoBlock) void segment_pool_long_kernel(const float *__restrict__ x, const int32_t *__restrict__ ptr,
                                                                     int64_t N, int64_t B, int64_t F, int C, int T,
                                                                     float *__restrict__ out, int32_t *__restrict__ argmax) {
    __shared__ float part_v[ro::kWays][kWave * VEC];
    __shared__ int32_t part_a[ro::kWays][kWave * VEC];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int64_t item = blockIdx.x; item < B * T; item += gridDim.x) {
        const int64_t g = item / T;
        const Seg s = segment_of(ptr, g, N);
        const int64_t n = s.hi - s.lo;
        if (n <= ro::kExactNodes) continue;  // (the same for the whole workgroup)
        const int slot = (int)(item % T) * kWave + lane;
        const bool active = slot < C;
        Acc<VEC, MODE> acc;
        acc.init(s.lo);
        if (active)
            for (int64_t c = wave; c * ro::kChunkRows < n; c += ro::kWays) {
                const int64_t r0 = s.lo + c * ro::kChunkRows;
                acc.rows(x + (int64_t)slot * VEC, F, r0, r0 + ro::kChunkRows < s.hi ? r0 + ro::kChunkRows : s.hi);
            }
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            part_v[wave][lane * VEC + q] = acc.v[q];
            part_a[wave][lane * VEC + q] = acc.arg[q];
        }
        __syncthreads();
        if (wave == 0 && active) {
#pragma unroll
            for (int q = 0; q < VEC; ++q)
                for (int w = 1; w < ro::kWays; ++w) {
                    const float v = part_v[w][lane * VEC + q];
                    const int32_t a = part_a[w][lane * VEC + q];
                    if (MODE == ro::kMax) {
                        if (ro::better(v, a, acc.v[q], acc.arg[q])) {
                            acc.v[q] = v;
                            acc.arg[q] = a;
                        }
                    } else {
                        acc.v[q] = acc.v[q] + v;
                    }
                }
            acc.store(out, argmax, g * F + (int64_t)slot * VEC, n);
        }
        __syncthreads();
    }
}

// ---- pooling, backward: a gather -------------------------------------------------------------------------------------
// The graph of row i: batch[i] where the caller has it, else the last g with ptr[g] <= i (bounded binary search).
__device__ __forceinline__ int64_t graph_of(const int32_t *__restrict__ ptr, const int64_t *__restrict__ batch, int64_t B,
                                            int64_t i) {
    if (batch) return batch[i];
    int64_t lo = 0, hi = B + 1;  // first j in [0, B] with ptr[j] > i
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)ptr[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

template <int VEC, int MODE>
__global__ __launch_bounds__(kRoBlock) void segment_pool_bwd_kernel(const float *__restrict__ grad, const int32_t *__restrict__ ptr,
                                                                    const int64_t *__restrict__ batch,
                                                                    const int32_t *__restrict__ argmax, int64_t N, int64_t B,
                                                                    int64_t F, int C, float *__restrict__ grad_x) {
    const int64_t total = N * C, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / C, at = (e % C) * VEC;
        const int64_t g = graph_of(ptr, batch, B, i);
        float o[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) o[q] = 0.0f;
        if (g >= 0 && g < B) {
            const Seg s = segment_of(ptr, g, N);
            if (s.hi > s.lo) {
                float gr[VEC];
                load_vec<float, VEC>(grad + g * F + at, gr);
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (MODE == ro::kSum) o[q] = gr[q];
                    else if (MODE == ro::kMean) o[q] = gr[q] / (float)(s.hi - s.lo);
                    else o[q] = (int64_t)argmax[g * F + at + q] == i ? gr[q] : 0.0f;
                }
            }
        }
        store_vec<float, VEC>(grad_x + i * F + at, o);
    }
}

// ---- sort-pool -------------------------------------------------------------------------------------------------------
// One workgroup per graph.  n <= kLdsNodes: the sort words are sorted in LDS (bitonic, padded to a power of two).  Above:
// the words go to the workspace and every row counts the words below its own -- its rank; O(n^2), correct at any size.
template <int VEC>
__global__ __launch_bounds__(kRoBlock) void sort_pool_kernel(const float *__restrict__ x, const int32_t *__restrict__ ptr, int64_t N,
                                                             int64_t F, int C, int64_t k, int64_t key_col, uint64_t *ws,
                                                             float *__restrict__ out, int32_t *idx) {
    __shared__ uint64_t w[ro::kLdsNodes];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const Seg s = segment_of(ptr, g, N);
    const int64_t n = s.hi - s.lo, kk = n < k ? n : k;
    int32_t *my_idx = idx + g * k;
    if (n <= ro::kLdsNodes) {
        int P = 1;
        while (P < n) P <<= 1;
        for (int t = tid; t < P; t += kRoBlock) w[t] = t < n ? ro::word(x[(s.lo + t) * F + key_col], t) : ro::kPadWord;
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int j = size >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P; t += kRoBlock) {
                    const int u = t ^ j;
                    if (u > t) {
                        const uint64_t a = w[t], b = w[u];
                        if ((a > b) == ((t & size) == 0)) {
                            w[t] = b;
                            w[u] = a;
                        }
                    }
                }
                __syncthreads();
            }
        for (int64_t j = tid; j < k; j += kRoBlock) my_idx[j] = j < kk ? (int32_t)(s.lo + (int64_t)(uint32_t)w[j]) : -1;
    } else {
        for (int64_t t = tid; t < n; t += kRoBlock) ws[s.lo + t] = ro::word(x[(s.lo + t) * F + key_col], t);
        for (int64_t j = kk + tid; j < k; j += kRoBlock) my_idx[j] = -1;
        __syncthreads();
        for (int64_t base = 0; base < n; base += kRoBlock) {  // (n is the same for the whole workgroup: the barriers are safe)
            const bool have = base + tid < n;
            const uint64_t mine = have ? ws[s.lo + base + tid] : 0;
            int64_t rank = 0;
            for (int64_t tile = 0; tile < n; tile += ro::kLdsNodes) {
                const int m = (int)(n - tile < ro::kLdsNodes ? n - tile : ro::kLdsNodes);
                for (int t = tid; t < m; t += kRoBlock) w[t] = ws[s.lo + tile + t];
                __syncthreads();
                for (int t = 0; t < m; ++t) rank += w[t] < mine ? 1 : 0;
                __syncthreads();
            }
            if (have && rank < kk) my_idx[rank] = (int32_t)(s.lo + base + tid);
        }
    }
    __syncthreads();  // my_idx was written by this workgroup: visible to it from here on
    for (int64_t e = tid; e < k * C; e += kRoBlock) {
        const int64_t j = e / C, at = (e % C) * VEC;
        const int64_t src = my_idx[j];
        float o[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) o[q] = 0.0f;
        if (src >= 0 && src < N) load_vec<float, VEC>(x + src * F + at, o);
        store_vec<float, VEC>(out + (g * k + j) * F + at, o);
    }
}

// grad_x was zeroed on the stream before; each node occurs at most once in idx, so plain stores do.
template <int VEC>
__global__ __launch_bounds__(kRoBlock) void sort_pool_bwd_kernel(const float *__restrict__ grad, const int32_t *__restrict__ idx,
                                                                 int64_t N, int64_t rows, int64_t F, int C,
                                                                 float *__restrict__ grad_x) {
    const int64_t total = rows * C, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int64_t j = e / C, at = (e % C) * VEC;
        const int64_t dst = idx[j];
        if (dst < 0 || dst >= N) continue;
        float o[VEC];
        load_vec<float, VEC>(grad + j * F + at, o);
        store_vec<float, VEC>(grad_x + dst * F + at, o);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static unsigned stride_grid(int64_t items) { return (unsigned)std::min<int64_t>((items + kRoBlock - 1) / kRoBlock, 8192); }

static bool vec4_ok(int64_t F, std::initializer_list<const void *> ps) {
    if (F % 4 != 0) return false;
    for (const void *p : ps)
        if (p && !aligned_to(p, 16)) return false;
    return true;
}

template <int VEC, int MODE>
static int pool_fwd_launch(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, float *out, int32_t *argmax,
                           hipStream_t s) {
    const int C = (int)(F / VEC);
    int G = 1;
    while (G < C && G < kWave) G <<= 1;
    const int T = (C + G - 1) / G;
    const int64_t waves = (B * T + kWave / G - 1) / (kWave / G);
    hipLaunchKernelGGL((segment_pool_kernel<VEC, MODE>), dim3((unsigned)((waves + kRoWaves - 1) / kRoWaves)), dim3(kRoBlock), 0, s, x,
                       ptr, N, B, F, C, G, T, out, argmax);
    int st = launch_status();
    if (st != COGDL_HIP_OK || N <= ro::kExactNodes) return st;  // (no segment can be long)
    const int T64 = (C + kWave - 1) / kWave;
    hipLaunchKernelGGL((segment_pool_long_kernel<VEC, MODE>), dim3((unsigned)std::min<int64_t>(B * T64, 2048)), dim3(kRoBlock), 0, s,
                       x, ptr, N, B, F, C, T64, out, argmax);
    return launch_status();
}

template <int VEC>
static int pool_fwd_mode(int mode, const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, float *out, int32_t *argmax,
                         hipStream_t s) {
    if (mode == ro::kSum) return pool_fwd_launch<VEC, ro::kSum>(x, ptr, N, B, F, out, argmax, s);
    if (mode == ro::kMean) return pool_fwd_launch<VEC, ro::kMean>(x, ptr, N, B, F, out, argmax, s);
    return pool_fwd_launch<VEC, ro::kMax>(x, ptr, N, B, F, out, argmax, s);
}

template <int VEC>
static int pool_bwd_mode(int mode, const float *grad, const int32_t *ptr, const int64_t *batch, const int32_t *argmax, int64_t N,
                         int64_t B, int64_t F, float *grad_x, hipStream_t s) {
    const int C = (int)(F / VEC);
    const dim3 grid(stride_grid(N * C)), block(kRoBlock);
    if (mode == ro::kSum)
        hipLaunchKernelGGL((segment_pool_bwd_kernel<VEC, ro::kSum>), grid, block, 0, s, grad, ptr, batch, argmax, N, B, F, C, grad_x);
    else if (mode == ro::kMean)
        hipLaunchKernelGGL((segment_pool_bwd_kernel<VEC, ro::kMean>), grid, block, 0, s, grad, ptr, batch, argmax, N, B, F, C, grad_x);
    else
        hipLaunchKernelGGL((segment_pool_bwd_kernel<VEC, ro::kMax>), grid, block, 0, s, grad, ptr, batch, argmax, N, B, F, C, grad_x);
    return launch_status();
}

static int sizes_rc(int64_t N, int64_t B, int64_t F, int64_t k) {
    const int rc = ro::sizes_status(N, B, F, k);
    return rc == 0 ? COGDL_HIP_OK : (rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_segment_exact_nodes(void) { return ro::kExactNodes; }
extern "C" int cogdl_hip_sort_pool_lds_nodes(void) { return ro::kLdsNodes; }

extern "C" int cogdl_hip_segment_ptr(const int64_t *batch, int64_t N, int64_t B, int32_t *ptr, int *flag, void *stream) {
    const int rc = sizes_rc(N, B, 1, 1);
    if (rc) return rc;
    if (N == 0 || B == 0) return COGDL_HIP_OK;
    if (!batch || !ptr || !flag) return COGDL_HIP_EINVAL;
    if (!aligned_to(batch, 8) || !aligned_to(ptr, 4) || !aligned_to(flag, 4)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = fill_u32_async(flag, 0u, 1, s);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return COGDL_HIP_ELAUNCH;
    }
    hipLaunchKernelGGL(segment_ptr_kernel, dim3(stride_grid(N + 1)), dim3(kRoBlock), 0, s, batch, N, B, ptr, flag);
    return launch_status();
}

extern "C" int cogdl_hip_segment_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int mode, float *out,
                                          int32_t *argmax, void *stream) {
    const int rc = sizes_rc(N, B, F, 1);
    if (rc) return rc;
    if (mode < ro::kSum || mode > ro::kMax) return COGDL_HIP_EINVAL;
    if (N == 0 || B == 0) return COGDL_HIP_OK;  // (nothing to reduce: the caller's zeros stand)
    if (!x || !ptr || !out || (mode == ro::kMax && !argmax)) return COGDL_HIP_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(ptr, 4) || !aligned_to(out, 4) || !aligned_to(argmax, 4)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (vec4_ok(F, {x, out, argmax})) return pool_fwd_mode<4>(mode, x, ptr, N, B, F, out, argmax, s);
    return pool_fwd_mode<1>(mode, x, ptr, N, B, F, out, argmax, s);
}

extern "C" int cogdl_hip_segment_pool_bwd(const float *grad, const int32_t *ptr, const int64_t *batch, const int32_t *argmax,
                                          int64_t N, int64_t B, int64_t F, int mode, float *grad_x, void *stream) {
    const int rc = sizes_rc(N, B, F, 1);
    if (rc) return rc;
    if (mode < ro::kSum || mode > ro::kMax) return COGDL_HIP_EINVAL;
    if (N == 0) return COGDL_HIP_OK;
    if (!ptr || !grad_x || (B > 0 && !grad) || (mode == ro::kMax && !argmax)) return COGDL_HIP_EINVAL;
    if (!aligned_to(grad, 4) || !aligned_to(ptr, 4) || !aligned_to(batch, 8) || !aligned_to(argmax, 4) || !aligned_to(grad_x, 4))
        return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (vec4_ok(F, {grad, grad_x, argmax})) return pool_bwd_mode<4>(mode, grad, ptr, batch, argmax, N, B, F, grad_x, s);
    return pool_bwd_mode<1>(mode, grad, ptr, batch, argmax, N, B, F, grad_x, s);
}

extern "C" size_t cogdl_hip_sort_pool_workspace_bytes(int64_t N) {
    return N > ro::kLdsNodes ? (size_t)N * sizeof(uint64_t) : 0;  // (at or below the bound no graph leaves the LDS path)
}

extern "C" int cogdl_hip_sort_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int64_t k,
                                       int64_t key_col, float *out, int32_t *idx, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    const int rc = sizes_rc(N, B, F, k);
    if (rc) return rc;
    if (key_col < 0 || key_col >= F) return COGDL_HIP_EINVAL;
    if (B * k > 0x7fffffff) return COGDL_HIP_ERANGE;
    if (B == 0) return COGDL_HIP_OK;
    if (!ptr || !out || !idx || (N > 0 && !x)) return COGDL_HIP_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(ptr, 4) || !aligned_to(out, 4) || !aligned_to(idx, 4) || !aligned_to(workspace, 8))
        return COGDL_HIP_EALIGN;
    const size_t need = cogdl_hip_sort_pool_workspace_bytes(N);
    if (need > 0 && (!workspace || workspace_bytes < need)) return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (vec4_ok(F, {x, out}))
        hipLaunchKernelGGL((sort_pool_kernel<4>), dim3((unsigned)B), dim3(kRoBlock), 0, s, x, ptr, N, F, (int)(F / 4), k, key_col,
                           (uint64_t *)workspace, out, idx);
    else
        hipLaunchKernelGGL((sort_pool_kernel<1>), dim3((unsigned)B), dim3(kRoBlock), 0, s, x, ptr, N, F, (int)F, k, key_col,
                           (uint64_t *)workspace, out, idx);
    return launch_status();
}

extern "C" int cogdl_hip_sort_pool_bwd(const float *grad, const int32_t *idx, int64_t N, int64_t B, int64_t F, int64_t k,
                                       float *grad_x, void *stream) {
    const int rc = sizes_rc(N, B, F, k);
    if (rc) return rc;
    if (B * k > 0x7fffffff) return COGDL_HIP_ERANGE;
    if (N == 0) return COGDL_HIP_OK;
    if (!grad_x || (B > 0 && (!grad || !idx))) return COGDL_HIP_EINVAL;
    if (!aligned_to(grad, 4) || !aligned_to(idx, 4) || !aligned_to(grad_x, 4)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = fill_u32_async(grad_x, 0u, (size_t)(N * F), s);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return COGDL_HIP_ELAUNCH;
    }
    if (B == 0) return COGDL_HIP_OK;
    if (vec4_ok(F, {grad, grad_x}))
        hipLaunchKernelGGL((sort_pool_bwd_kernel<4>), dim3(stride_grid(B * k * (F / 4))), dim3(kRoBlock), 0, s, grad, idx, N, B * k, F,
                           (int)(F / 4), grad_x);
    else
        hipLaunchKernelGGL((sort_pool_bwd_kernel<1>), dim3(stride_grid(B * k * F)), dim3(kRoBlock), 0, s, grad, idx, N, B * k, F,
                           (int)F, grad_x);
    return launch_status();
}
