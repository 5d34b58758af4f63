// contrast.hip -- the row-wise log-sum-exp of a dense pairwise score matrix and its two gradients, without a score matrix:
//     lse[i]    = log SUM_{j != skip[i]} exp(<q[i], k[j]> / tau)                  q [M, d], k [N, d], fp32
//     grad_q[i] = (g_i / tau) SUM_j p_ij k[j]      grad_k[j] = (1 / tau) SUM_i g_i p_ij q[i]      p_ij = exp(s_ij / tau - lse_i)
// (GRACE's contrastive loss: cogdl/wrappers/model_wrapper/node_classification/grace_mw.py:64-77; operators/contrast.py.)
//
// One tile loop serves the three passes.  A workgroup OWNS 64 rows of one side (queries for the forward and grad_q, keys for
// grad_k), keeps them in LDS for all of d, and walks a slice of the OTHER side in tiles of 64 rows, each staged for all of d:
//   scores   (pairtile.h, shared with recon.hip) v_mfma_f32_32x32x2_f32 with A = 32 rows of the other tile, B = 32 owned rows.  The four waves take the four 32 x 32
//            blocks of the 64 x 64 tile, so in the C/D map a lane owns ONE owned row (its column) and 16 rows of the other tile
//            in its registers.  Rows are [row][k] with a stride of DP + 2 words; a lane reads k = 4 g + 2 half and the next as
//            one 8-byte LDS read and feeds two MFMAs (a product is a sum over k: which k meets which step is free as long as A
//            and B agree), on two accumulators that are added at the end of the tile.
//   forward  the lane's running {max of the raw dots, sum of exp2((s - max) log2e / tau)} of its query: one exp2 to rescale, 16
//            to add, per tile.  Keys at and beyond N and the skipped key are -inf and add nothing; a lane that has seen nothing
//            stays (-inf, 0) and is passed over by every merge (exp2(-inf - -inf) is never formed).  The four partials of a
//            query (2 lane halves x 2 waves) are merged through LDS in slot order; slices write (max, sum) per (slice, query)
//            and pair_lse_merge_kernel merges them in slice order.  lse = max / tau + ln(sum).
//   backward w = exp2((s - m') log2e / tau - corr) g_i / tau per score, 0 at the skipped entry, beyond M and N, and where lse_i
//            is -inf; m' = lse_i tau and corr_i = log2(sum_i) + (max_i - m') log2e / tau is the [M] vector the forward leaves
//            next to lse: s - m' is a difference of raw dots (about 1e-7 absolute), where s / tau - lse loses 1e-5 at scores of
//            several hundred.  W goes to LDS as [owned row][other row] (stride 66) and a second MFMA adds
//            W[64 x 64] . Other[64 x d] into the owned rows' gradient: a wave holds 32 rows x DP / 2 columns, 16 DP / 64
//            accumulator registers.  Slices write partial gradients, pair_lse_fold_kernel adds them in slice order.
// No float atomics and every sum in a fixed order: equal results from run to run.  DP = 64, 128 or 256 is the smallest that holds
// d (d > 256: COGDL_HIP_EUNSUPPORTED); an odd end of d is zero columns.  Every global read is checked against M, N and d; skip
// is only ever compared.  16-byte global loads where d % 4 == 0 and both bases are 16-byte aligned, 4-byte loads otherwise.
#include "common.h"
#include "pairtile.h"

namespace cogdl {

constexpr int kPlWStride = kPlTile + 2;       // W tile: [owned row][other row]
constexpr int kPlWantGroups = 1024;           // workgroups a launch aims for: 4 per CU where one is resident (d > 128)
constexpr int64_t kPlBudget = 64ll << 20;     // bytes of slice partials, at most (and at most an eighth of M x N floats)
constexpr int kPlMaxD = 256;
constexpr float kPlLog2e = 1.44269504088896340736f;
#define PL_NEG_INF (-__builtin_inff())

// (m, l) <- (m, l) merged with (m2, l2): l counts exp2((s - m) c).  Nothing there is (-inf, 0) and is passed over.
__device__ __forceinline__ void pl_merge(float &m, float &l, float m2, float l2, float c) {
    if (m2 == PL_NEG_INF) return;
    if (m == PL_NEG_INF) {
        m = m2;
        l = l2;
    } else if (m2 > m) {
        l = l * exp2f((m - m2) * c) + l2;
        m = m2;
    } else {
        l = l + l2 * exp2f((m2 - m) * c);
    }
}

__device__ __forceinline__ void pl_finish(float m, float l, float tau, float c, float *lse, float *corr) {
    if (m == PL_NEG_INF) {  // an empty sum
        *lse = PL_NEG_INF;
        *corr = 0.0f;
        return;
    }
    const float v = m / tau + logf(l);
    *lse = v;
    *corr = log2f(l) + (m - v * tau) * c;  // against m' = lse tau, which the backward forms by the same product
}

template <int DP>
__global__ __launch_bounds__(256) void pair_lse_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                           const int32_t *__restrict__ skip, int64_t M, int64_t N, int d,
                                                           float tau, float c, int64_t tiles_per_slice, int vec,
                                                           float *__restrict__ lse, float *__restrict__ corr,
                                                           float *__restrict__ part) {
    __shared__ float xs[kPlTile * (DP + 2)];
    __shared__ float ys[kPlTile * (DP + 2)];
    __shared__ float pm[4 * kPlTile], pl[4 * kPlTile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31, oh = wave & 1, th = wave >> 1;
    const int dk = (d + 3) & ~3;
    const int64_t q0 = (int64_t)blockIdx.x * kPlTile;
    const int64_t n_tiles = (N + kPlTile - 1) / kPlTile;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_slice, t1 = min(n_tiles, t0 + tiles_per_slice);
    pl_stage<DP>(q, q0, M, d, dk, vec, xs);
    const int64_t qi = q0 + 32 * oh + j;  // this lane's query
    const int64_t my_skip = (skip != nullptr && qi < M) ? (int64_t)skip[qi] : -1;
    float mx = PL_NEG_INF, l = 0.0f;
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();  // the previous tile's operand reads are done
        pl_stage<DP>(k, t * kPlTile, N, d, dk, vec, ys);
        __syncthreads();
        float s[16];
        pl_scores<DP>(xs, ys, dk, oh, th, j, half, s);
        const int64_t kb = t * kPlTile + 32 * th + 4 * half;
        float tmax = PL_NEG_INF;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t kj = kb + (r & 3) + 8 * (r >> 2);
            s[r] = (kj < N && kj != my_skip) ? s[r] : PL_NEG_INF;
            tmax = fmaxf(tmax, s[r]);
        }
        if (tmax > mx) {
            l = mx == PL_NEG_INF ? 0.0f : l * exp2f((mx - tmax) * c);
            mx = tmax;
        }
        if (mx != PL_NEG_INF) {
#pragma unroll
            for (int r = 0; r < 16; ++r) l += exp2f((s[r] - mx) * c);  // (-inf: exp2 gives 0)
        }
    }
    pm[(2 * th + half) * kPlTile + 32 * oh + j] = mx;
    pl[(2 * th + half) * kPlTile + 32 * oh + j] = l;
    __syncthreads();
    if (threadIdx.x < kPlTile) {
        float m = PL_NEG_INF, sum = 0.0f;
#pragma unroll
        for (int slot = 0; slot < 4; ++slot) pl_merge(m, sum, pm[slot * kPlTile + threadIdx.x], pl[slot * kPlTile + threadIdx.x], c);
        const int64_t i = q0 + threadIdx.x;
        if (i < M) {
            if (gridDim.y == 1) {
                pl_finish(m, sum, tau, c, lse + i, corr + i);
            } else {
                part[2 * ((int64_t)blockIdx.y * M + i)] = m;
                part[2 * ((int64_t)blockIdx.y * M + i) + 1] = sum;
            }
        }
    }
}

__global__ void pair_lse_merge_kernel(const float *__restrict__ part, int64_t M, int64_t slices, float tau, float c,
                                      float *__restrict__ lse, float *__restrict__ corr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    float m = PL_NEG_INF, sum = 0.0f;
    for (int64_t sl = 0; sl < slices; ++sl) pl_merge(m, sum, part[2 * (sl * M + i)], part[2 * (sl * M + i) + 1], c);
    pl_finish(m, sum, tau, c, lse + i, corr + i);
}

// OWNER_Q: the workgroup owns 64 queries, walks keys, out = grad_q [M, d]; else it owns 64 keys, walks queries, out = grad_k.
template <int DP, bool OWNER_Q>
__global__ __launch_bounds__(256) void pair_lse_grad_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                            const int32_t *__restrict__ skip, const float *__restrict__ lse,
                                                            const float *__restrict__ corr, const float *__restrict__ g,
                                                            int64_t M, int64_t N, int d, float tau, float c,
                                                            int64_t tiles_per_slice, int vec, float *__restrict__ out,
                                                            float *__restrict__ part) {
    constexpr int S = DP + 2, NB = DP / 64;
    __shared__ float xs[kPlTile * S];
    __shared__ float ys[kPlTile * S];
    __shared__ float ws[kPlTile * kPlWStride];
    __shared__ float a_mp[kPlTile], a_corr[kPlTile], a_gs[kPlTile];  // of the 64 queries in play: lse tau, corr, g / tau
    __shared__ int a_skip[kPlTile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31, oh = wave & 1, th = wave >> 1;
    const int dk = (d + 3) & ~3;
    const float *x = OWNER_Q ? q : k, *y = OWNER_Q ? k : q;
    const int64_t rows_x = OWNER_Q ? M : N, rows_y = OWNER_Q ? N : M;
    const int64_t x0 = (int64_t)blockIdx.x * kPlTile;
    const int64_t n_tiles = (rows_y + kPlTile - 1) / kPlTile;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_slice, t1 = min(n_tiles, t0 + tiles_per_slice);
    auto stage_queries = [&](int64_t base) {
        if (threadIdx.x < kPlTile) {
            const int64_t i = base + threadIdx.x;
            const bool live = i < M;
            a_mp[threadIdx.x] = live ? lse[i] * tau : PL_NEG_INF;  // (-inf stays -inf: a row with an empty sum)
            a_corr[threadIdx.x] = live ? corr[i] : 0.0f;
            a_gs[threadIdx.x] = live ? g[i] / tau : 0.0f;
            a_skip[threadIdx.x] = (live && skip != nullptr) ? skip[i] : -1;
        }
    };
    pl_stage<DP>(x, x0, rows_x, d, dk, vec, xs);
    if (OWNER_Q) stage_queries(x0);
    pl_f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
    const int xl = 32 * oh + j;  // the lane's owned row in the score block
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();  // the previous tile's reads of ys, ws and the query values are done
        pl_stage<DP>(y, t * kPlTile, rows_y, d, dk, vec, ys);
        if (!OWNER_Q) stage_queries(t * kPlTile);
        __syncthreads();
        float s[16];
        pl_scores<DP>(xs, ys, dk, oh, th, j, half, s);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int yl = 32 * th + 4 * half + (r & 3) + 8 * (r >> 2);
            const int ql = OWNER_Q ? xl : yl;
            const int64_t kj = OWNER_Q ? t * kPlTile + yl : x0 + xl;
            const float mp = a_mp[ql];
            float w = 0.0f;
            if (mp != PL_NEG_INF && kj < N && kj != (int64_t)a_skip[ql]) w = exp2f((s[r] - mp) * c - a_corr[ql]) * a_gs[ql];
            ws[xl * kPlWStride + yl] = w;
        }
        __syncthreads();
        // out[32 oh .. + 32][th DP / 2 .. + DP / 2] += W[owned][other] . Other[other][column]
        const float *ap = ws + (32 * oh + j) * kPlWStride + 2 * half;  // A[i = j][k]
        const float *bp = ys + (2 * half) * S + th * (DP / 2) + j;     // B[k][n = j]
        for (int kk = 0; kk < kPlTile; kk += 4) {
            const float2 av = *reinterpret_cast<const float2 *>(ap + kk);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (th * (DP / 2) + 32 * b < d) {  // (columns at and beyond dk are never staged; beyond d never stored)
                    const float b0 = bp[kk * S + 32 * b], b1 = bp[(kk + 1) * S + 32 * b];
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0, acc[b], 0, 0, 0);
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1, acc[b], 0, 0, 0);
                }
            }
        }
    }
    float *dst = gridDim.y == 1 ? out : part + (int64_t)blockIdx.y * rows_x * d;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int col = th * (DP / 2) + 32 * b + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = x0 + 32 * oh + 4 * half + (r & 3) + 8 * (r >> 2);
            if (row < rows_x && col < d) dst[row * d + col] = acc[b][r];
        }
    }
}

__global__ void pair_lse_fold_kernel(const float *__restrict__ part, int64_t total, int64_t slices, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float v = part[i];
    for (int64_t sl = 1; sl < slices; ++sl) v += part[sl * total + i];
    out[i] = v;
}

static int64_t pl_tiles(int64_t rows) { return (rows + kPlTile - 1) / kPlTile; }

// which: 0 forward, 1 grad_q, 2 grad_k
static int64_t pl_slices(int64_t M, int64_t N, int64_t d, int which) {
    const int64_t owned = which == 2 ? N : M, other = which == 2 ? M : N;
    const int64_t want = std::max<int64_t>(1, kPlWantGroups / std::max<int64_t>(1, pl_tiles(owned)));
    const int64_t per_slice = owned * 4 * (which == 0 ? 2 : d);  // bytes of one slice's partials
    const int64_t budget = std::min<int64_t>(kPlBudget, M * N / 2);  // an eighth of M x N floats
    int64_t slices = std::min<int64_t>(want, std::max<int64_t>(1, budget / std::max<int64_t>(1, per_slice)));
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slices, pl_tiles(other)), 65535));
}

// the tiles one slice walks when `slices` are asked for, and the slices that are then not empty
static void pl_split(int64_t other_rows, int64_t slices, int64_t *tiles_per_slice, int64_t *eff) {
    const int64_t tiles = std::max<int64_t>(1, pl_tiles(other_rows));
    slices = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slices, tiles), 65535));
    *tiles_per_slice = (tiles + slices - 1) / slices;
    *eff = (tiles + *tiles_per_slice - 1) / *tiles_per_slice;
}

static int pl_sizes_status(int64_t M, int64_t N, int64_t d) {
    if (M < 0 || N < 1 || d < 1) return COGDL_HIP_EINVAL;
    if (M >= 0x7fffffff || N >= 0x7fffffff) return COGDL_HIP_ERANGE;
    if (d > kPlMaxD) return COGDL_HIP_EUNSUPPORTED;
    return COGDL_HIP_OK;
}

static int pl_vec(const float *q, const float *k, int64_t d) { return d % 4 == 0 && aligned_to(q, 16) && aligned_to(k, 16); }

template <bool OWNER_Q>
static void pl_launch_grad(dim3 grid, hipStream_t s, const float *q, const float *k, const int32_t *skip, const float *lse,
                           const float *corr, const float *g, int64_t M, int64_t N, int d, float tau, int64_t tps, float *out,
                           float *part) {
    const float c = kPlLog2e / tau;
    const int vec = pl_vec(q, k, d);
    if (d <= 64)
        hipLaunchKernelGGL((pair_lse_grad_kernel<64, OWNER_Q>), grid, dim3(256), 0, s, q, k, skip, lse, corr, g, M, N, d, tau, c,
                           tps, vec, out, part);
    else if (d <= 128)
        hipLaunchKernelGGL((pair_lse_grad_kernel<128, OWNER_Q>), grid, dim3(256), 0, s, q, k, skip, lse, corr, g, M, N, d, tau, c,
                           tps, vec, out, part);
    else
        hipLaunchKernelGGL((pair_lse_grad_kernel<256, OWNER_Q>), grid, dim3(256), 0, s, q, k, skip, lse, corr, g, M, N, d, tau, c,
                           tps, vec, out, part);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int64_t cogdl_hip_pair_lse_slices(int64_t M, int64_t N, int64_t d, int which) {
    if (M < 1 || N < 1 || d < 1 || which < 0 || which > 2) return 1;
    return pl_slices(M, N, d, which);
}

extern "C" size_t cogdl_hip_pair_lse_workspace_bytes(int64_t M, int64_t N, int64_t d, int64_t slices) {
    (void)N;
    if (M < 1 || d < 1 || slices <= 1) return 0;
    return (size_t)slices * (size_t)M * (size_t)std::max<int64_t>(d, 2) * sizeof(float);
}

extern "C" int cogdl_hip_pair_lse_fwd(const float *q, const float *k, const int32_t *skip, int64_t M, int64_t N, int64_t d,
                                      float tau, int64_t slices, float *lse, float *corr, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    int status = pl_sizes_status(M, N, d);
    if (status != COGDL_HIP_OK) return status;
    if (!(tau > 0.0f) || slices < 1) return COGDL_HIP_EINVAL;
    if (M == 0) return COGDL_HIP_OK;
    if (!q || !k || !lse || !corr) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 4) || !aligned_to(k, 4) || !aligned_to(skip, 4) || !aligned_to(lse, 4) || !aligned_to(corr, 4) ||
        !aligned_to(workspace, 4))
        return COGDL_HIP_EALIGN;
    int64_t tps, eff;
    pl_split(N, slices, &tps, &eff);
    if (eff > 1 && (!workspace || workspace_bytes < cogdl_hip_pair_lse_workspace_bytes(M, N, 2, eff))) return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const float c = kPlLog2e / tau;
    const int vec = pl_vec(q, k, d);
    const dim3 grid((unsigned)pl_tiles(M), (unsigned)eff);
    float *part = (float *)workspace;
    if (d <= 64)
        hipLaunchKernelGGL(pair_lse_fwd_kernel<64>, grid, dim3(256), 0, s, q, k, skip, M, N, (int)d, tau, c, tps, vec, lse, corr,
                           part);
    else if (d <= 128)
        hipLaunchKernelGGL(pair_lse_fwd_kernel<128>, grid, dim3(256), 0, s, q, k, skip, M, N, (int)d, tau, c, tps, vec, lse, corr,
                           part);
    else
        hipLaunchKernelGGL(pair_lse_fwd_kernel<256>, grid, dim3(256), 0, s, q, k, skip, M, N, (int)d, tau, c, tps, vec, lse, corr,
                           part);
    status = launch_status();
    if (status != COGDL_HIP_OK || eff == 1) return status;
    hipLaunchKernelGGL(pair_lse_merge_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, part, M, eff, tau, c, lse, corr);
    return launch_status();
}

extern "C" int cogdl_hip_pair_lse_grad(const float *q, const float *k, const int32_t *skip, const float *lse, const float *corr,
                                       const float *g, int64_t M, int64_t N, int64_t d, float tau, int64_t slices_q,
                                       int64_t slices_k, float *grad_q, float *grad_k, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    int status = pl_sizes_status(M, N, d);
    if (status != COGDL_HIP_OK) return status;
    if (!(tau > 0.0f) || slices_q < 1 || slices_k < 1) return COGDL_HIP_EINVAL;
    if (M == 0 && !grad_k) return COGDL_HIP_OK;
    if (!q || !k || (M > 0 && (!lse || !corr || !g))) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 4) || !aligned_to(k, 4) || !aligned_to(skip, 4) || !aligned_to(lse, 4) || !aligned_to(corr, 4) ||
        !aligned_to(g, 4) || !aligned_to(grad_q, 4) || !aligned_to(grad_k, 4) || !aligned_to(workspace, 4))
        return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    float *part = (float *)workspace;
    for (int pass = 0; pass < 2; ++pass) {
        float *out = pass == 0 ? grad_q : grad_k;
        const int64_t owned = pass == 0 ? M : N, other = pass == 0 ? N : M;
        if (!out || owned == 0) continue;
        int64_t tps, eff;
        pl_split(other, pass == 0 ? slices_q : slices_k, &tps, &eff);
        if (eff > 1 && (!workspace || workspace_bytes < cogdl_hip_pair_lse_workspace_bytes(owned, other, d, eff)))
            return COGDL_HIP_EWORKSPACE;
        const dim3 grid((unsigned)pl_tiles(owned), (unsigned)eff);
        if (pass == 0)
            pl_launch_grad<true>(grid, s, q, k, skip, lse, corr, g, M, N, (int)d, tau, tps, out, part);
        else
            pl_launch_grad<false>(grid, s, q, k, skip, lse, corr, g, M, N, (int)d, tau, tps, out, part);
        status = launch_status();
        if (status != COGDL_HIP_OK) return status;
        if (eff > 1) {
            const int64_t total = owned * d;
            hipLaunchKernelGGL(pair_lse_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, total, eff, out);
            status = launch_status();
            if (status != COGDL_HIP_OK) return status;
        }
    }
    return COGDL_HIP_OK;
}
