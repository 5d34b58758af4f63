// recon.hip -- the inner-product decoder loss of a graph auto-encoder and its gradient, without an [N, N] matrix:
//     loss = SUM_ij softplus(<z_i, z_j>) - SUM_e w_e <z_row[e], z_col[e]>                       z [N, d] fp32, edges int32 [E]
//     gZ_i = 2 g SUM_j sigmoid(<z_i, z_j>) z_j - g SUM_{e: row[e] = i} w_e z_col[e] - g SUM_{e: col[e] = i} w_e z_row[e]
// which is binary_cross_entropy(sigmoid(Z Z^T), A, reduction="sum") for A = the dense sum of the weighted edges, log(1 - sigmoid)
// not clamped (VGAE.make_loss, cogdl/models/nn/gae.py:76-84; DAEGC.recon_loss, cogdl/models/nn/daegc.py:82-84;
// operators/recon.py).
//
// Dense term.  A workgroup of 256 threads OWNS tile I, 64 rows of z, staged in LDS for all of d (pairtile.h: stride DP + 2
// words, 64 x 64 scores from v_mfma_f32_32x32x2_f32, one 32 x 32 block per wave), and walks other tiles J of 64 rows:
//   forward   Z Z^T is symmetric, so only J >= I is walked: a tile with J > I counts twice, the diagonal tile once.  Slice s of
//             gridDim.y takes its share of the T - I tiles of its row tile.  On the accumulators softplus(s) = max(s, 0) +
//             log1p(exp(-|s|)), which never overflows; rows and columns at and beyond N count nothing.  A lane adds its 16 values
//             of a tile in float and the tile sums in double; the workgroup's double goes to part[I slices + s], and
//             recon_loss_fold_kernel adds all partials in index order.  Heavy row tiles (small I) have the small block ids and
//             start first.
//   backward  the owner walks ALL J (using the symmetry here would need atomics or [tiles, N, d] partials): scores by MFMA,
//             sigmoid in registers (the scores are recomputed: only z is kept), W to LDS as [owned row][other row] (stride 66)
//             and a second MFMA adds W[64 x 64] . Z_J[64 x d] into the owned rows' [64, d] accumulator: a wave holds 32 rows x
//             DP / 2 columns, 16 DP / 64 registers.  Slices over J write partial [N, d] blocks.
// Edge term.  forward: groups of G = 16 (d <= 64) or 64 lanes take one edge each, lanes across d, a wave takes a run of 256
// edges and writes one double.  backward: recon_grad_finish_kernel, one wave per row of gZ, lanes across d: folds the slices of
// the dense term in slice order, scales by 2 g, and gathers the row's edges from the row-sorted CSR and the column-sorted one
// (duplicates add up, a self loop is in both and so counts as the derivative of <z_i, z_i> does).  Nothing of size [E, d].
// No float atomics and every sum in a fixed order: equal results from run to run.  Every global read of z is checked against N
// and d in the tile loops; edge endpoints are the caller's to keep in [0, N) (operators/recon.py checks them before any launch).
#include "common.h"
#include "pairtile.h"

namespace cogdl {

constexpr int kRcWStride = kPlTile + 2;      // W tile: [owned row][other row]
constexpr int kRcWantGroups = 1024;          // workgroups a launch aims for: 4 per CU
constexpr int64_t kRcBudget = 64ll << 20;    // bytes of the backward's slice partials, at most (and an eighth of N x N floats)
constexpr int kRcMaxD = 256;
constexpr int kRcEdgeRun = 256;              // edges per wave and per partial of the forward's edge term

__device__ __forceinline__ double rc_wave_sum(double v) {
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, kWave);
    return v;
}

template <int DP>
__global__ __launch_bounds__(256) void recon_softplus_kernel(const float *__restrict__ z, int64_t N, int d, int vec,
                                                             double *__restrict__ part) {
    __shared__ float xs[kPlTile * (DP + 2)];
    __shared__ float ys[kPlTile * (DP + 2)];
    __shared__ double wsum[4];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31, oh = wave & 1, th = wave >> 1;
    const int dk = (d + 3) & ~3;
    const int64_t I = blockIdx.x, T = (N + kPlTile - 1) / kPlTile;
    const int64_t tps = (T - I + gridDim.y - 1) / gridDim.y;  // of the T - I tiles J >= I
    const int64_t t0 = I + (int64_t)blockIdx.y * tps, t1 = min(T, t0 + tps);
    pl_stage<DP>(z, I * kPlTile, N, d, dk, vec, xs);
    const bool own_live = I * kPlTile + 32 * oh + j < N;
    double acc = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();  // the previous tile's operand reads are done
        pl_stage<DP>(z, t * kPlTile, N, d, dk, vec, ys);
        __syncthreads();
        float s[16];
        pl_scores<DP>(xs, ys, dk, oh, th, j, half, s);
        const int64_t kb = t * kPlTile + 32 * th + 4 * half;
        float ts = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float sp = fmaxf(s[r], 0.0f) + log1pf(expf(-fabsf(s[r])));
            ts += (own_live && kb + (r & 3) + 8 * (r >> 2) < N) ? sp : 0.0f;
        }
        acc += (double)(t > I ? 2.0f * ts : ts);
    }
    acc = rc_wave_sum(acc);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[I * gridDim.y + blockIdx.y] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// part[wave run] = SUM_{e in the run} w_e <z_row[e], z_col[e]>: G lanes per edge, 64 / G edges of the run at a time
template <int G>
__global__ __launch_bounds__(256) void recon_edge_dot_kernel(const float *__restrict__ z, const int32_t *__restrict__ row,
                                                             const int32_t *__restrict__ col, const float *__restrict__ w,
                                                             int64_t E, int d, double *__restrict__ part) {
    const int lane = threadIdx.x & (kWave - 1), sub = lane / G, l = lane % G;
    const int64_t run = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t e0 = run * kRcEdgeRun, e1 = min(E, e0 + kRcEdgeRun);
    if (e0 >= E) return;  // (the whole wave)
    double acc = 0.0;
    for (int64_t eb = e0; eb < e1; eb += kWave / G) {
        const int64_t e = eb + sub;
        float dot = 0.0f;
        if (e < e1) {
            const float *zr = z + (int64_t)row[e] * d, *zc = z + (int64_t)col[e] * d;
            for (int c = l; c < d; c += G) dot += zr[c] * zc[c];
        }
        dot = group_sum<G>(dot);
        if (e < e1 && l == 0) acc += (double)((w != nullptr ? w[e] : 1.0f) * dot);
    }
    acc = rc_wave_sum(acc);
    if (lane == 0) part[run] = acc;
}

// loss = (the nd dense partials, in index order) - (the ne edge partials, in index order): thread t adds the t-th 256th of
// either list, thread 0 the 256 results
__global__ __launch_bounds__(256) void recon_loss_fold_kernel(const double *__restrict__ dpart, int64_t nd,
                                                              const double *__restrict__ epart, int64_t ne,
                                                              float *__restrict__ loss) {
    __shared__ double sd[256], se[256];
    const int t = threadIdx.x;
    auto chunk = [&](const double *p, int64_t n) {
        const int64_t per = (n + 255) / 256, a = t * per, b = min(n, a + per);
        double v = 0.0;
        for (int64_t i = a; i < b; ++i) v += p[i];
        return v;
    };
    sd[t] = chunk(dpart, nd);
    se[t] = chunk(epart, ne);
    __syncthreads();
    if (t == 0) {
        double D = 0.0, Ed = 0.0;
        for (int i = 0; i < 256; ++i) {
            D += sd[i];
            Ed += se[i];
        }
        *loss = (float)(D - Ed);
    }
}

// dst[owned rows] = SUM_{J in the slice} sigmoid(Z_I Z_J^T) Z_J, unscaled (recon_grad_finish_kernel has the 2 g)
template <int DP>
__global__ __launch_bounds__(256) void recon_sigmoid_grad_kernel(const float *__restrict__ z, int64_t N, int d,
                                                                 int64_t tiles_per_slice, int vec, float *__restrict__ out,
                                                                 float *__restrict__ part) {
    constexpr int S = DP + 2, NB = DP / 64;
    __shared__ float xs[kPlTile * S];
    __shared__ float ys[kPlTile * S];
    __shared__ float ws[kPlTile * kRcWStride];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31, oh = wave & 1, th = wave >> 1;
    const int dk = (d + 3) & ~3;
    const int64_t x0 = (int64_t)blockIdx.x * kPlTile;
    const int64_t T = (N + kPlTile - 1) / kPlTile;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_slice, t1 = min(T, t0 + tiles_per_slice);
    pl_stage<DP>(z, x0, N, d, dk, vec, xs);
    pl_f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
    const int xl = 32 * oh + j;  // the lane's owned row in the score block
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();  // the previous tile's reads of ys and ws are done
        pl_stage<DP>(z, t * kPlTile, N, d, dk, vec, ys);
        __syncthreads();
        float s[16];
        pl_scores<DP>(xs, ys, dk, oh, th, j, half, s);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int yl = 32 * th + 4 * half + (r & 3) + 8 * (r >> 2);
            const float e = expf(-fabsf(s[r])), inv = 1.0f / (1.0f + e);  // sigmoid(s) = 1 / (1 + e^-s) = e^s / (1 + e^s)
            ws[xl * kRcWStride + yl] = t * kPlTile + yl < N ? (s[r] >= 0.0f ? inv : e * inv) : 0.0f;
        }
        __syncthreads();
        // acc[32 oh .. + 32][th DP / 2 .. + DP / 2] += W[owned][other] . Z_J[other][column]
        const float *ap = ws + (32 * oh + j) * kRcWStride + 2 * half;  // A[i = j][k]
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
    float *dst = gridDim.y == 1 ? out : part + (int64_t)blockIdx.y * N * d;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int col = th * (DP / 2) + 32 * b + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = x0 + 32 * oh + 4 * half + (r & 3) + 8 * (r >> 2);
            if (row < N && col < d) dst[row * d + col] = acc[b][r];
        }
    }
}

// out[i] = 2 g (part[0][i] + part[1][i] + ...) - g (SUM_{e in row i of A} w_e z[col_e] + SUM_{e in row i of A^T} tw_e z[tcol_e]).
// One wave per row, a lane has columns lane, lane + 64, .. (d <= 256: four at the most).  part may be out itself (one slice).
__global__ __launch_bounds__(256) void recon_grad_finish_kernel(const float *__restrict__ z, const float *__restrict__ g,
                                                                const float *part, int64_t slices,
                                                                const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                                const float *__restrict__ w, const int32_t *__restrict__ tptr,
                                                                const int32_t *__restrict__ tcol, const float *__restrict__ tw,
                                                                int64_t N, int d, float *out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const float g1 = *g;
    float dense[4], edge[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + kWave * k;
        dense[k] = edge[k] = 0.0f;
        if (c < d) {
            float v = part[i * d + c];
            for (int64_t sl = 1; sl < slices; ++sl) v += part[(sl * N + i) * d + c];
            dense[k] = v;
        }
    }
    auto gather = [&](const int32_t *ptr, const int32_t *cols, const float *wts) {
        if (ptr == nullptr) return;
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const float *zr = z + (int64_t)cols[e] * d;
            const float wv = wts != nullptr ? wts[e] : 1.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = lane + kWave * k;
                if (c < d) edge[k] += wv * zr[c];
            }
        }
    };
    gather(rowptr, col, w);
    gather(tptr, tcol, tw);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + kWave * k;
        if (c < d) out[i * d + c] = (2.0f * g1) * dense[k] - g1 * edge[k];
    }
}

static int64_t rc_tiles(int64_t rows) { return (rows + kPlTile - 1) / kPlTile; }

// which: 0 forward (double partials, one per workgroup), 1 backward ([N, d] float partials per slice)
static int64_t rc_slices(int64_t N, int64_t d, int which) {
    const int64_t tiles = std::max<int64_t>(1, rc_tiles(N));
    int64_t slices = std::max<int64_t>(1, kRcWantGroups / tiles);
    if (which == 1) {
        const int64_t budget = std::min<int64_t>(kRcBudget, N * N / 2);  // an eighth of N x N floats
        slices = std::min<int64_t>(slices, std::max<int64_t>(1, budget / std::max<int64_t>(1, N * d * 4)));
    }
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slices, tiles), 65535));
}

// the slices that are launched when `slices` are asked for; the backward's are not empty (tiles_per_slice: what one walks)
static int64_t rc_effective(int64_t N, int64_t slices, int which, int64_t *tiles_per_slice) {
    const int64_t tiles = std::max<int64_t>(1, rc_tiles(N));
    slices = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slices, tiles), 65535));
    const int64_t tps = (tiles + slices - 1) / slices;
    if (tiles_per_slice) *tiles_per_slice = tps;
    return which == 0 ? slices : (tiles + tps - 1) / tps;
}

static int64_t rc_edge_runs(int64_t E) { return (E + kRcEdgeRun - 1) / kRcEdgeRun; }

static int rc_sizes_status(int64_t N, int64_t d, int64_t E) {
    if (N < 0 || d < 1 || E < 0 || (N == 0 && E > 0)) return COGDL_HIP_EINVAL;
    if (N >= 0x7fffffff || E >= 0x7fffffff) return COGDL_HIP_ERANGE;
    if (d > kRcMaxD) return COGDL_HIP_EUNSUPPORTED;
    return COGDL_HIP_OK;
}

static int rc_vec(const float *z, int64_t d) { return d % 4 == 0 && aligned_to(z, 16); }

}  // namespace cogdl

using namespace cogdl;

extern "C" int64_t cogdl_hip_recon_bce_slices(int64_t N, int64_t d, int which) {
    if (N < 1 || d < 1 || which < 0 || which > 1) return 1;
    return rc_slices(N, d, which);
}

extern "C" size_t cogdl_hip_recon_bce_workspace_bytes(int64_t N, int64_t d, int64_t E, int64_t slices, int which) {
    if (N < 0 || d < 1 || E < 0 || slices < 1 || which < 0 || which > 1) return 0;
    const int64_t eff = rc_effective(N, slices, which, nullptr);
    if (which == 0) return (size_t)(rc_tiles(N) * eff + rc_edge_runs(E)) * sizeof(double);
    return eff > 1 ? (size_t)eff * (size_t)N * (size_t)d * sizeof(float) : 0;
}

extern "C" int cogdl_hip_recon_bce_fwd(const float *z, const int32_t *row, const int32_t *col, const float *w, int64_t N,
                                       int64_t d, int64_t E, int64_t slices, float *loss, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    int status = rc_sizes_status(N, d, E);
    if (status != COGDL_HIP_OK) return status;
    if (slices < 1 || !loss || (N > 0 && !z) || (E > 0 && (!row || !col))) return COGDL_HIP_EINVAL;
    if (!aligned_to(z, 4) || !aligned_to(row, 4) || !aligned_to(col, 4) || !aligned_to(w, 4) || !aligned_to(loss, 4) ||
        !aligned_to(workspace, 8))
        return COGDL_HIP_EALIGN;
    if (workspace_bytes < cogdl_hip_recon_bce_workspace_bytes(N, d, E, slices, 0) || (N > 0 && !workspace))
        return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t tiles = rc_tiles(N), eff = rc_effective(N, slices, 0, nullptr), runs = rc_edge_runs(E);
    double *dpart = (double *)workspace, *epart = dpart + tiles * eff;
    if (N > 0) {
        const dim3 grid((unsigned)tiles, (unsigned)eff);
        const int vec = rc_vec(z, d);
        if (d <= 64)
            hipLaunchKernelGGL(recon_softplus_kernel<64>, grid, dim3(256), 0, s, z, N, (int)d, vec, dpart);
        else if (d <= 128)
            hipLaunchKernelGGL(recon_softplus_kernel<128>, grid, dim3(256), 0, s, z, N, (int)d, vec, dpart);
        else
            hipLaunchKernelGGL(recon_softplus_kernel<256>, grid, dim3(256), 0, s, z, N, (int)d, vec, dpart);
        status = launch_status();
        if (status != COGDL_HIP_OK) return status;
    }
    if (E > 0) {
        const dim3 grid((unsigned)((runs + 3) / 4));
        if (d <= 64)
            hipLaunchKernelGGL(recon_edge_dot_kernel<16>, grid, dim3(256), 0, s, z, row, col, w, E, (int)d, epart);
        else
            hipLaunchKernelGGL(recon_edge_dot_kernel<64>, grid, dim3(256), 0, s, z, row, col, w, E, (int)d, epart);
        status = launch_status();
        if (status != COGDL_HIP_OK) return status;
    }
    hipLaunchKernelGGL(recon_loss_fold_kernel, dim3(1), dim3(256), 0, s, dpart, tiles * eff, epart, runs, loss);
    return launch_status();
}

extern "C" int cogdl_hip_recon_bce_grad(const float *z, const float *g, const int32_t *rowptr, const int32_t *col, const float *w,
                                        const int32_t *tptr, const int32_t *tcol, const float *tw, int64_t N, int64_t d,
                                        int64_t slices, float *grad_z, void *workspace, size_t workspace_bytes, void *stream) {
    int status = rc_sizes_status(N, d, 0);
    if (status != COGDL_HIP_OK) return status;
    if (slices < 1) return COGDL_HIP_EINVAL;
    if (N == 0) return COGDL_HIP_OK;
    if (!z || !g || !grad_z || (rowptr && !col) || (tptr && !tcol)) return COGDL_HIP_EINVAL;
    if (!aligned_to(z, 4) || !aligned_to(g, 4) || !aligned_to(rowptr, 4) || !aligned_to(col, 4) || !aligned_to(w, 4) ||
        !aligned_to(tptr, 4) || !aligned_to(tcol, 4) || !aligned_to(tw, 4) || !aligned_to(grad_z, 4) || !aligned_to(workspace, 4))
        return COGDL_HIP_EALIGN;
    int64_t tps;
    const int64_t eff = rc_effective(N, slices, 1, &tps);
    if (eff > 1 && (!workspace || workspace_bytes < cogdl_hip_recon_bce_workspace_bytes(N, d, 0, slices, 1)))
        return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *part = (float *)workspace;
    const dim3 grid((unsigned)rc_tiles(N), (unsigned)eff);
    const int vec = rc_vec(z, d);
    if (d <= 64)
        hipLaunchKernelGGL(recon_sigmoid_grad_kernel<64>, grid, dim3(256), 0, s, z, N, (int)d, tps, vec, grad_z, part);
    else if (d <= 128)
        hipLaunchKernelGGL(recon_sigmoid_grad_kernel<128>, grid, dim3(256), 0, s, z, N, (int)d, tps, vec, grad_z, part);
    else
        hipLaunchKernelGGL(recon_sigmoid_grad_kernel<256>, grid, dim3(256), 0, s, z, N, (int)d, tps, vec, grad_z, part);
    status = launch_status();
    if (status != COGDL_HIP_OK) return status;
    hipLaunchKernelGGL(recon_grad_finish_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, z, g,
                       eff > 1 ? (const float *)part : (const float *)grad_z, eff, rowptr, col, w, tptr, tcol, tw, N, (int)d,
                       grad_z);
    return launch_status();
}
