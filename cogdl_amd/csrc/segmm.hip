// segmm.hip -- dense products whose reduction, or whose weight block, follows a ragged segmentation of the rows (fp32):
//     tn   out_p[g] = S[ptr[g] : ptr[g+1]]^T  X_p[ptr[g] : ptr[g+1]]        S [N, K], X_p [N, F_p], out_p [B, K, F_p], p < 3
//     nn   out[i]  (+)= X[i] W[g(i)]                                          X [N, P], W [B, P, Q], out [N, Q]
// ptr int64 [B + 1] in device memory, never read on the host; g(i) is the segment with ptr[g] <= i < ptr[g + 1].  Each is the
// other's backward (operators/segmm.py).  DiffPool's pooling layer is one tn launch with the panels (embed, A S, S).
//
// tn.  The reduction index is the row, so both operands are k-major as they lie in memory: for v_mfma_f32_32x32x2_f32 lane l
// supplies A[i = l % 32][k = l / 32] = S[r + l / 32][a0 + l % 32] and B[k = l / 32][n = l % 32] = X[r + l / 32][c0 + l % 32],
// consecutive words for consecutive lanes, and nothing is transposed on the way.  The column tiles (64 wide) of all panels form
// one list; a workgroup of 4 waves owns, for one slice of one segment, a 64-wide tile of S's columns and a GROUP of up to 4
// consecutive column tiles of that list, i.e. up to four 64 x 64 output tiles that share their left operand.  It walks its rows
// in chunks of 16: the S chunk [16][64] is staged once and serves every tile of the group, wave w stages column tile w
// [16][64] (a wave reads 256 consecutive bytes of one row; 4-byte loads only, so any 4-byte aligned operand is served and no
// 16-byte load is ever issued).  Two LDS buffers: the next chunk's global loads are issued into registers before the chunk's
// MFMAs (8 k-steps x up to 4 tiles per wave) and written to the other buffer after them, one barrier per chunk.  Row strides
// of 96 and 288 words put the two rows a k-step reads on different halves of the 64 banks.  LDS: 2 x 16 x (96 + 288) x 4 =
// 48 KiB.  Wave (oh, th) holds the 32 x 32 block (32 oh, 32 th) of each tile: 16 accumulators per tile.  Rows at and past the
// slice's end, columns at and past K or F_p are staged as zeros and never stored; an empty segment writes zeros.
// Long segments: `split` slices, the same number for every segment; slice s of a segment of n rows takes rows
// [n s / split, n (s + 1) / split) of it.  With split > 1 the tiles go to the workspace ([slice][panel][B, K, F_p]) and
// segment_matmul_fold_kernel adds them in slice order.  The automatic split (sg_auto_split) is a function of N, B and the tile
// counts: about 1024 workgroups, at least 64 rows per slice of an average segment, partials within 64 MiB.
//
// nn.  A workgroup of 4 waves takes 32 consecutive rows x 128 output columns (wave w columns 32 w ..).  It finds the segment of
// its first row by bisection over ptr and then makes one pass per non-empty segment that its rows touch: P in chunks of 32, the
// X block [32][32] (stride 33) and the W[g] tile [32][128] (stride 160) staged in LDS, A[i = row][k], B[k][n = column] from
// there.  A pass's accumulators are taken over only for the rows of its segment (a select, not a multiply by a 0 / 1 mask:
// another segment's infinities stay out).  Every output element belongs to one lane of one workgroup, which adds to what is
// there when `accumulate` is set: no atomics.
// No float atomics, every sum in a fixed order: equal bytes from run to run.  A malformed ptr gives wrong numbers, never an
// access outside the operands: segment bounds are clamped to [0, N], every global access is checked against N, B, K, F, P, Q.
#include "common.h"

namespace cogdl {

typedef float sg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSgTile = 64;                          // tn: edge of an output tile
constexpr int kSgChunk = 16;                         // tn: rows per staged chunk
constexpr int kSgGroup = 4;                          // tn: column tiles per workgroup
constexpr int kSgSS = kSgTile + 32;                  // tn: LDS row stride of the S chunk
constexpr int kSgXS = kSgGroup * kSgTile + 32;       // tn: LDS row stride of the panel chunk
constexpr int kSgWantGroups = 1024;                  // tn: workgroups a launch aims for
constexpr int kSgMinRows = 64;                       // tn: rows of an average segment a slice should keep
constexpr int64_t kSgBudget = 64ll << 20;            // tn: bytes of slice partials, at most
constexpr int kSgMaxSplit = 1024;
constexpr int kSnRows = 32, kSnCols = 128, kSnK = 32;  // nn: rows and columns of a workgroup, P per staged chunk
constexpr int kSnXS = kSnK + 1, kSnWS = kSnCols + 32;

struct SgPanels {
    const float *x[3];
    float *out[3];
    int f[3];
    int tile0[4];    // panel p's first column tile in the list of all panels' tiles; tile0[3]: how many there are
    int64_t off[4];  // panel p's [B, K, F_p] block inside one slice's partials, in floats; off[3]: floats per slice
};

// (selects between values, not indexing: a kernel argument indexed by a register would be copied to scratch)
template <typename T>
__device__ __forceinline__ T sg_pick(int p, T v0, T v1, T v2) { return p == 0 ? v0 : (p == 1 ? v1 : v2); }
#define SG_PICK(pn, member, p) sg_pick((p), (pn).member[0], (pn).member[1], (pn).member[2])
__device__ __forceinline__ int sg_panel_of(const SgPanels &pn, int vt) { return (vt >= pn.tile0[1]) + (vt >= pn.tile0[2]); }

__global__ __launch_bounds__(256) void segment_matmul_tn_kernel(const float *__restrict__ s, SgPanels pn,
                                                                const int64_t *__restrict__ ptr, int64_t N, int K, int split,
                                                                int ktiles, int cgroups, float *__restrict__ part) {
    __shared__ float ss[2][kSgChunk * kSgSS];
    __shared__ float xs[2][kSgChunk * kSgXS];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31, oh = wave & 1, th = wave >> 1;
    int64_t b = blockIdx.x;  // ((segment, slice), S column tile, column tile group), the last fastest
    const int cg = (int)(b % cgroups);
    b /= cgroups;
    const int a0 = (int)(b % ktiles) * kSgTile;
    b /= ktiles;
    const int sl = (int)(b % split);
    const int64_t g = b / split;
    const int64_t p0 = min(max(ptr[g], (int64_t)0), N), p1 = min(max(ptr[g + 1], p0), N), n = p1 - p0;
    const int64_t r0 = p0 + n * sl / split, r1 = p0 + n * (sl + 1) / split;
    const int nt = min(kSgGroup, pn.tile0[3] - cg * kSgGroup);  // column tiles of this group

    // what this thread stages: column a0 + lane of S for rows wave, wave + 4, ..; column `xc` of panel `xp` (tile `wave` of the
    // group) for all 16 rows
    const int sc = a0 + lane;
    const int vt = cg * kSgGroup + wave, xpn = sg_panel_of(pn, vt);
    const float *xp = SG_PICK(pn, x, xpn);
    const int xf = SG_PICK(pn, f, xpn), xc = (vt - SG_PICK(pn, tile0, xpn)) * kSgTile + lane;
    const bool x_live = wave < nt && xc < xf, s_live = sc < K;
    float sr[kSgChunk / 4], xr[kSgChunk];
    auto load = [&](int64_t base) {
#pragma unroll
        for (int i = 0; i < kSgChunk / 4; ++i) {
            const int64_t row = base + wave + 4 * i;
            sr[i] = (s_live && row < r1) ? s[row * K + sc] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kSgChunk; ++i) {
            const int64_t row = base + i;
            xr[i] = (x_live && row < r1) ? xp[row * xf + xc] : 0.0f;
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < kSgChunk / 4; ++i) ss[buf][(wave + 4 * i) * kSgSS + lane] = sr[i];
#pragma unroll
        for (int i = 0; i < kSgChunk; ++i) xs[buf][i * kSgXS + wave * kSgTile + lane] = xr[i];
    };

    sg_f32x16 acc[kSgGroup];
#pragma unroll
    for (int t = 0; t < kSgGroup; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const bool wave_live = a0 + 32 * oh < K;  // (a wave whose 32 columns of S lie past K has nothing to add)
    load(r0);
    store(0);
    __syncthreads();
    int buf = 0;
    for (int64_t r = r0; r < r1; r += kSgChunk) {
        const bool more = r + kSgChunk < r1;
        if (more) load(r + kSgChunk);  // in flight during the MFMAs below
        if (wave_live) {
            const float *ap = ss[buf] + half * kSgSS + 32 * oh + j;  // A[i = j][k = half]
            const float *bp = xs[buf] + half * kSgXS + 32 * th + j;  // B[k = half][n = j]
#pragma unroll
            for (int kk = 0; kk < kSgChunk; kk += 2) {
                const float av = ap[kk * kSgSS];
#pragma unroll
                for (int t = 0; t < kSgGroup; ++t)
                    if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[kk * kSgXS + t * kSgTile], acc[t], 0, 0, 0);
            }
        }
        if (more) store(buf ^ 1);  // (last read in the previous iteration, before its barrier)
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int t = 0; t < kSgGroup; ++t) {
        if (t >= nt) continue;
        const int ot = cg * kSgGroup + t, p = sg_panel_of(pn, ot);
        const int f = SG_PICK(pn, f, p), c = (ot - SG_PICK(pn, tile0, p)) * kSgTile + 32 * th + j;
        float *dst = split == 1 ? SG_PICK(pn, out, p) : part + (int64_t)sl * pn.off[3] + SG_PICK(pn, off, p);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a = a0 + 32 * oh + 4 * half + (r & 3) + 8 * (r >> 2);
            if (a < K && c < f) dst[(g * K + a) * f + c] = acc[t][r];
        }
    }
}

// out_p = part[slice 0] + part[slice 1] + .., element by element, in slice order
__global__ __launch_bounds__(256) void segment_matmul_fold_kernel(const float *__restrict__ part, SgPanels pn, int split) {
    const int64_t total = pn.off[3];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float v = part[i];
        for (int sl = 1; sl < split; ++sl) v += part[(int64_t)sl * total + i];
        const int p = (i >= pn.off[1]) + (i >= pn.off[2]);
        SG_PICK(pn, out, p)[i - SG_PICK(pn, off, p)] = v;
    }
}

__global__ __launch_bounds__(256) void segment_matmul_nn_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                const int64_t *__restrict__ ptr, int64_t N, int64_t B, int P, int Q,
                                                                int accumulate, float *out) {
    __shared__ float xs[kSnRows * kSnXS];
    __shared__ float ws[kSnK * kSnWS];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, half = lane >> 5, j = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * kSnRows, rend = min(N, row0 + kSnRows);
    const int q0 = blockIdx.y * kSnCols, qw = q0 + 32 * wave;
    int64_t lo = 0, hi = B;  // the last g in [0, B) with ptr[g] <= row0 (g = 0 where there is none)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid] <= row0) lo = mid; else hi = mid;
    }
    sg_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int64_t g = lo; g < B; ++g) {
        const int64_t gb = ptr[g];
        if (gb >= rend) break;
        const int64_t ra = max(gb, row0), rb = min(ptr[g + 1], rend);
        if (ra >= rb) continue;  // an empty segment, or one that ends before the block
        sg_f32x16 pass;
#pragma unroll
        for (int r = 0; r < 16; ++r) pass[r] = 0.0f;
        const float *wg = w + g * (int64_t)P * Q;
        for (int k0 = 0; k0 < P; k0 += kSnK) {
            __syncthreads();  // the previous chunk's operand reads are done
#pragma unroll
            for (int i = 0; i < kSnRows / 8; ++i) {  // X: 32 consecutive k of a row per half wave
                const int rr = (tid >> 5) + 8 * i, k = k0 + j;
                xs[rr * kSnXS + j] = (row0 + rr < rend && k < P) ? x[(row0 + rr) * P + k] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < kSnK / 2; ++i) {  // W[g]: 128 consecutive columns of a k per two waves
                const int kr = (tid >> 7) + 2 * i, c = tid & (kSnCols - 1);
                ws[kr * kSnWS + c] = (k0 + kr < P && q0 + c < Q) ? wg[(int64_t)(k0 + kr) * Q + q0 + c] : 0.0f;
            }
            __syncthreads();
            if (qw < Q) {
                const float *ap = xs + j * kSnXS + half;                // A[i = j][k = half]
                const float *bp = ws + half * kSnWS + 32 * wave + j;    // B[k = half][n = j]
#pragma unroll
                for (int kk = 0; kk < kSnK; kk += 2)
                    pass = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk * kSnWS], pass, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + 4 * half + (r & 3) + 8 * (r >> 2);
            if (row >= ra && row < rb) acc[r] = pass[r];
        }
    }
    const int col = qw + j;
    if (col < Q) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row0 + 4 * half + (r & 3) + 8 * (r >> 2);
            if (row < rend) {
                float *o = out + row * Q + col;
                *o = accumulate ? *o + acc[r] : acc[r];
            }
        }
    }
}

static int64_t sg_tiles(int64_t n) { return (n + kSgTile - 1) / kSgTile; }

// the slices of every segment when the caller names none: from N, B and the tile counts only
static int64_t sg_auto_split(int64_t N, int64_t B, int64_t ktiles, int64_t tiles) {
    if (B < 1 || N < 1) return 1;
    const int64_t groups = B * ktiles * ((tiles + kSgGroup - 1) / kSgGroup);
    int64_t split = std::max<int64_t>(1, kSgWantGroups / groups);
    split = std::min<int64_t>(split, std::max<int64_t>(1, N / B / kSgMinRows));
    const int64_t slice_bytes = B * ktiles * tiles * kSgTile * kSgTile * (int64_t)sizeof(float);
    split = std::min<int64_t>(split, std::max<int64_t>(1, kSgBudget / slice_bytes));
    return std::min<int64_t>(split, kSgMaxSplit);
}

struct SgShape {
    int64_t ktiles, tiles, split, total;
    int n_panels;
};

static int sg_shape(int64_t N, int64_t B, int64_t K, const int64_t (&F)[3], int64_t split, SgShape *sh) {
    if (N < 0 || B < 0 || K < 1 || F[0] < 1 || F[1] < 0 || F[2] < 0 || (F[1] == 0 && F[2] > 0) || split < 0) return COGDL_HIP_EINVAL;
    if (N >= 0x7fffffff || B >= 0x7fffffff || K >= 0x7fffffff || split > kSgMaxSplit) return COGDL_HIP_ERANGE;
    sh->n_panels = 1 + (F[1] > 0) + (F[2] > 0);
    sh->ktiles = sg_tiles(K);
    sh->tiles = sh->total = 0;
    for (int p = 0; p < 3; ++p) {
        if (F[p] >= 0x7fffffff) return COGDL_HIP_ERANGE;
        sh->tiles += sg_tiles(F[p]);
        sh->total += B * K * F[p];
    }
    sh->split = split > 0 ? split : sg_auto_split(N, B, sh->ktiles, sh->tiles);
    const int64_t groups = (sh->tiles + kSgGroup - 1) / kSgGroup;
    if (sh->ktiles * groups >= 0x7fffffff || B * sh->split * sh->ktiles * groups >= 0x7fffffff) return COGDL_HIP_ERANGE;
    return COGDL_HIP_OK;
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_segment_matmul_workspace_bytes(int64_t N, int64_t B, int64_t K, int64_t F0, int64_t F1, int64_t F2,
                                                           int64_t split) {
    SgShape sh;
    const int64_t F[3] = {F0, F1, F2};
    if (sg_shape(N, B, K, F, split, &sh) != COGDL_HIP_OK) return 0;
    return sh.split > 1 ? (size_t)sh.split * (size_t)sh.total * sizeof(float) : 0;
}

extern "C" int cogdl_hip_segment_matmul_tn(const float *s, const float *x0, const float *x1, const float *x2, const int64_t *ptr,
                                           int64_t N, int64_t B, int64_t K, int64_t F0, int64_t F1, int64_t F2, int64_t split,
                                           float *out0, float *out1, float *out2, void *workspace, size_t workspace_bytes,
                                           void *stream) {
    SgShape sh;
    const int64_t F[3] = {F0, F1, F2};
    const float *x[3] = {x0, x1, x2};
    float *out[3] = {out0, out1, out2};
    int status = sg_shape(N, B, K, F, split, &sh);
    if (status != COGDL_HIP_OK) return status;
    if (B == 0) return COGDL_HIP_OK;
    if (!ptr || (N > 0 && !s)) return COGDL_HIP_EINVAL;
    if (!aligned_to(s, 4) || !aligned_to(ptr, 8) || !aligned_to(workspace, 4)) return COGDL_HIP_EALIGN;
    SgPanels pn = {};
    int tile = 0;
    int64_t off = 0;
    for (int p = 0; p < 3; ++p) {
        pn.tile0[p] = tile;
        pn.off[p] = off;
        if (p >= sh.n_panels) continue;
        if (!out[p] || (N > 0 && !x[p])) return COGDL_HIP_EINVAL;
        if (!aligned_to(x[p], 4) || !aligned_to(out[p], 4)) return COGDL_HIP_EALIGN;
        pn.x[p] = x[p];
        pn.out[p] = out[p];
        pn.f[p] = (int)F[p];
        tile += (int)sg_tiles(F[p]);
        off += B * K * F[p];
    }
    pn.tile0[3] = tile;
    pn.off[3] = off;
    if (sh.split > 1 && (!workspace || workspace_bytes < (size_t)sh.split * (size_t)sh.total * sizeof(float)))
        return COGDL_HIP_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t groups = (sh.tiles + kSgGroup - 1) / kSgGroup;
    hipLaunchKernelGGL(segment_matmul_tn_kernel, dim3((unsigned)(B * sh.split * sh.ktiles * groups)), dim3(256), 0, st, s, pn, ptr,
                       N, (int)K, (int)sh.split, (int)sh.ktiles, (int)groups, (float *)workspace);
    status = launch_status();
    if (status != COGDL_HIP_OK || sh.split == 1) return status;
    const unsigned blocks = (unsigned)std::min<int64_t>((sh.total + 255) / 256, 4096);
    hipLaunchKernelGGL(segment_matmul_fold_kernel, dim3(blocks), dim3(256), 0, st, (const float *)workspace, pn, (int)sh.split);
    return launch_status();
}

extern "C" int cogdl_hip_segment_matmul_nn(const float *x, const float *w, const int64_t *ptr, int64_t N, int64_t B, int64_t P,
                                           int64_t Q, int accumulate, float *out, void *stream) {
    if (N < 0 || B < 0 || P < 1 || Q < 1) return COGDL_HIP_EINVAL;
    if (N >= 0x7fffffff || B >= 0x7fffffff || P >= 0x7fffffff || Q >= 0x7fffffff) return COGDL_HIP_ERANGE;
    if (N == 0) return COGDL_HIP_OK;
    if (!x || !out || !ptr || (B > 0 && !w)) return COGDL_HIP_EINVAL;
    if (!aligned_to(x, 4) || !aligned_to(w, 4) || !aligned_to(out, 4) || !aligned_to(ptr, 8)) return COGDL_HIP_EALIGN;
    const int64_t qblocks = (Q + kSnCols - 1) / kSnCols;
    if (qblocks > 65535) return COGDL_HIP_ERANGE;
    const dim3 grid((unsigned)((N + kSnRows - 1) / kSnRows), (unsigned)qblocks);
    hipLaunchKernelGGL(segment_matmul_nn_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, w, ptr, N, B, (int)P, (int)Q,
                       accumulate, out);
    return launch_status();
}
