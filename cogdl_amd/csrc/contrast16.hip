// contrast16.hip -- the pairwise log-sum-exp of contrast.hip and its two gradients on fp16 / bf16 operands:
//     lse[i]    = log SUM_{j != skip[i]} exp(<q[i], k[j]> / tau)                  q [M, d], k [N, d] 16-bit; lse, corr fp32 [M]
//     grad_q[i] = (g_i / tau) SUM_j p_ij k[j]      grad_k[j] = (1 / tau) SUM_i g_i p_ij q[i]      p_ij = exp(s_ij / tau - lse_i)
// on v_mfma_f32_32x32x16_{f16,bf16}: fp32 arithmetic on the rounded operands, every 16-bit result rounded once where it is stored.
// The split of the work is contrast.hip's: a workgroup of four waves OWNS 64 rows of one side, keeps them in LDS for all of d and
// walks a slice of the other side in tiles of 64; wave (oh, th) takes the 32 x 32 score block <owned 32 oh .. , other 32 th ..>,
// and in the C/D map a lane holds ONE owned row (lane & 31) and 16 rows of the other tile.  What is this file's own:
//   staging   rows sit in LDS as 16-bit [row][k], k zero-padded to dk = a multiple of 16, with a row stride of DP + 8 elements
//             (DP = 64, 128 or 256, the smallest that holds d).  A lane of the 32x32x16 MFMA supplies row lane & 31, k = 8 (lane
//             >> 5) .. + 8: one 16-byte LDS read, aligned because (DP + 8) * 2 is a multiple of 16, and free of bank conflicts
//             because consecutive rows start (DP / 2 + 4) mod 64 = 36 or 4 words apart: sixteen lanes' four words tile the 64
//             banks.  A thread carries DP / 32 vectors of 8 elements of the NEXT tile in registers while the current one is
//             computed (the loads are issued right after the barrier that publishes the current tile): 16-byte global loads where
//             d % 8 == 0 and both bases are 16-byte aligned, element loads otherwise; every read is checked against the row count
//             and d, rows and columns beyond them are zeros.
//   scores    one MFMA per 16 columns of d and 32 x 32 block, alternating between two accumulators.  A product of two 16-bit
//             values is exact in fp32: the forward is as accurate as contrast.hip on the same (rounded) inputs.
//   backward  W[owned 64][other 64] . Other[other 64][d] contracts over the other tile's ROWS: the B operand is 8 consecutive
//             other-rows of one column, the transpose of the staged tile.  Remedy: a transposed 16-bit copy yt[column][other row]
//             (stride 72), written from the staged tile while the scores are computed -- a thread reads the same 8 columns of two
//             neighbouring rows (2 x 16 bytes) and writes 8 packed words, 32 lanes to 32 consecutive words -- so the second
//             product reads A (W, [owned row][other row], stride 72) and B with one aligned 16-byte LDS read each.
//   W         is computed in fp32 and rounded to nearest even ONCE into the operand type, but never as p_ij g_i / tau: p_ij ~
//             1 / N is below fp16's normal range (2^-14) from 16384 keys on and g_i / tau ~ 1 / (M tau) far below it.
//             grad_q holds p_ij 2^14 (p <= 1: at most 2^14, and a row's largest entry is at least 2^14 / N) and multiplies the
//             fp32 accumulators of owned row i by (g_i / tau) 2^-14 at the end.  grad_k contracts over i, so the factor cannot
//             wait: it holds p_ij g_i 2^(14 - e) with ONE e per launch, the binary exponent of max |g_i| over the rows whose
//             lse is finite (|g_i| 2^-e < 1), found on the device by pair_lse16_scale_kernel (the host never reads g), and
//             multiplies by 2^(e - 14) / tau at the end.  Powers of two: the scaling itself is exact.  bf16 takes the same path.
//   outputs   one slice: the kernel's store rounds the fp32 accumulator to the operand type.  Several slices: fp32 partials,
//             added in slice order and rounded by pair_lse16_fold_kernel.  lse and corr are fp32, merged and finished exactly
//             as contrast.hip does (l16_merge / l16_finish restate pl_merge / pl_finish: that file stays as it is).
// No float atomics and every sum in a fixed order: equal results from run to run.  skip is only ever compared.  d <= 256.
#include "common.h"

namespace cogdl {

constexpr int kL16Tile = 64;                  // rows of either side per step
constexpr int kL16TS = kL16Tile + 8;          // stride of W [owned row][other row] and of yt [column][other row]
constexpr int kL16WExp = 14;                  // W is held times 2^14
constexpr int kL16MaxD = 256;
constexpr size_t kL16ScaleBytes = 256;        // the head of the backward's workspace: the exponent word of grad_k
constexpr float kL16Log2e = 1.44269504088896340736f;
#define L16_NEG_INF (-__builtin_inff())

typedef float l16_f32x16 __attribute__((ext_vector_type(16)));
typedef float l16_f32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct L16;
template <> struct L16<_Float16> {
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    typedef _Float16 vec4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ l16_f32x16 mfma(vec8 a, vec8 b, l16_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct L16<__bf16> {
    typedef __bf16 vec8 __attribute__((ext_vector_type(8)));
    typedef __bf16 vec4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ l16_f32x16 mfma(vec8 a, vec8 b, l16_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

// (m, l) <- (m, l) merged with (m2, l2): l counts exp2((s - m) c).  Nothing there is (-inf, 0) and is passed over.
__device__ __forceinline__ void l16_merge(float &m, float &l, float m2, float l2, float c) {
    if (m2 == L16_NEG_INF) return;
    if (m == L16_NEG_INF) {
        m = m2;
        l = l2;
    } else if (m2 > m) {
        l = l * exp2f((m - m2) * c) + l2;
        m = m2;
    } else {
        l = l + l2 * exp2f((m2 - m) * c);
    }
}

__device__ __forceinline__ void l16_finish(float m, float l, float tau, float c, float *lse, float *corr) {
    if (m == L16_NEG_INF) {  // an empty sum
        *lse = L16_NEG_INF;
        *corr = 0.0f;
        return;
    }
    const float v = m / tau + logf(l);
    *lse = v;
    *corr = log2f(l) + (m - v * tau) * c;  // against m' = lse tau, which the backward forms by the same product
}

// A tile of 64 rows x dk columns on its way from global memory to LDS: item i of a thread is the 8 columns lcol[i] .. + 8 of
// tile row lrow[i] (lcol < 0: no item; consecutive threads take consecutive vectors of a row).  The map does not depend on the
// tile, so it is worked out once.
template <typename T, int DP>
struct L16Stage {
    static constexpr int kItems = DP / 32, S = DP + 8;
    int lrow[kItems], lcol[kItems];
    uint4 r[kItems];

    __device__ __forceinline__ void init(int dk) {
        const int nvp = dk >> 3;
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const int idx = (int)threadIdx.x + 256 * i;
            lrow[i] = idx / nvp;
            lcol[i] = idx < kL16Tile * nvp ? 8 * (idx % nvp) : -1;
        }
    }
    __device__ __forceinline__ void load(const T *__restrict__ src, int64_t row0, int64_t rows, int d, int vec) {
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            r[i] = make_uint4(0u, 0u, 0u, 0u);
            const int64_t row = row0 + lrow[i];
            if (lcol[i] < 0 || row >= rows) continue;
            if (vec) {  // d % 8 == 0, 16-byte aligned rows
                if (lcol[i] < d) r[i] = *reinterpret_cast<const uint4 *>(src + row * d + lcol[i]);
            } else {
                union { uint4 u; T e[8]; } t;
                t.u = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (lcol[i] + e < d) t.e[e] = src[row * d + lcol[i] + e];
                r[i] = t.u;
            }
        }
    }
    __device__ __forceinline__ void store(T *dst) const {
#pragma unroll
        for (int i = 0; i < kItems; ++i)
            if (lcol[i] >= 0) *reinterpret_cast<uint4 *>(dst + lrow[i] * S + lcol[i]) = r[i];
    }
};

// The wave's 32 x 32 block of scores: register r = <owned row 32 oh + j, other row 32 th + 4 half + (r & 3) + 8 (r >> 2)>.
template <typename T, int DP>
__device__ __forceinline__ void l16_scores(const T *xs, const T *ys, int dk, int oh, int th, int j, int half, float (&s)[16]) {
    using vec8 = typename L16<T>::vec8;
    constexpr int S = DP + 8;
    l16_f32x16 a0, a1;
#pragma unroll
    for (int r = 0; r < 16; ++r) a0[r] = a1[r] = 0.0f;
    const T *ap = ys + (32 * th + j) * S + 8 * half;  // A[i = j][k = 8 half ..]: rows of the other tile
    const T *bp = xs + (32 * oh + j) * S + 8 * half;  // B[k = 8 half ..][n = j]: owned rows
    for (int kk = 0; kk < dk; kk += 32) {
        a0 = L16<T>::mfma(*reinterpret_cast<const vec8 *>(ap + kk), *reinterpret_cast<const vec8 *>(bp + kk), a0);
        if (kk + 16 < dk)
            a1 = L16<T>::mfma(*reinterpret_cast<const vec8 *>(ap + kk + 16), *reinterpret_cast<const vec8 *>(bp + kk + 16), a1);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = a0[r] + a1[r];
}

template <typename T, int DP>
__global__ __launch_bounds__(256) void pair_lse16_fwd_kernel(const T *__restrict__ q, const T *__restrict__ k,
                                                             const int32_t *__restrict__ skip, int64_t M, int64_t N, int d,
                                                             float tau, float c, int64_t tiles_per_slice, int vec,
                                                             float *__restrict__ lse, float *__restrict__ corr,
                                                             float *__restrict__ part) {
    constexpr int S = DP + 8;
    __shared__ __attribute__((aligned(16))) T xs[kL16Tile * S];
    __shared__ __attribute__((aligned(16))) T ys[kL16Tile * S];
    __shared__ float pm[4 * kL16Tile], pl[4 * kL16Tile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31, oh = wave & 1, th = wave >> 1;
    const int dk = (d + 15) & ~15;
    const int64_t q0 = (int64_t)blockIdx.x * kL16Tile;
    const int64_t n_tiles = (N + kL16Tile - 1) / kL16Tile;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_slice, t1 = min(n_tiles, t0 + tiles_per_slice);
    L16Stage<T, DP> st;
    st.init(dk);
    st.load(q, q0, M, d, vec);
    st.store(xs);
    st.load(k, t0 * kL16Tile, N, d, vec);
    const int64_t qi = q0 + 32 * oh + j;  // this lane's query
    const int64_t my_skip = (skip != nullptr && qi < M) ? (int64_t)skip[qi] : -1;
    float mx = L16_NEG_INF, l = 0.0f;
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();  // the previous tile's operand reads are done
        st.store(ys);
        __syncthreads();
        if (t + 1 < t1) st.load(k, (t + 1) * kL16Tile, N, d, vec);  // in flight while this tile is computed
        float s[16];
        l16_scores<T, DP>(xs, ys, dk, oh, th, j, half, s);
        const int64_t kb = t * kL16Tile + 32 * th + 4 * half;
        float tmax = L16_NEG_INF;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t kj = kb + (r & 3) + 8 * (r >> 2);
            s[r] = (kj < N && kj != my_skip) ? s[r] : L16_NEG_INF;
            tmax = fmaxf(tmax, s[r]);
        }
        if (tmax > mx) {
            l = mx == L16_NEG_INF ? 0.0f : l * exp2f((mx - tmax) * c);
            mx = tmax;
        }
        if (mx != L16_NEG_INF) {
#pragma unroll
            for (int r = 0; r < 16; ++r) l += exp2f((s[r] - mx) * c);  // (-inf: exp2 gives 0)
        }
    }
    pm[(2 * th + half) * kL16Tile + 32 * oh + j] = mx;
    pl[(2 * th + half) * kL16Tile + 32 * oh + j] = l;
    __syncthreads();
    if (threadIdx.x < kL16Tile) {
        float m = L16_NEG_INF, sum = 0.0f;
#pragma unroll
        for (int slot = 0; slot < 4; ++slot) l16_merge(m, sum, pm[slot * kL16Tile + threadIdx.x], pl[slot * kL16Tile + threadIdx.x], c);
        const int64_t i = q0 + threadIdx.x;
        if (i < M) {
            if (gridDim.y == 1) {
                l16_finish(m, sum, tau, c, lse + i, corr + i);
            } else {
                part[2 * ((int64_t)blockIdx.y * M + i)] = m;
                part[2 * ((int64_t)blockIdx.y * M + i) + 1] = sum;
            }
        }
    }
}

__global__ void pair_lse16_merge_kernel(const float *__restrict__ part, int64_t M, int64_t slices, float tau, float c,
                                        float *__restrict__ lse, float *__restrict__ corr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    float m = L16_NEG_INF, sum = 0.0f;
    for (int64_t sl = 0; sl < slices; ++sl) l16_merge(m, sum, part[2 * (sl * M + i)], part[2 * (sl * M + i) + 1], c);
    l16_finish(m, sum, tau, c, lse + i, corr + i);
}

// *e_out = the binary exponent e of max |g_i| over the rows with a finite lse (|g_i| < 2^e; 0 where that maximum is 0 or not
// finite: such a g scales itself).  One workgroup, no atomics: a maximum does not depend on the order it is taken in.
__global__ __launch_bounds__(1024) void pair_lse16_scale_kernel(const float *__restrict__ g, const float *__restrict__ lse,
                                                                int64_t M, int *__restrict__ e_out) {
    __shared__ float part[1024 / kWave];
    float m = 0.0f;
    for (int64_t i = threadIdx.x; i < M; i += 1024) {
        const float a = fabsf(g[i]);
        if (lse[i] != L16_NEG_INF && !(a <= m)) m = a;  // (a NaN gets through and stays)
    }
    for (int s = kWave / 2; s > 0; s >>= 1) {
        const float o = __shfl_xor(m, s, kWave);
        if (!(o <= m)) m = (m != m) ? m : o;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 1024 / kWave; ++w)
            if (!(part[w] <= m)) m = (m != m) ? m : part[w];
        int e = 0;
        if (m > 0.0f && m < __builtin_inff()) (void)frexpf(m, &e);
        *e_out = e;
    }
}

// OWNER_Q: the workgroup owns 64 queries, walks keys, out = grad_q [M, d]; else it owns 64 keys, walks queries, out = grad_k.
template <typename T, int DP, bool OWNER_Q>
__global__ __launch_bounds__(256, DP <= 128 ? 2 : 1) void pair_lse16_grad_kernel(const T *__restrict__ q, const T *__restrict__ k,
                                                              const int32_t *__restrict__ skip, const float *__restrict__ lse,
                                                              const float *__restrict__ corr, const float *__restrict__ g,
                                                              const int *__restrict__ g_exp, int64_t M, int64_t N, int d,
                                                              float tau, float c, int64_t tiles_per_slice, int vec,
                                                              T *__restrict__ out, float *__restrict__ part) {
    using vec8 = typename L16<T>::vec8;
    using vec4 = typename L16<T>::vec4;
    constexpr int S = DP + 8, NB = DP / 64;
    __shared__ __attribute__((aligned(16))) T xs[kL16Tile * S];
    __shared__ __attribute__((aligned(16))) T ys[kL16Tile * S];
    __shared__ __attribute__((aligned(16))) T yt[DP * kL16TS];        // [column][other row]
    __shared__ __attribute__((aligned(16))) T ws[kL16Tile * kL16TS];  // [owned row][other row]
    __shared__ float a_mp[kL16Tile], a_corr[kL16Tile], a_gs[kL16Tile];  // of the 64 queries in play: lse tau, corr, g's factor
    __shared__ int a_skip[kL16Tile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int half = lane >> 5, j = lane & 31, oh = wave & 1, th = wave >> 1;
    const int dk = (d + 15) & ~15;
    const T *x = OWNER_Q ? q : k, *y = OWNER_Q ? k : q;
    const int64_t rows_x = OWNER_Q ? M : N, rows_y = OWNER_Q ? N : M;
    const int64_t x0 = (int64_t)blockIdx.x * kL16Tile;
    const int64_t n_tiles = (rows_y + kL16Tile - 1) / kL16Tile;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per_slice, t1 = min(n_tiles, t0 + tiles_per_slice);
    const int e_g = OWNER_Q ? 0 : *g_exp;
    auto stage_queries = [&](int64_t base) {
        if (threadIdx.x < kL16Tile) {
            const int64_t i = base + threadIdx.x;
            const float mp = i < M ? lse[i] * tau : L16_NEG_INF;  // (-inf stays -inf: a row with an empty sum)
            const bool live = mp != L16_NEG_INF;                 // a row without a sum takes nothing of its g, whatever g holds
            a_mp[threadIdx.x] = mp;
            a_corr[threadIdx.x] = live ? corr[i] : 0.0f;
            // grad_q: W = p 2^14 and the row's accumulators take (g / tau) 2^-14 at the end; grad_k: W = p g 2^(14 - e)
            a_gs[threadIdx.x] = live ? (OWNER_Q ? ldexpf(g[i] / tau, -kL16WExp) : ldexpf(g[i], kL16WExp - e_g)) : 0.0f;
            a_skip[threadIdx.x] = (live && skip != nullptr) ? skip[i] : -1;
        }
    };
    L16Stage<T, DP> st;
    st.init(dk);
    st.load(x, x0, rows_x, d, vec);
    st.store(xs);
    st.load(y, t0 * kL16Tile, rows_y, d, vec);
    if (OWNER_Q) stage_queries(x0);
    l16_f32x16 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
    const int xl = 32 * oh + j;  // the lane's owned row in the score block
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();  // the previous tile's reads of ys, yt, ws and the query values are done
        st.store(ys);
        if (!OWNER_Q) stage_queries(t * kL16Tile);
        __syncthreads();
        if (t + 1 < t1) st.load(y, (t + 1) * kL16Tile, rows_y, d, vec);  // in flight while this tile is computed
        float s[16];
        l16_scores<T, DP>(xs, ys, dk, oh, th, j, half, s);
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {  // the four other-rows 32 th + 4 half + 8 rg .. + 4 of the lane: one 8-byte write
            l16_f32x4 w4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int yl = 32 * th + 4 * half + 8 * rg + e;
                const int ql = OWNER_Q ? xl : yl;
                const int64_t kj = OWNER_Q ? t * kL16Tile + yl : x0 + xl;
                const float mp = a_mp[ql];
                float w = 0.0f;
                if (mp != L16_NEG_INF && kj < N && kj != (int64_t)a_skip[ql])
                    w = exp2f((s[4 * rg + e] - mp) * c - a_corr[ql]) * (OWNER_Q ? (float)(1 << kL16WExp) : a_gs[ql]);
                w4[e] = w;
            }
            *reinterpret_cast<vec4 *>(ws + xl * kL16TS + 32 * th + 4 * half + 8 * rg) = __builtin_convertvector(w4, vec4);
        }
        {  // yt[column][other row] <- ys[other row][column]: rows 2 rp, 2 rp + 1, columns 8 v .. + 8 per step
            const int rp = threadIdx.x & 31;
            uint32_t *yt32 = reinterpret_cast<uint32_t *>(yt);
            for (int v = threadIdx.x >> 5; v < (dk >> 3); v += 8) {
                const uint4 ua = *reinterpret_cast<const uint4 *>(ys + (2 * rp) * S + 8 * v);
                const uint4 ub = *reinterpret_cast<const uint4 *>(ys + (2 * rp + 1) * S + 8 * v);
                const uint32_t a4[4] = {ua.x, ua.y, ua.z, ua.w}, b4[4] = {ub.x, ub.y, ub.z, ub.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    yt32[((8 * v + 2 * e) * kL16TS >> 1) + rp] = (a4[e] & 0xffffu) | (b4[e] << 16);
                    yt32[((8 * v + 2 * e + 1) * kL16TS >> 1) + rp] = (a4[e] >> 16) | (b4[e] & 0xffff0000u);
                }
            }
        }
        __syncthreads();
        // out[32 oh .. + 32][th DP / 2 .. + DP / 2] += W[owned][other] . Other[other][column]
        const T *ap = ws + (32 * oh + j) * kL16TS + 8 * half;           // A[i = j][k = 8 half ..]
        const T *bp = yt + (th * (DP / 2) + j) * kL16TS + 8 * half;     // B[k = 8 half ..][n = j]
#pragma unroll
        for (int kk = 0; kk < kL16Tile; kk += 16) {
            const vec8 av = *reinterpret_cast<const vec8 *>(ap + kk);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (th * (DP / 2) + 32 * b < d)  // (columns at and beyond dk are never staged; beyond d never stored)
                    acc[b] = L16<T>::mfma(av, *reinterpret_cast<const vec8 *>(bp + 32 * b * kL16TS + kk), acc[b]);
            }
        }
    }
    __syncthreads();  // (a_gs of the owned queries, also where no tile was walked)
    const float f_all = OWNER_Q ? 0.0f : ldexpf(1.0f / tau, e_g - kL16WExp);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int col = th * (DP / 2) + 32 * b + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = 32 * oh + 4 * half + (r & 3) + 8 * (r >> 2);
            const int64_t row = x0 + rl;
            if (row < rows_x && col < d) {
                const float v = acc[b][r] * (OWNER_Q ? a_gs[rl] : f_all);
                if (gridDim.y == 1)
                    out[row * d + col] = (T)v;
                else
                    part[((int64_t)blockIdx.y * rows_x + row) * d + col] = v;
            }
        }
    }
}

template <typename T>
__global__ void pair_lse16_fold_kernel(const float *__restrict__ part, int64_t total, int64_t slices, T *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float v = part[i];
    for (int64_t sl = 1; sl < slices; ++sl) v += part[sl * total + i];
    out[i] = (T)v;
}

static int64_t l16_tiles(int64_t rows) { return (rows + kL16Tile - 1) / kL16Tile; }

// the tiles one slice walks when `slices` are asked for, and the slices that are then not empty
static void l16_split(int64_t other_rows, int64_t slices, int64_t *tiles_per_slice, int64_t *eff) {
    const int64_t tiles = std::max<int64_t>(1, l16_tiles(other_rows));
    slices = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(slices, tiles), 65535));
    *tiles_per_slice = (tiles + slices - 1) / slices;
    *eff = (tiles + *tiles_per_slice - 1) / *tiles_per_slice;
}

static int l16_sizes_status(int64_t M, int64_t N, int64_t d, int dtype) {
    if (M < 0 || N < 1 || d < 1) return COGDL_HIP_EINVAL;
    if (M >= 0x7fffffff || N >= 0x7fffffff) return COGDL_HIP_ERANGE;
    if (d > kL16MaxD || (dtype != COGDL_HIP_F16 && dtype != COGDL_HIP_BF16)) return COGDL_HIP_EUNSUPPORTED;
    return COGDL_HIP_OK;
}

static int l16_vec(const void *q, const void *k, int64_t d) { return d % 8 == 0 && aligned_to(q, 16) && aligned_to(k, 16); }

template <typename T>
static int l16_fwd(const T *q, const T *k, const int32_t *skip, int64_t M, int64_t N, int d, float tau, int64_t tps, int64_t eff,
                   float *lse, float *corr, float *part, hipStream_t s) {
    const float c = kL16Log2e / tau;
    const int vec = l16_vec(q, k, d);
    const dim3 grid((unsigned)l16_tiles(M), (unsigned)eff);
    if (d <= 64)
        hipLaunchKernelGGL((pair_lse16_fwd_kernel<T, 64>), grid, dim3(256), 0, s, q, k, skip, M, N, d, tau, c, tps, vec, lse, corr, part);
    else if (d <= 128)
        hipLaunchKernelGGL((pair_lse16_fwd_kernel<T, 128>), grid, dim3(256), 0, s, q, k, skip, M, N, d, tau, c, tps, vec, lse, corr, part);
    else
        hipLaunchKernelGGL((pair_lse16_fwd_kernel<T, 256>), grid, dim3(256), 0, s, q, k, skip, M, N, d, tau, c, tps, vec, lse, corr, part);
    return launch_status();
}

template <typename T, bool OWNER_Q>
static int l16_grad(dim3 grid, hipStream_t s, const T *q, const T *k, const int32_t *skip, const float *lse, const float *corr,
                    const float *g, const int *g_exp, int64_t M, int64_t N, int d, float tau, int64_t tps, T *out, float *part,
                    int64_t eff) {
    const float c = kL16Log2e / tau;
    const int vec = l16_vec(q, k, d);
    if (d <= 64)
        hipLaunchKernelGGL((pair_lse16_grad_kernel<T, 64, OWNER_Q>), grid, dim3(256), 0, s, q, k, skip, lse, corr, g, g_exp, M, N, d, tau,
                           c, tps, vec, out, part);
    else if (d <= 128)
        hipLaunchKernelGGL((pair_lse16_grad_kernel<T, 128, OWNER_Q>), grid, dim3(256), 0, s, q, k, skip, lse, corr, g, g_exp, M, N, d, tau,
                           c, tps, vec, out, part);
    else
        hipLaunchKernelGGL((pair_lse16_grad_kernel<T, 256, OWNER_Q>), grid, dim3(256), 0, s, q, k, skip, lse, corr, g, g_exp, M, N, d, tau,
                           c, tps, vec, out, part);
    int status = launch_status();
    if (status != COGDL_HIP_OK || eff == 1) return status;
    const int64_t total = (OWNER_Q ? M : N) * d;
    hipLaunchKernelGGL(pair_lse16_fold_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, total, eff, out);
    return launch_status();
}

template <typename T>
static int l16_grad_passes(const T *q, const T *k, const int32_t *skip, const float *lse, const float *corr, const float *g, int64_t M,
                           int64_t N, int d, float tau, int64_t slices_q, int64_t slices_k, T *grad_q, T *grad_k, void *workspace,
                           size_t workspace_bytes, hipStream_t s) {
    int *g_exp = (int *)workspace;
    float *part = (float *)((char *)workspace + kL16ScaleBytes);
    for (int pass = 0; pass < 2; ++pass) {
        T *out = pass == 0 ? grad_q : grad_k;
        const int64_t owned = pass == 0 ? M : N, other = pass == 0 ? N : M;
        if (!out || owned == 0) continue;
        int64_t tps, eff;
        l16_split(other, pass == 0 ? slices_q : slices_k, &tps, &eff);
        if (workspace_bytes < cogdl_hip_pair_lse16_workspace_bytes(owned, other, d, eff)) return COGDL_HIP_EWORKSPACE;
        const dim3 grid((unsigned)l16_tiles(owned), (unsigned)eff);
        int status;
        if (pass == 0) {
            status = l16_grad<T, true>(grid, s, q, k, skip, lse, corr, g, g_exp, M, N, d, tau, tps, out, part, eff);
        } else {
            hipLaunchKernelGGL(pair_lse16_scale_kernel, dim3(1), dim3(1024), 0, s, g, lse, M, g_exp);
            status = launch_status();
            if (status != COGDL_HIP_OK) return status;
            status = l16_grad<T, false>(grid, s, q, k, skip, lse, corr, g, g_exp, M, N, d, tau, tps, out, part, eff);
        }
        if (status != COGDL_HIP_OK) return status;
    }
    return COGDL_HIP_OK;
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_pair_lse16_workspace_bytes(int64_t M, int64_t N, int64_t d, int64_t slices) {
    return kL16ScaleBytes + cogdl_hip_pair_lse_workspace_bytes(M, N, d, slices);
}

extern "C" int cogdl_hip_pair_lse16_fwd(const void *q, const void *k, int dtype, const int32_t *skip, int64_t M, int64_t N,
                                        int64_t d, float tau, int64_t slices, float *lse, float *corr, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    int status = l16_sizes_status(M, N, d, dtype);
    if (status != COGDL_HIP_OK) return status;
    if (!(tau > 0.0f) || slices < 1) return COGDL_HIP_EINVAL;
    if (M == 0) return COGDL_HIP_OK;
    if (!q || !k || !lse || !corr) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 2) || !aligned_to(k, 2) || !aligned_to(skip, 4) || !aligned_to(lse, 4) || !aligned_to(corr, 4) ||
        !aligned_to(workspace, 4))
        return COGDL_HIP_EALIGN;
    int64_t tps, eff;
    l16_split(N, slices, &tps, &eff);
    if (eff > 1 && (!workspace || workspace_bytes < cogdl_hip_pair_lse_workspace_bytes(M, N, 2, eff))) return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *part = (float *)workspace;
    status = dtype == COGDL_HIP_F16
                 ? l16_fwd<_Float16>((const _Float16 *)q, (const _Float16 *)k, skip, M, N, (int)d, tau, tps, eff, lse, corr, part, s)
                 : l16_fwd<__bf16>((const __bf16 *)q, (const __bf16 *)k, skip, M, N, (int)d, tau, tps, eff, lse, corr, part, s);
    if (status != COGDL_HIP_OK || eff == 1) return status;
    hipLaunchKernelGGL(pair_lse16_merge_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, part, M, eff, tau,
                       kL16Log2e / tau, lse, corr);
    return launch_status();
}

extern "C" int cogdl_hip_pair_lse16_grad(const void *q, const void *k, int dtype, const int32_t *skip, const float *lse,
                                         const float *corr, const float *g, int64_t M, int64_t N, int64_t d, float tau,
                                         int64_t slices_q, int64_t slices_k, void *grad_q, void *grad_k, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    int status = l16_sizes_status(M, N, d, dtype);
    if (status != COGDL_HIP_OK) return status;
    if (!(tau > 0.0f) || slices_q < 1 || slices_k < 1) return COGDL_HIP_EINVAL;
    if (M == 0 && !grad_k) return COGDL_HIP_OK;
    if (!q || !k || (M > 0 && (!lse || !corr || !g))) return COGDL_HIP_EINVAL;
    if (!aligned_to(q, 2) || !aligned_to(k, 2) || !aligned_to(skip, 4) || !aligned_to(lse, 4) || !aligned_to(corr, 4) ||
        !aligned_to(g, 4) || !aligned_to(grad_q, 2) || !aligned_to(grad_k, 2) || !aligned_to(workspace, 4))
        return COGDL_HIP_EALIGN;
    if (!workspace || workspace_bytes < kL16ScaleBytes) return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == COGDL_HIP_F16)
        return l16_grad_passes<_Float16>((const _Float16 *)q, (const _Float16 *)k, skip, lse, corr, g, M, N, (int)d, tau, slices_q,
                                         slices_k, (_Float16 *)grad_q, (_Float16 *)grad_k, workspace, workspace_bytes, s);
    return l16_grad_passes<__bf16>((const __bf16 *)q, (const __bf16 *)k, skip, lse, corr, g, M, N, (int)d, tau, slices_q, slices_k,
                                   (__bf16 *)grad_q, (__bf16 *)grad_k, workspace, workspace_bytes, s);
}
