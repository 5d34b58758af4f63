// hin2vec.hip -- HIN2Vec's training rows and its score on the device (the reference builds the rows in interpreted Python,
// one list append per walk position, hop and negative, and scores a batch through two [B, N] x [N, d] one-hot products;
// cogdl/models/emb/hin2vec.py:14-117).  Slots, keys, draws, the order of every sum: hin2vec_law.h.
//
// Pair builder, three steps on the caller's stream:
//   hin_pairs_count_kernel   a workgroup of four waves takes a run of kHpRun walks, a wave one walk at a time.  The wave stages
//                            a tile of kHpTile positions plus `hop` of halo -- ids as int32, types as bytes -- in its LDS slice
//                            once (this is also where a walk is validated), then its lanes stride over the positions: the hop
//                            slots of a position share every load.  Live slots are counted per walk.
//   device_exclusive_sum     scan.h, over W + 1 counts: offsets[W] is the number of live slots.
//   hin_pairs_emit_kernel    the same staging; a wave numbers its live slots in slot order with one wave scan per 64 positions
//                            and a running carry, and the lane that owns a slot writes its 1 + negative rows.
// Scorer:
//   hin_score_kernel         one wave per sample, four per workgroup.  Lanes stride over groups of four terms (one 16-byte
//                            load per row where rows start on 16 bytes), f(Wr[r]) is computed in registers, the 64 partials
//                            are folded by the law's butterfly.  Nothing of size [B, d] exists.
//   hin_grad_chunk_kernel    grid (chunks, column blocks of 1024).  The occurrences of a table row come from an inverted index
//                            cut into chunks of 512; chunk_ptr[row] numbers a row's first chunk (every row has at least one),
//                            a workgroup finds its row by a uniform binary search.  A thread owns four columns and keeps four
//                            occurrences' loads in flight.  Chunk 0 of a row goes to the gradient row itself -- for a row of one
//                            chunk that is the result, zeros included, so no memset precedes the launch --, chunk c >= 1 to
//                            slot chunk_ptr[row] - row + c - 1 of the partials (at most occurrences / 512 slots in all).
//   hin_grad_fold_kernel     grid (rows, column blocks): a row of several chunks adds them in ascending chunk order.  With tens
//                            of relations and thousands of samples every Wr row is such a row: its chunks run on as many
//                            workgroups as there are, not on one.
// No atomics, no packed fp32: results are equal from run to run.  Every global read is bounds-checked.
#include "common.h"
#include "hin2vec_law.h"
#include "scan.h"

namespace cogdl {
namespace hv = cogdl_hin2vec;

constexpr int kHpThreads = 256;
constexpr int kHpWaves = kHpThreads / kWave;
constexpr int kHpRun = 64;      // walks per workgroup
constexpr int kHpTile = 1024;   // positions a wave stages at a time (plus hop of halo)
constexpr int kHpStage = kHpTile + hv::kMaxHop;

struct HpStage {
    int32_t id[kHpWaves][kHpStage];
    int8_t type[kHpWaves][kHpStage];
};

// positions [p0, p0 + n) of one walk into the wave's slice; returns the flags this lane met
__device__ __forceinline__ int hp_stage(HpStage &st, int wave, int lane, const int64_t *__restrict__ row, int64_t p0, int n,
                                        int64_t L, const int32_t *__restrict__ node_type, int64_t N) {
    int err = 0;
    for (int q = lane; q < n; q += kWave) {
        const int64_t p = p0 + q;
        const int64_t v = row[p], next = p + 1 < L ? row[p + 1] : -1;
        int32_t id, type;
        hv::stage(v, next, node_type, N, id, type, err);
        st.id[wave][q] = id;
        st.type[wave][q] = (int8_t)type;
    }
    return err;
}

__global__ __launch_bounds__(kHpThreads) void hin_pairs_count_kernel(const int64_t *__restrict__ walks, int64_t W, int64_t L,
                                                                     int hop, const int32_t *__restrict__ node_type, int64_t N,
                                                                     int64_t *__restrict__ counts, int *__restrict__ flags) {
    __shared__ HpStage st;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * kHpRun;
    const int64_t positions = L - hop;
    int err = 0;
    for (int64_t w = w0 + wave; w - wave < w0 + kHpRun && w - wave < W; w += kHpWaves) {  // (workgroup-uniform trip count)
        const bool active = w < W;
        const int64_t *row = walks + (active ? w : 0) * L;
        int32_t live = 0;
        for (int64_t p0 = 0; p0 < positions; p0 += kHpTile) {
            const int tile = (int)(positions - p0 < kHpTile ? positions - p0 : kHpTile);
            if (active) err |= hp_stage(st, wave, lane, row, p0, tile + hop, L, node_type, N);
            __syncthreads();  // a lane reads what its neighbours staged
            const int32_t *ids = st.id[wave];
            for (int q = lane; active && q < tile; q += kWave)
                for (int j = 1; j <= hop; ++j) live += hv::slot_live([ids](int64_t p) { return ids[p]; }, q, j, hop) ? 1 : 0;
            __syncthreads();  // ... before the next tile overwrites it
        }
#pragma unroll
        for (int off = kWave / 2; off >= 1; off >>= 1) live += __shfl_xor(live, off, kWave);
        if (active && lane == 0) counts[w] = live;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[W] = 0;
    raise_flags(flags, err);
}

__global__ __launch_bounds__(kHpThreads) void hin_pairs_emit_kernel(const int64_t *__restrict__ walks, int64_t W, int64_t L, int hop,
                                                                    int64_t negative, const int32_t *__restrict__ node_type,
                                                                    hv::TypeTables tb, uint64_t seed,
                                                                    const int64_t *__restrict__ offsets, int64_t total,
                                                                    int64_t *__restrict__ out_x, int64_t *__restrict__ out_y,
                                                                    int64_t *__restrict__ out_key, int64_t *__restrict__ out_label,
                                                                    int *__restrict__ flags) {
    __shared__ HpStage st;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * kHpRun;
    const int64_t positions = L - hop, per = negative + 1;
    int err = 0;
    for (int64_t w = w0 + wave; w - wave < w0 + kHpRun && w - wave < W; w += kHpWaves) {  // (workgroup-uniform trip count)
        const bool active = w < W;
        const int64_t *row = walks + (active ? w : 0) * L;
        int64_t base = active ? offsets[w] : 0;  // the walk's first live slot; advanced by the carry of every 64 positions
        for (int64_t p0 = 0; p0 < positions; p0 += kHpTile) {
            const int tile = (int)(positions - p0 < kHpTile ? positions - p0 : kHpTile);
            if (active) (void)hp_stage(st, wave, lane, row, p0, tile + hop, L, node_type, tb.N);  // (the count kernel raised these)
            __syncthreads();
            const int32_t *ids = st.id[wave];
            const int8_t *types = st.type[wave];
            for (int q0 = 0; active && q0 < tile; q0 += kWave) {  // (wave-uniform trip count: all lanes execute the scan)
                const int q = q0 + lane;
                uint32_t mask = 0;
                if (q < tile)
                    for (int j = 1; j <= hop; ++j)
                        mask |= hv::slot_live([ids](int64_t p) { return ids[p]; }, q, j, hop) ? 1u << j : 0u;
                const int32_t mine = __popc(mask);
                const int32_t incl = wave_inclusive(mine, lane, ScanPlus());
                int64_t slot = base + (incl - mine);
                base += __shfl(incl, kWave - 1, kWave);
                for (int j = 1; j <= hop; ++j) {
                    if (!(mask & (1u << j))) continue;
                    if (slot >= 0 && slot < total) {
                        const int32_t x = ids[q], y = ids[q + j];
                        const int64_t key = hv::slot_key([types](int64_t p) { return (int32_t)types[p]; }, q, j);
                        const int64_t at = slot * per;
                        out_x[at] = x, out_y[at] = y, out_key[at] = key, out_label[at] = 1;
                        const uint64_t s = hv::slot_number(w, p0 + q, j, L, hop);
                        for (int64_t n = 0; n < negative; ++n) {
                            int64_t nx, ny;
                            hv::negative_row(tb, seed, s, n, x, y, types[q], types[q + j], nx, ny, err);
                            out_x[at + 1 + n] = nx, out_y[at + 1 + n] = ny, out_key[at + 1 + n] = key, out_label[at + 1 + n] = 0;
                        }
                    }
                    ++slot;
                }
            }
            __syncthreads();
        }
    }
    raise_flags(flags, err);
}

// ---------------------------------------------------------------- the scorer
constexpr int kHsThreads = 256;
constexpr int kHsWaves = kHsThreads / kWave;
constexpr int kHsInFlight = 4;                 // occurrences a gradient thread loads before it folds them
constexpr int kHsBlockCols = kHsThreads * 4;   // columns per workgroup of the gradient kernels

template <bool VEC>
__device__ __forceinline__ void hs_load4(const float *__restrict__ row, int64_t k, int64_t limit, float (&v)[4]) {
    if constexpr (VEC) {
        const float4 t = *reinterpret_cast<const float4 *>(row + k);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = k + c < limit ? row[k + c] : 0.0f;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kHsThreads) void hin_score_kernel(const float *__restrict__ Wx, const float *__restrict__ Wr,
                                                               const int32_t *__restrict__ x, const int32_t *__restrict__ y,
                                                               const int32_t *__restrict__ r, int64_t B, int64_t N, int64_t R,
                                                               int64_t D, float *__restrict__ p) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * kHsWaves + wave;  // wave-uniform
    if (b >= B) return;
    const int64_t xb = x[b], yb = y[b], rb = r[b];
    if (xb < 0 || xb >= N || yb < 0 || yb >= N || rb < 0 || rb >= R) {
        if (lane == 0) p[b] = __builtin_nanf("");
        return;
    }
    const float *rx = Wx + xb * D, *ry = Wx + yb * D, *rr = Wr + rb * D;
    const int64_t groups = (D + 3) >> 2;
    float acc = 0.0f;
    for (int64_t g = lane; g < groups; g += kWave) {
        float a[4], c[4], w[4];
        hs_load4<VEC>(rx, 4 * g, D, a);
        hs_load4<VEC>(ry, 4 * g, D, c);
        hs_load4<VEC>(rr, 4 * g, D, w);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (VEC || 4 * g + k < D) acc = hv::term_step(acc, a[k], c[k], w[k]);
    }
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, kWave);
    if (lane == 0) p[b] = hv::sigmoid_of(acc);
}

// the column a thread owns as its c-th (kgscore.hip's ownership: four consecutive ones for 16-byte rows, else strided)
template <bool VEC>
__device__ __forceinline__ int64_t hs_col(int64_t block0, int c) {
    return VEC ? block0 + 4 * (int64_t)threadIdx.x + c : block0 + (int64_t)threadIdx.x + (int64_t)kHsThreads * c;
}

template <bool VEC>
__device__ __forceinline__ void hs_load_cols(const float *__restrict__ row, int64_t block0, int64_t D, float (&v)[4]) {
    if constexpr (VEC) {
        const int64_t k = hs_col<true>(block0, 0);
        if (k < D) hs_load4<true>(row, k, D, v);
        else v[0] = v[1] = v[2] = v[3] = 0.0f;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t k = hs_col<false>(block0, c);
            v[c] = k < D ? row[k] : 0.0f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void hs_put_cols(float *__restrict__ row, int64_t block0, int64_t D, const float (&v)[4]) {
    if constexpr (VEC) {
        const int64_t k = hs_col<true>(block0, 0);
        if (k < D) *reinterpret_cast<float4 *>(row + k) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t k = hs_col<false>(block0, c);
            if (k < D) row[k] = v[c];
        }
    }
}

// What both gradient kernels are given.  rows = N (RELATION false: occurrences are the 2 B positions x then y) or R (true:
// the B positions of r).
struct HsGrad {
    const float *Wx, *Wr;
    const int32_t *x, *y, *r;
    const float *p, *grad_p;
    const int32_t *occ_ptr, *occ_pos, *chunk_ptr;
    int64_t B, N, R, D, rows, n_occ, n_slots;
    float *grad, *partials;
};

template <bool RELATION, bool VEC>
__global__ __launch_bounds__(kHsThreads) void hin_grad_chunk_kernel(HsGrad a) {
    const int64_t item = blockIdx.x, block0 = (int64_t)blockIdx.y * kHsBlockCols;
    if (item >= (int64_t)a.chunk_ptr[a.rows]) return;  // (the grid is an upper bound of the number of chunks)
    int64_t lo_row = 0, hi_row = a.rows;               // the last row whose first chunk is <= item; workgroup-uniform
    while (hi_row - lo_row > 1) {
        const int64_t mid = lo_row + ((hi_row - lo_row) >> 1);
        if ((int64_t)a.chunk_ptr[mid] <= item) lo_row = mid;
        else hi_row = mid;
    }
    const int64_t row = lo_row, c = item - a.chunk_ptr[row];
    int64_t lo = (int64_t)a.occ_ptr[row] + c * hv::kChunk, hi = a.occ_ptr[row + 1];
    if (c < 0 || lo < 0) return;
    hi = hi > a.n_occ ? a.n_occ : hi;
    hi = hi > lo + hv::kChunk ? lo + hv::kChunk : hi;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t i0 = lo; i0 < hi; i0 += kHsInFlight) {
        float u[kHsInFlight][4], v[kHsInFlight][4], g[kHsInFlight];
        bool ok[kHsInFlight];
#pragma unroll
        for (int t = 0; t < kHsInFlight; ++t) {
            const int64_t i = i0 + t;
            const int64_t pos = i < hi ? (int64_t)a.occ_pos[i] : -1;  // workgroup-uniform
            ok[t] = pos >= 0 && pos < a.n_occ;
            const int64_t b = ok[t] ? (pos < a.B ? pos : pos - a.B) : 0;
            const int64_t xb = a.x[b], yb = a.y[b], rb = a.r[b];
            ok[t] = ok[t] && xb >= 0 && xb < a.N && yb >= 0 && yb < a.N && rb >= 0 && rb < a.R;
            g[t] = ok[t] ? hv::sample_grad(a.grad_p[b], a.p[b]) : 0.0f;
            const int64_t D = ok[t] ? a.D : 0;  // (a refused occurrence loads nothing)
            if constexpr (RELATION) {
                hs_load_cols<VEC>(a.Wx + (ok[t] ? xb : 0) * a.D, block0, D, u[t]);
                hs_load_cols<VEC>(a.Wx + (ok[t] ? yb : 0) * a.D, block0, D, v[t]);
            } else {
                const int64_t other = pos < a.B ? yb : xb;
                hs_load_cols<VEC>(a.Wx + (ok[t] ? other : 0) * a.D, block0, D, u[t]);
                hs_load_cols<VEC>(a.Wr + (ok[t] ? rb : 0) * a.D, block0, D, v[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < kHsInFlight; ++t) {
            if (ok[t]) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float second = RELATION ? v[t][k] : hv::regularise_f(v[t][k]);
                    const float prod = u[t][k] * second;
                    acc[k] = hv::add_contribution(acc[k], g[t], prod);
                }
            }
        }
    }
    const bool single = a.chunk_ptr[row + 1] - a.chunk_ptr[row] <= 1;
    if (RELATION && single) {  // the row's one chunk is its sum: close it with f'
        float w[4];
        hs_load_cols<VEC>(a.Wr + row * a.D, block0, a.D, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float f, df;
            hv::regularise(w[k], f, df);
            acc[k] = acc[k] * df;
        }
    }
    if (c == 0) {
        hs_put_cols<VEC>(a.grad + row * a.D, block0, a.D, acc);
    } else {
        const int64_t slot = (int64_t)a.chunk_ptr[row] - row + c - 1;
        if (slot >= 0 && slot < a.n_slots) hs_put_cols<VEC>(a.partials + slot * a.D, block0, a.D, acc);
    }
}

template <bool RELATION, bool VEC>
__global__ __launch_bounds__(kHsThreads) void hin_grad_fold_kernel(HsGrad a) {
    const int64_t row = blockIdx.x, block0 = (int64_t)blockIdx.y * kHsBlockCols;
    const int64_t chunks = (int64_t)a.chunk_ptr[row + 1] - a.chunk_ptr[row];
    if (chunks <= 1) return;
    float tot[4], part[4];
    hs_load_cols<VEC>(a.grad + row * a.D, block0, a.D, part);  // chunk 0
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k] = 0.0f + part[k];
    const int64_t slot0 = (int64_t)a.chunk_ptr[row] - row;
    for (int64_t c = 1; c < chunks; ++c) {
        const int64_t slot = slot0 + c - 1;
        if (slot < 0 || slot >= a.n_slots) break;
        hs_load_cols<VEC>(a.partials + slot * a.D, block0, a.D, part);
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[k] = tot[k] + part[k];
    }
    if constexpr (RELATION) {
        float w[4];
        hs_load_cols<VEC>(a.Wr + row * a.D, block0, a.D, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float f, df;
            hv::regularise(w[k], f, df);
            tot[k] = tot[k] * df;
        }
    }
    hs_put_cols<VEC>(a.grad + row * a.D, block0, a.D, tot);
}

template <bool RELATION>
static int hs_grad(const HsGrad &a, hipStream_t s) {
    const bool vec = a.D % 4 == 0 && aligned_to(a.Wx, 16) && aligned_to(a.Wr, 16) && aligned_to(a.grad, 16) &&
                     aligned_to(a.partials, 16);
    const int64_t items = a.rows + a.n_occ / hv::kChunk;  // every row has a chunk, a row of c occurrences (c - 1) / 512 more
    const unsigned cols = (unsigned)((a.D + kHsBlockCols - 1) / kHsBlockCols);
    const dim3 block(kHsThreads), grid((unsigned)items, cols), fold((unsigned)a.rows, cols);
    if (vec) hipLaunchKernelGGL((hin_grad_chunk_kernel<RELATION, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((hin_grad_chunk_kernel<RELATION, false>), grid, block, 0, s, a);
    if (a.n_occ > hv::kChunk) {  // (otherwise no row has a second chunk)
        if (vec) hipLaunchKernelGGL((hin_grad_fold_kernel<RELATION, true>), fold, block, 0, s, a);
        else hipLaunchKernelGGL((hin_grad_fold_kernel<RELATION, false>), fold, block, 0, s, a);
    }
    return launch_status();
}

static int hv_status(int rc) { return rc == 0 ? COGDL_HIP_OK : (rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE); }

}  // namespace cogdl

using namespace cogdl;

extern "C" int64_t cogdl_hip_hin_pairs_scratch_words(int64_t W) {
    return W < 0 ? 0 : (int64_t)(device_scan_temp_bytes(W + 1, sizeof(int64_t)) / sizeof(int64_t));
}

extern "C" int cogdl_hip_hin_pairs_count(const int64_t *walks, int64_t W, int64_t L, int hop, const int32_t *node_type, int64_t N,
                                         int64_t *offsets, int64_t *scratch, int *flags, void *stream) {
    const int rc = hv::pairs_status(W, L, hop, 0, N);
    if (rc != 0) return hv_status(rc);
    if (!flags || !offsets) return COGDL_HIP_EINVAL;
    if (!aligned_to(flags, 4) || !aligned_to(offsets, 8) || !aligned_to(walks, 8) || !aligned_to(node_type, 4) ||
        !aligned_to(scratch, 8))
        return COGDL_HIP_EALIGN;
    if (W > 0 && (!walks || (N > 0 && !node_type))) return COGDL_HIP_EINVAL;
    if (cogdl_hip_hin_pairs_scratch_words(W) > 0 && !scratch) return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cleared = clear_flags_async(flags, s);
    if (cleared != COGDL_HIP_OK) return cleared;
    const int64_t groups = (W + kHpRun - 1) / kHpRun;
    hipLaunchKernelGGL(hin_pairs_count_kernel, dim3((unsigned)std::max<int64_t>(groups, 1)), dim3(kHpThreads), 0, s, walks, W, L, hop,
                       node_type, N, offsets, flags);
    const int scanned = device_exclusive_sum((const int64_t *)offsets, offsets, W + 1, scratch, s);
    if (scanned != COGDL_HIP_OK) return scanned;
    return launch_status();
}

extern "C" int cogdl_hip_hin_pairs_emit(const int64_t *walks, int64_t W, int64_t L, int hop, int64_t negative,
                                        const int32_t *node_type, const int32_t *type_ptr, const int32_t *type_nodes,
                                        const int32_t *rank, int64_t N, uint64_t seed, const int64_t *offsets, int64_t total,
                                        int64_t *x, int64_t *y, int64_t *key, int64_t *label, int *flags, void *stream) {
    const int rc = hv::pairs_status(W, L, hop, negative, N);
    if (rc != 0) return hv_status(rc);
    if (total < 0 || !flags) return COGDL_HIP_EINVAL;
    if (W == 0 || total == 0) return COGDL_HIP_OK;
    if (!walks || !node_type || !offsets || !x || !y || !key || !label) return COGDL_HIP_EINVAL;
    if (negative > 0 && (!type_ptr || !type_nodes || !rank)) return COGDL_HIP_EINVAL;
    if (!aligned_to(walks, 8) || !aligned_to(offsets, 8) || !aligned_to(x, 8) || !aligned_to(y, 8) || !aligned_to(key, 8) ||
        !aligned_to(label, 8) || !aligned_to(node_type, 4) || !aligned_to(type_ptr, 4) || !aligned_to(type_nodes, 4) ||
        !aligned_to(rank, 4) || !aligned_to(flags, 4))
        return COGDL_HIP_EALIGN;
    const hv::TypeTables tb = {type_ptr, type_nodes, rank, N};
    hipLaunchKernelGGL(hin_pairs_emit_kernel, dim3((unsigned)((W + kHpRun - 1) / kHpRun)), dim3(kHpThreads), 0, (hipStream_t)stream,
                       walks, W, L, hop, negative, node_type, tb, seed, offsets, total, x, y, key, label, flags);
    return launch_status();
}

extern "C" int cogdl_hip_hin_score(const float *Wx, const float *Wr, const int32_t *x, const int32_t *y, const int32_t *r, int64_t B,
                                   int64_t N, int64_t R, int64_t D, float *p, void *stream) {
    const int rc = hv::score_status(B, N, R, D);
    if (rc != 0) return hv_status(rc);
    if (B == 0) return COGDL_HIP_OK;
    if (!x || !y || !r || !p || (D > 0 && ((N > 0 && !Wx) || (R > 0 && !Wr)))) return COGDL_HIP_EINVAL;
    if (!aligned_to(Wx, 4) || !aligned_to(Wr, 4) || !aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(r, 4) || !aligned_to(p, 4))
        return COGDL_HIP_EALIGN;
    const dim3 grid((unsigned)((B + kHsWaves - 1) / kHsWaves)), block(kHsThreads);
    if (D % 4 == 0 && aligned_to(Wx, 16) && aligned_to(Wr, 16))
        hipLaunchKernelGGL(hin_score_kernel<true>, grid, block, 0, (hipStream_t)stream, Wx, Wr, x, y, r, B, N, R, D, p);
    else
        hipLaunchKernelGGL(hin_score_kernel<false>, grid, block, 0, (hipStream_t)stream, Wx, Wr, x, y, r, B, N, R, D, p);
    return launch_status();
}

extern "C" int cogdl_hip_hin_score_grad(const float *Wx, const float *Wr, const int32_t *x, const int32_t *y, const int32_t *r,
                                        const float *p, const float *grad_p, const int32_t *occ_ptr, const int32_t *occ_pos,
                                        const int32_t *chunk_ptr, int64_t B, int64_t N, int64_t R, int64_t D, int relation,
                                        float *grad, float *partials, int64_t partial_rows, void *stream) {
    const int rc = hv::score_status(B, N, R, D);
    if (rc != 0) return hv_status(rc);
    const int64_t rows = relation ? R : N, n_occ = relation ? B : 2 * B;
    if (rows == 0 || D == 0) return COGDL_HIP_OK;
    if (!Wx || !Wr || !grad || !occ_ptr || !chunk_ptr || partial_rows < 0) return COGDL_HIP_EINVAL;
    if (B > 0 && (!x || !y || !r || !p || !grad_p || !occ_pos)) return COGDL_HIP_EINVAL;
    if (partial_rows < n_occ / hv::kChunk || (partial_rows > 0 && !partials)) return COGDL_HIP_EINVAL;
    if (!aligned_to(Wx, 4) || !aligned_to(Wr, 4) || !aligned_to(x, 4) || !aligned_to(y, 4) || !aligned_to(r, 4) || !aligned_to(p, 4) ||
        !aligned_to(grad_p, 4) || !aligned_to(occ_ptr, 4) || !aligned_to(occ_pos, 4) || !aligned_to(chunk_ptr, 4) ||
        !aligned_to(grad, 4) || !aligned_to(partials, 4))
        return COGDL_HIP_EALIGN;
    if (rows + n_occ / hv::kChunk >= 0x7fffffff) return COGDL_HIP_ERANGE;
    const HsGrad a = {Wx, Wr, x, y, r, p, grad_p, occ_ptr, occ_pos, chunk_ptr, B, N, R, D, rows, n_occ, partial_rows, grad, partials};
    return relation ? hs_grad<true>(a, (hipStream_t)stream) : hs_grad<false>(a, (hipStream_t)stream);
}
