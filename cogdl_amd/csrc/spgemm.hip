// spgemm.hip -- sparse x sparse product C = A . B on int32 CSR with fp32 values, its value gradients, and the segmented
// duplicate sum behind COO canonicalisation, for gfx950 (wave64).  The reference reaches this product through
// torch_sparse.spspmm (models/nn/srgcn.py, models/nn/graph_unet.py, models/nn/gtn.py).
//
// Forward, per output row i, with ub_i = sum over k in A_i of nnz(B_k) (the row's number of products):
//   count   spgemm_ub_kernel: ub_i; spgemm_bin_kernel: the row goes to one of four lists by ub_i (integer atomics on the
//           list counters, one per wave and list: the order inside a list varies, nothing computed from it does);
//           spgemm_rows_kernel<.., FILL = false> on the three LDS bins (ub <= 256 / 1024 / 4096): the row's product
//           columns go into an LDS hash set (integer CAS), whose insertions are the row's nnz;
//           rowptrC = the scan (scan.h) of the counts, nnz(C) into the plan's header.
//   hub     rows with ub_i > 4096 (the global-memory path): cogdl_hip_spgemm_expand writes their products into a CSR in
//           global memory (expansion order); the caller sorts every row by column with two stable transposes
//           (cogdl_hip_csr2csc) and sums the runs (cogdl_hip_coo_dupsum); cogdl_hip_spgemm_rowptr then redoes the scan.
//   fill    spgemm_rows_kernel<.., FILL = true> on the LDS bins: the products expanded into LDS as 64-bit keys (column << 32 |
//           expansion index), bitonic-sorted, the column runs summed; a copy of the hub rows' canonical results.
// Every output value is the sum of its products in expansion order (A_i's entries in CSR order, then B_k's), summed by
// one thread: no float atomics, the same bits on every call, whichever path a row takes.  The pattern is structural:
// a run whose products cancel stays in C as an explicit 0.
// Backward (one 16-lane group per gradient entry, each a gather with a single owner; no atomics):
//   gA[(i,k)] = sum_j G[i,j] B[k,j]     B_k's entries, each looked up in row i of C by binary search
//   gB[(k,j)] = sum_i A[i,k] G[i,j]     column k of A (the CSC of cogdl_hip_csr2csc), each row i of C searched for j
#include "common.h"
#include "scan.h"

namespace cogdl {
namespace {

constexpr int64_t kSpgCap0 = 256, kSpgCap1 = 1024, kSpgCap2 = 4096;  // LDS bins 0..2; list 3 holds the hub rows
constexpr int kSpgHdr = 8;                          // int64 header: bin counts [0..3], hub products [4], nnz(C) [5]
constexpr int kGroup = 16;                          // lanes per gradient entry

struct Plan {
    int64_t *hdr;
    int64_t *ub;
    int32_t *row_nnz;
    int32_t *lists;  // 4 lists of m entries
};

__host__ __device__ inline size_t plan_bytes(int64_t m) { return (size_t)kSpgHdr * 8 + (size_t)m * (8 + 4 + 16); }

inline Plan plan_of(void *p, int64_t m) {
    char *c = (char *)p;
    Plan pl;
    pl.hdr = (int64_t *)c;
    pl.ub = (int64_t *)(c + kSpgHdr * 8);
    pl.row_nnz = (int32_t *)(c + kSpgHdr * 8 + m * 8);
    pl.lists = (int32_t *)(c + kSpgHdr * 8 + m * 12);
    return pl;
}

__global__ void spgemm_zero_hdr_kernel(int64_t *hdr) {
    if (threadIdx.x < kSpgHdr) hdr[threadIdx.x] = 0;
}

// One wave per row: ub_i and row_nnz_i = 0.
__global__ __launch_bounds__(256) void spgemm_ub_kernel(const int32_t *__restrict__ rowptrA, const int32_t *__restrict__ colA,
                                                        const int32_t *__restrict__ rowptrB, int64_t m, Plan pl) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x / kWave);
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x >> 6); i < m; i += waves) {
        const int a0 = rowptrA[i], a1 = rowptrA[i + 1];
        int64_t ub = 0;
        for (int e = a0 + lane; e < a1; e += kWave) {
            const int kk = colA[e];
            ub += rowptrB[kk + 1] - rowptrB[kk];
        }
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) {  // (integer: any order)
            const unsigned lo = __shfl_xor((unsigned)(uint64_t)ub, s, kWave), hi = __shfl_xor((unsigned)((uint64_t)ub >> 32), s, kWave);
            ub += (int64_t)(((uint64_t)hi << 32) | lo);
        }
        if (lane == 0) {
            pl.ub[i] = ub;
            pl.row_nnz[i] = 0;
        }
    }
}

// One thread per row: the row's bin, appended to the bin's list with ONE counter atomic per wave and bin (ballot + rank):
// one atomic per row on the four counters serialised at ~12 ns each -- 2.0 ms of the arxiv-sized product (kernel trace).
__global__ __launch_bounds__(256) void spgemm_bin_kernel(int64_t m, Plan pl) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < m; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        int b = -1;
        int64_t ub = 0;
        if (i < m) {
            ub = pl.ub[i];
            if (ub > 0) b = ub <= kSpgCap0 ? 0 : ub <= kSpgCap1 ? 1 : ub <= kSpgCap2 ? 2 : 3;
        }
        for (int bb = 0; bb < 4; ++bb) {
            const unsigned long long mask = __ballot(b == bb);
            if (mask == 0) continue;  // (wave-uniform)
            const int leader = __ffsll((long long)mask) - 1;
            unsigned long long first = 0;
            if (lane == leader) first = atomicAdd((unsigned long long *)&pl.hdr[bb], (unsigned long long)__popcll(mask));
            const unsigned lo = __shfl((unsigned)first, leader, kWave), hi = __shfl((unsigned)(first >> 32), leader, kWave);
            first = ((unsigned long long)hi << 32) | lo;
            if (b == bb) {
                const int rank = __popcll(mask & ((1ull << lane) - 1));
                pl.lists[(int64_t)bb * m + (int64_t)(first + rank)] = (int32_t)i;
                if (bb == 3) atomicAdd((unsigned long long *)&pl.hdr[4], (unsigned long long)ub);
            }
        }
    }
}

// Exclusive sum of one int per thread over the workgroup; `total` = the workgroup's sum.  s_wsum: THREADS / 64 ints.
template <int THREADS>
__device__ __forceinline__ int block_exclusive_sum(int v, int *s_wsum, int &total) {
    const int lane = threadIdx.x & (kWave - 1);
    const int incl = wave_inclusive(v, lane, ScanPlus());
    const int before = waves_exclusive<int, ScanPlus, THREADS / kWave>(scan_bcast_last(incl), 0, ScanPlus(), s_wsum, total);
    return before + incl - v;
}

// The products of one row in expansion order: emit(p, column, value) for p = 0, 1, .. (value = valA * valB, or 0 when
// valA is NULL).  A's entries are taken THREADS at a time; a workgroup scan of their B-row lengths places them, then the
// threads share the chunk's products evenly (a binary search over the chunk's offsets per product).  Ends with a barrier.
template <int THREADS, class Emit>
__device__ __forceinline__ void expand_row(const int32_t *__restrict__ colA, const float *__restrict__ valA,
                                           const int32_t *__restrict__ rowptrB, const int32_t *__restrict__ colB,
                                           const float *__restrict__ valB, int a0, int a1, int *s_start, int *s_off,
                                           float *s_av, int *s_wsum, Emit emit) {
    const int tid = threadIdx.x;
    int64_t pos = 0;
    for (int c = a0; c < a1; c += THREADS) {
        const int e = c + tid;
        int len = 0, start = 0;
        float av = 0.f;
        if (e < a1) {
            const int kk = colA[e];
            start = rowptrB[kk];
            len = rowptrB[kk + 1] - start;
            if (valA) av = valA[e];
        }
        int total;
        const int ex = block_exclusive_sum<THREADS>(len, s_wsum, total);
        s_start[tid] = start;
        s_off[tid] = ex;
        s_av[tid] = av;
        __syncthreads();
        const int nvalid = min(THREADS, a1 - c);
        for (int p = tid; p < total; p += THREADS) {
            int lo = 0, hi = nvalid - 1;  // the last entry whose offset is <= p (it has products: see below)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= p) lo = mid; else hi = mid - 1;
            }
            // (an entry without products shares its offset with the next one, and the last entry's offset + length is
            //  `total` > p: the entry found has p < offset + length)
            const int q = s_start[lo] + (p - s_off[lo]);
            emit(pos + p, colB[q], valA ? s_av[lo] * valB[q] : 0.f);
        }
        pos += total;
        __syncthreads();
    }
}

__device__ __forceinline__ int key_col(uint64_t k) { return (int)(k >> 32); }

// One workgroup per row of LDS bin `bin` (grid-stride over the list).  Count: the row's distinct columns (row_nnz) through
// an LDS hash set.  Fill: expand, bitonic sort of (column, expansion index), every column run written to C, summed by one
// thread in expansion order.
template <int THREADS, int CAP, bool FILL>
__global__ __launch_bounds__(THREADS) void spgemm_rows_kernel(const int32_t *__restrict__ rowptrA, const int32_t *__restrict__ colA,
                                                              const float *__restrict__ valA, const int32_t *__restrict__ rowptrB,
                                                              const int32_t *__restrict__ colB, const float *__restrict__ valB,
                                                              int64_t m, Plan pl, int bin, const int32_t *__restrict__ rowptrC,
                                                              int32_t *__restrict__ colC, float *__restrict__ valC) {
    __shared__ uint64_t s_key[CAP];
    __shared__ float s_val[FILL ? CAP : 1];
    __shared__ int s_start[THREADS], s_off[THREADS], s_wsum[THREADS / kWave];
    __shared__ float s_av[THREADS];
    const int tid = threadIdx.x;
    const int64_t count = pl.hdr[bin];
    const int32_t *list = pl.lists + (int64_t)bin * m;
    for (int64_t li = blockIdx.x; li < count; li += gridDim.x) {
        const int i = list[li];
        const int total = (int)pl.ub[i];  // 1 .. CAP (the bin's bound)
        if constexpr (!FILL) {
            // count: the distinct columns through an LDS hash set (integer CAS on the keys only, load factor <= 1/2) --
            // no sort; the table (<= 2 CAP ints) lives in s_key's storage
            int lg = 1;
            while ((1 << lg) < 2 * total) ++lg;
            const int tsize = 1 << lg;
            int *s_hash = reinterpret_cast<int *>(s_key);
            for (int p = tid; p < tsize; p += THREADS) s_hash[p] = -1;
            __syncthreads();
            int mine = 0;
            expand_row<THREADS>(colA, nullptr, rowptrB, colB, valB, rowptrA[i], rowptrA[i + 1], s_start, s_off, s_av, s_wsum,
                                [&](int64_t, int col, float) {
                                    unsigned h = ((unsigned)col * 2654435761u) >> (32 - lg);
                                    while (true) {
                                        const int prev = atomicCAS(&s_hash[h], -1, col);
                                        if (prev == -1) {
                                            ++mine;
                                            break;
                                        }
                                        if (prev == col) break;
                                        h = (h + 1) & (unsigned)(tsize - 1);
                                    }
                                });
            int tot;
            (void)block_exclusive_sum<THREADS>(mine, s_wsum, tot);
            if (tid == 0) pl.row_nnz[i] = tot;
            __syncthreads();  // (LDS reused by the next row)
            continue;
        }
        expand_row<THREADS>(colA, FILL ? valA : nullptr, rowptrB, colB, valB, rowptrA[i], rowptrA[i + 1], s_start, s_off, s_av,
                            s_wsum, [&](int64_t p, int col, float v) {
                                s_key[p] = ((uint64_t)(uint32_t)col << 32) | (uint32_t)p;
                                if constexpr (FILL) s_val[p] = v;
                            });
        int size = 1;
        while (size < total) size <<= 1;
        for (int p = total + tid; p < size; p += THREADS) s_key[p] = ~0ull;
        __syncthreads();
        for (int k2 = 2; k2 <= size; k2 <<= 1) {
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < size / 2; t += THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
                    const uint64_t a = s_key[lo], b = s_key[hi];
                    if ((a > b) == ((lo & k2) == 0)) {
                        s_key[lo] = b;
                        s_key[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        int carry = 0;
        const int base = FILL ? rowptrC[i] : 0;
        for (int c = 0; c < total; c += THREADS) {
            const int q = c + tid;
            const bool head = q < total && (q == 0 || key_col(s_key[q]) != key_col(s_key[q - 1]));
            int tot;
            const int ex = block_exclusive_sum<THREADS>(head ? 1 : 0, s_wsum, tot);
            if constexpr (FILL) {
                if (head) {
                    const int col = key_col(s_key[q]);
                    float s = s_val[(uint32_t)s_key[q]];
                    for (int t = q + 1; t < total && key_col(s_key[t]) == col; ++t) s += s_val[(uint32_t)s_key[t]];
                    colC[base + carry + ex] = col;
                    valC[base + carry + ex] = s;
                }
            }
            carry += tot;
        }
        if (!FILL && tid == 0) pl.row_nnz[i] = carry;
        __syncthreads();  // (LDS reused by the next row)
    }
}

// row_nnz of the hub rows from their canonical CSR.
__global__ void spgemm_hub_counts_kernel(Plan pl, int64_t m, const int32_t *__restrict__ hub_rowptr, int64_t n_hub) {
    const int32_t *list = pl.lists + 3 * m;
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hub; h += (int64_t)gridDim.x * blockDim.x)
        pl.row_nnz[list[h]] = hub_rowptr[h + 1] - hub_rowptr[h];
}

// rowptrC from the inclusive int64 scan of row_nnz; nnz(C) into the header (rowptrC is only meaningful when it fits int32).
__global__ void spgemm_rowptr_kernel(const int64_t *__restrict__ incl, int64_t m, int32_t *__restrict__ rowptrC, int64_t *hdr) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = i == 0 ? 0 : incl[i - 1];
        rowptrC[i] = (int32_t)(v <= 0x7fffffff ? v : 0x7fffffff);
        if (i == m) hdr[5] = v;
    }
}

__global__ void spgemm_hub_ub_kernel(Plan pl, int64_t m, int64_t n_hub, int64_t *__restrict__ out) {
    const int32_t *list = pl.lists + 3 * m;
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_hub; h += (int64_t)gridDim.x * blockDim.x)
        out[h] = pl.ub[list[h]];
}

__global__ void spgemm_hub_rowptr_kernel(const int64_t *__restrict__ incl, int64_t n_hub, int32_t *__restrict__ hub_rowptr) {
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h <= n_hub; h += (int64_t)gridDim.x * blockDim.x)
        hub_rowptr[h] = h == 0 ? 0 : (int32_t)incl[h - 1];
}

// The hub rows' products into global memory, row h at hub_rowptr[h], in expansion order.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void spgemm_expand_kernel(const int32_t *__restrict__ rowptrA, const int32_t *__restrict__ colA,
                                                                const float *__restrict__ valA, const int32_t *__restrict__ rowptrB,
                                                                const int32_t *__restrict__ colB, const float *__restrict__ valB,
                                                                int64_t m, Plan pl, int64_t n_hub, const int32_t *__restrict__ hub_rowptr,
                                                                int32_t *__restrict__ out_col, float *__restrict__ out_val) {
    __shared__ int s_start[THREADS], s_off[THREADS], s_wsum[THREADS / kWave];
    __shared__ float s_av[THREADS];
    const int32_t *list = pl.lists + 3 * m;
    for (int64_t h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const int i = list[h];
        const int64_t base = hub_rowptr[h];
        expand_row<THREADS>(colA, valA, rowptrB, colB, valB, rowptrA[i], rowptrA[i + 1], s_start, s_off, s_av, s_wsum,
                            [&](int64_t p, int col, float v) {
                                out_col[base + p] = col;
                                out_val[base + p] = v;
                            });
    }
}

// The hub rows' canonical results into C (one workgroup per hub row).
__global__ __launch_bounds__(256) void spgemm_hub_copy_kernel(Plan pl, int64_t m, int64_t n_hub, const int32_t *__restrict__ hub_rowptr,
                                                              const int32_t *__restrict__ hub_col, const float *__restrict__ hub_val,
                                                              const int32_t *__restrict__ rowptrC, int32_t *__restrict__ colC,
                                                              float *__restrict__ valC) {
    const int32_t *list = pl.lists + 3 * m;
    for (int64_t h = blockIdx.x; h < n_hub; h += gridDim.x) {
        const int64_t src = hub_rowptr[h], len = hub_rowptr[h + 1] - src, dst = rowptrC[list[h]];
        for (int64_t t = threadIdx.x; t < len; t += blockDim.x) {
            colC[dst + t] = hub_col[src + t];
            valC[dst + t] = hub_val[src + t];
        }
    }
}

// ---- segmented duplicate sum -------------------------------------------------------------------------------------
__global__ void dupsum_row_starts_kernel(const int32_t *__restrict__ rowptr, int64_t rows, int32_t *__restrict__ flag) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x)
        if (rowptr[r] < rowptr[r + 1]) flag[rowptr[r]] = 1;
}

__global__ void dupsum_heads_kernel(const int32_t *__restrict__ col, int64_t nnz, int32_t *__restrict__ flag) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * blockDim.x)
        if (t > 0 && col[t] != col[t - 1]) flag[t] = 1;
}

__global__ void dupsum_rowptr_kernel(const int32_t *__restrict__ rowptr, int64_t rows, int64_t nnz, const int32_t *__restrict__ flag,
                                     const int32_t *__restrict__ uex, int32_t *__restrict__ rowptr_u) {
    const int32_t u_total = uex[nnz - 1] + flag[nnz - 1];
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int32_t p = rowptr[r];
        rowptr_u[r] = p < nnz ? uex[p] : u_total;
    }
}

// One thread per run head: the run's values summed in sorted order; map[order[t]] = the run's index.
__global__ void dupsum_runs_kernel(const int32_t *__restrict__ col, const int32_t *__restrict__ order, const float *__restrict__ val,
                                   int64_t nnz, const int32_t *__restrict__ flag, const int32_t *__restrict__ uex,
                                   int32_t *__restrict__ col_u, float *__restrict__ val_u, int32_t *__restrict__ map) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * blockDim.x) {
        if (!flag[t]) continue;
        const int32_t u = uex[t];
        col_u[u] = col[t];
        float s = 0.f;
        int64_t q = t;
        do {
            const int32_t o = order ? order[q] : (int32_t)q;
            if (val) s = q == t ? val[o] : s + val[o];
            if (map) map[o] = u;
            ++q;
        } while (q < nnz && !flag[q]);
        if (val_u) val_u[u] = s;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------
// Largest r in [0, n) with ptr[r] <= e (the row of CSR position e; empty rows share their start with the next row).
__device__ __forceinline__ int row_of(const int32_t *__restrict__ ptr, int n, int e) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ptr[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Position of column j in colC[c0, c1) (sorted), or -1.
__device__ __forceinline__ int find_col(const int32_t *__restrict__ colC, int c0, int c1, int j) {
    int lo = c0, hi = c1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (colC[mid] < j) lo = mid + 1; else hi = mid;
    }
    return lo < c1 && colC[lo] == j ? lo : -1;
}

__device__ __forceinline__ float group_sum(float s) {  // fixed tree over the 16 lanes of a group
#pragma unroll
    for (int o = kGroup / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kGroup);
    return s;
}

__global__ __launch_bounds__(256) void spgemm_grad_a_kernel(const int32_t *__restrict__ rowptrA, const int32_t *__restrict__ colA,
                                                            const int32_t *__restrict__ rowptrB, const int32_t *__restrict__ colB,
                                                            const float *__restrict__ valB, const int32_t *__restrict__ rowptrC,
                                                            const int32_t *__restrict__ colC, const float *__restrict__ gradC,
                                                            float *__restrict__ gradA, int m, int64_t nnzA) {
    const int l = threadIdx.x & (kGroup - 1);
    const int64_t groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; e < nnzA; e += groups) {
        const int i = row_of(rowptrA, m, (int)e), kk = colA[e];
        const int c0 = rowptrC[i], c1 = rowptrC[i + 1];
        float s = 0.f;
        for (int q = rowptrB[kk] + l; q < rowptrB[kk + 1]; q += kGroup) {
            const int p = find_col(colC, c0, c1, colB[q]);
            if (p >= 0) s += gradC[p] * valB[q];
        }
        s = group_sum(s);
        if (l == 0) gradA[e] = s;
    }
}

__global__ __launch_bounds__(256) void spgemm_grad_b_kernel(const int32_t *__restrict__ colptrAT, const int32_t *__restrict__ rowindAT,
                                                            const int32_t *__restrict__ permAT, const float *__restrict__ valA,
                                                            const int32_t *__restrict__ rowptrB, const int32_t *__restrict__ colB,
                                                            const int32_t *__restrict__ rowptrC, const int32_t *__restrict__ colC,
                                                            const float *__restrict__ gradC, float *__restrict__ gradB, int k,
                                                            int64_t nnzB) {
    const int l = threadIdx.x & (kGroup - 1);
    const int64_t groups = (int64_t)gridDim.x * (blockDim.x / kGroup);
    for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup; e < nnzB; e += groups) {
        const int kk = row_of(rowptrB, k, (int)e), j = colB[e];
        float s = 0.f;
        for (int q = colptrAT[kk] + l; q < colptrAT[kk + 1]; q += kGroup) {
            const int i = rowindAT[q];
            const int p = find_col(colC, rowptrC[i], rowptrC[i + 1], j);
            if (p >= 0) s += valA[permAT[q]] * gradC[p];
        }
        s = group_sum(s);
        if (l == 0) gradB[e] = s;
    }
}

inline bool fits_i32(int64_t v) { return v >= 0 && v <= 0x7fffffff; }
inline unsigned grid_for(int64_t work, int per_block, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + per_block - 1) / per_block, cap));
}
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// Scan of row_nnz -> rowptrC, nnz(C) into hdr[5].  workspace: spgemm_scan_bytes(m).
size_t spgemm_scan_bytes(int64_t m) { return up256((size_t)m * 8) + device_scan_temp_bytes(m, 8); }

int spgemm_scan(Plan pl, int64_t m, int32_t *rowptrC, void *ws, hipStream_t s) {
    int64_t *incl = (int64_t *)ws;
    void *temp = (char *)ws + up256((size_t)m * 8);
    const int rc = device_scan<true>((const int32_t *)pl.row_nnz, incl, m, (int64_t)0, (int64_t)0, ScanPlus(), temp, s);
    if (rc != COGDL_HIP_OK) return rc;
    hipLaunchKernelGGL(spgemm_rowptr_kernel, dim3(grid_for(m + 1, 256, 4096)), dim3(256), 0, s, (const int64_t *)incl, m, rowptrC,
                       pl.hdr);
    return launch_status();
}

template <bool FILL>
void launch_rows(const int32_t *rowptrA, const int32_t *colA, const float *valA, const int32_t *rowptrB, const int32_t *colB,
                 const float *valB, int64_t m, Plan pl, const int32_t *rowptrC, int32_t *colC, float *valC, hipStream_t s) {
    const unsigned g = grid_for(m, 1, 65536);  // (a grid of 4096 left the 64-thread bin at 16 waves per CU: 0.64x torch)
    hipLaunchKernelGGL((spgemm_rows_kernel<64, (int)kSpgCap0, FILL>), dim3(g), dim3(64), 0, s, rowptrA, colA, valA, rowptrB, colB,
                       valB, m, pl, 0, rowptrC, colC, valC);
    hipLaunchKernelGGL((spgemm_rows_kernel<256, (int)kSpgCap1, FILL>), dim3(g), dim3(256), 0, s, rowptrA, colA, valA, rowptrB, colB,
                       valB, m, pl, 1, rowptrC, colC, valC);
    hipLaunchKernelGGL((spgemm_rows_kernel<512, (int)kSpgCap2, FILL>), dim3(g), dim3(512), 0, s, rowptrA, colA, valA, rowptrB, colB,
                       valB, m, pl, 2, rowptrC, colC, valC);
}

}  // namespace
}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_spgemm_plan_bytes(int64_t m) { return m < 0 ? 0 : plan_bytes(m); }

extern "C" size_t cogdl_hip_spgemm_count_workspace_bytes(int64_t m) { return m < 0 ? 0 : std::max<size_t>(256, spgemm_scan_bytes(m)); }

extern "C" int cogdl_hip_spgemm_count(const int32_t *rowptrA, const int32_t *colA, const int32_t *rowptrB, const int32_t *colB,
                                      int64_t m, int64_t k, int64_t n, void *plan, int32_t *rowptrC, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    if (m < 0 || k < 0 || n < 0) return COGDL_HIP_EINVAL;
    if (!fits_i32(m) || !fits_i32(k) || !fits_i32(n) || m + 1 > 0x7fffffff) return COGDL_HIP_ERANGE;
    if (!plan || !rowptrC || !rowptrA || (k > 0 && !rowptrB)) return COGDL_HIP_EINVAL;
    if (!aligned_to(plan, 8)) return COGDL_HIP_EALIGN;
    if (!workspace || workspace_bytes < spgemm_scan_bytes(m)) return COGDL_HIP_EWORKSPACE;
    if (!aligned_to(workspace, 256)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    Plan pl = plan_of(plan, m);
    hipLaunchKernelGGL(spgemm_zero_hdr_kernel, dim3(1), dim3(64), 0, s, pl.hdr);
    if (m > 0) {
        hipLaunchKernelGGL(spgemm_ub_kernel, dim3(grid_for(m, 4, 8192)), dim3(256), 0, s, rowptrA, colA, rowptrB, m, pl);
        hipLaunchKernelGGL(spgemm_bin_kernel, dim3(grid_for(m, 256, 4096)), dim3(256), 0, s, m, pl);
        launch_rows<false>(rowptrA, colA, nullptr, rowptrB, colB, nullptr, m, pl, nullptr, nullptr, nullptr, s);
    }
    if (launch_status() != COGDL_HIP_OK) return COGDL_HIP_ELAUNCH;
    return spgemm_scan(pl, m, rowptrC, workspace, s);
}

extern "C" size_t cogdl_hip_spgemm_expand_workspace_bytes(int64_t n_hub) {
    return n_hub < 0 ? 0 : std::max<size_t>(256, up256((size_t)n_hub * 16) + device_scan_temp_bytes(n_hub, 8));
}

extern "C" int cogdl_hip_spgemm_expand(const int32_t *rowptrA, const int32_t *colA, const float *valA, const int32_t *rowptrB,
                                       const int32_t *colB, const float *valB, int64_t m, const void *plan, int64_t n_hub,
                                       int64_t hub_products, int32_t *hub_rowptr, int32_t *hub_col, float *hub_val, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    if (m < 0 || n_hub < 0 || n_hub > m || hub_products < 0) return COGDL_HIP_EINVAL;
    if (!fits_i32(m) || hub_products > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    if (n_hub == 0) return COGDL_HIP_OK;
    if (!plan || !hub_rowptr || !rowptrA || !colA || !valA || !rowptrB || !colB || !valB || !hub_col || !hub_val)
        return COGDL_HIP_EINVAL;
    if (!workspace || workspace_bytes < cogdl_hip_spgemm_expand_workspace_bytes(n_hub)) return COGDL_HIP_EWORKSPACE;
    if (!aligned_to(workspace, 256)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    Plan pl = plan_of((void *)plan, m);
    int64_t *ub = (int64_t *)workspace, *incl = ub + n_hub;
    void *temp = (char *)workspace + up256((size_t)n_hub * 16);
    hipLaunchKernelGGL(spgemm_hub_ub_kernel, dim3(grid_for(n_hub, 256, 4096)), dim3(256), 0, s, pl, m, n_hub, ub);
    int rc = device_scan<true>((const int64_t *)ub, incl, n_hub, (int64_t)0, (int64_t)0, ScanPlus(), temp, s);
    if (rc != COGDL_HIP_OK) return rc;
    hipLaunchKernelGGL(spgemm_hub_rowptr_kernel, dim3(grid_for(n_hub + 1, 256, 4096)), dim3(256), 0, s, (const int64_t *)incl, n_hub,
                       hub_rowptr);
    hipLaunchKernelGGL(spgemm_expand_kernel<256>, dim3(grid_for(n_hub, 1, 4096)), dim3(256), 0, s, rowptrA, colA, valA, rowptrB, colB,
                       valB, m, pl, n_hub, (const int32_t *)hub_rowptr, hub_col, hub_val);
    return launch_status();
}

extern "C" size_t cogdl_hip_spgemm_rowptr_workspace_bytes(int64_t m) { return cogdl_hip_spgemm_count_workspace_bytes(m); }

extern "C" int cogdl_hip_spgemm_rowptr(void *plan, int64_t m, int64_t n_hub, const int32_t *hub_rowptr, int32_t *rowptrC,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    if (m < 0 || n_hub < 0 || n_hub > m) return COGDL_HIP_EINVAL;
    if (!fits_i32(m)) return COGDL_HIP_ERANGE;
    if (!plan || !rowptrC || (n_hub > 0 && !hub_rowptr)) return COGDL_HIP_EINVAL;
    if (!workspace || workspace_bytes < spgemm_scan_bytes(m)) return COGDL_HIP_EWORKSPACE;
    if (!aligned_to(workspace, 256) || !aligned_to(plan, 8)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    Plan pl = plan_of(plan, m);
    if (n_hub > 0)
        hipLaunchKernelGGL(spgemm_hub_counts_kernel, dim3(grid_for(n_hub, 256, 4096)), dim3(256), 0, s, pl, m, hub_rowptr, n_hub);
    if (launch_status() != COGDL_HIP_OK) return COGDL_HIP_ELAUNCH;
    return spgemm_scan(pl, m, rowptrC, workspace, s);
}

extern "C" int cogdl_hip_spgemm_fill(const int32_t *rowptrA, const int32_t *colA, const float *valA, const int32_t *rowptrB,
                                     const int32_t *colB, const float *valB, int64_t m, int64_t k, int64_t n, const void *plan,
                                     const int32_t *rowptrC, int64_t nnzC, int32_t *colC, float *valC, int64_t n_hub,
                                     const int32_t *hub_rowptr, const int32_t *hub_col, const float *hub_val, void *stream) {
    if (m < 0 || k < 0 || n < 0 || nnzC < 0 || n_hub < 0 || n_hub > m) return COGDL_HIP_EINVAL;
    if (!fits_i32(m) || !fits_i32(k) || !fits_i32(n) || !fits_i32(nnzC)) return COGDL_HIP_ERANGE;
    if (m == 0 || nnzC == 0) return COGDL_HIP_OK;
    if (!plan || !rowptrC || !colC || !valC || !rowptrA || !colA || !valA || !rowptrB || !colB || !valB) return COGDL_HIP_EINVAL;
    if (n_hub > 0 && (!hub_rowptr || !hub_col || !hub_val)) return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    Plan pl = plan_of((void *)plan, m);
    launch_rows<true>(rowptrA, colA, valA, rowptrB, colB, valB, m, pl, rowptrC, colC, valC, s);
    if (n_hub > 0)
        hipLaunchKernelGGL(spgemm_hub_copy_kernel, dim3(grid_for(n_hub, 1, 4096)), dim3(256), 0, s, pl, m, n_hub, hub_rowptr, hub_col,
                           hub_val, rowptrC, colC, valC);
    return launch_status();
}

extern "C" size_t cogdl_hip_coo_dupsum_workspace_bytes(int64_t nnz) {
    return nnz < 0 ? 0 : std::max<size_t>(256, 2 * up256((size_t)nnz * 4) + device_scan_temp_bytes(nnz, 4));
}

extern "C" int cogdl_hip_coo_dupsum(const int32_t *rowptr, const int32_t *col, const int32_t *order, const float *val, int64_t rows,
                                    int64_t nnz, int32_t *rowptr_u, int32_t *col_u, float *val_u, int32_t *map, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    if (rows < 0 || nnz < 0) return COGDL_HIP_EINVAL;
    if (!fits_i32(rows) || rows + 1 > 0x7fffffff || nnz > COGDL_HIP_SEGMENT_MAX_EDGES) return COGDL_HIP_ERANGE;
    if (!rowptr || !rowptr_u || (nnz > 0 && (!col || !col_u || (val && !val_u)))) return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (nnz == 0) {
        (void)fill_u32_async(rowptr_u, 0, (size_t)rows + 1, s);
        return launch_status();
    }
    if (!workspace || workspace_bytes < cogdl_hip_coo_dupsum_workspace_bytes(nnz)) return COGDL_HIP_EWORKSPACE;
    if (!aligned_to(workspace, 256)) return COGDL_HIP_EALIGN;
    int32_t *flag = (int32_t *)workspace, *uex = (int32_t *)((char *)workspace + up256((size_t)nnz * 4));
    void *temp = (char *)workspace + 2 * up256((size_t)nnz * 4);
    (void)fill_u32_async(flag, 0, (size_t)nnz, s);
    const unsigned g = grid_for(nnz, 256, 8192);
    hipLaunchKernelGGL(dupsum_row_starts_kernel, dim3(grid_for(rows, 256, 4096)), dim3(256), 0, s, rowptr, rows, flag);
    hipLaunchKernelGGL(dupsum_heads_kernel, dim3(g), dim3(256), 0, s, col, nnz, flag);
    const int rc = device_exclusive_sum((const int32_t *)flag, uex, nnz, temp, s);
    if (rc != COGDL_HIP_OK) return rc;
    hipLaunchKernelGGL(dupsum_rowptr_kernel, dim3(grid_for(rows + 1, 256, 4096)), dim3(256), 0, s, rowptr, rows, nnz,
                       (const int32_t *)flag, (const int32_t *)uex, rowptr_u);
    hipLaunchKernelGGL(dupsum_runs_kernel, dim3(g), dim3(256), 0, s, col, order, val, nnz, (const int32_t *)flag, (const int32_t *)uex,
                       col_u, val_u, map);
    return launch_status();
}

extern "C" int cogdl_hip_spgemm_grad_a(const int32_t *rowptrA, const int32_t *colA, const int32_t *rowptrB, const int32_t *colB,
                                       const float *valB, const int32_t *rowptrC, const int32_t *colC, const float *gradC,
                                       float *gradA, int64_t m, int64_t nnzA, void *stream) {
    if (m < 0 || nnzA < 0) return COGDL_HIP_EINVAL;
    if (!fits_i32(m) || !fits_i32(nnzA)) return COGDL_HIP_ERANGE;
    if (nnzA == 0) return COGDL_HIP_OK;
    if (m == 0 || !rowptrA || !colA || !rowptrB || !colB || !valB || !rowptrC || !colC || !gradC || !gradA) return COGDL_HIP_EINVAL;
    hipLaunchKernelGGL(spgemm_grad_a_kernel, dim3(grid_for(nnzA, 256 / kGroup, 65536)), dim3(256), 0, (hipStream_t)stream, rowptrA,
                       colA, rowptrB, colB, valB, rowptrC, colC, gradC, gradA, (int)m, nnzA);
    return launch_status();
}

extern "C" int cogdl_hip_spgemm_grad_b(const int32_t *colptrAT, const int32_t *rowindAT, const int32_t *permAT, const float *valA,
                                       const int32_t *rowptrB, const int32_t *colB, const int32_t *rowptrC, const int32_t *colC,
                                       const float *gradC, float *gradB, int64_t k, int64_t nnzB, void *stream) {
    if (k < 0 || nnzB < 0) return COGDL_HIP_EINVAL;
    if (!fits_i32(k) || !fits_i32(nnzB)) return COGDL_HIP_ERANGE;
    if (nnzB == 0) return COGDL_HIP_OK;
    if (k == 0 || !colptrAT || !rowptrB || !colB || !rowptrC || !gradC || !gradB) return COGDL_HIP_EINVAL;
    hipLaunchKernelGGL(spgemm_grad_b_kernel, dim3(grid_for(nnzB, 256 / kGroup, 65536)), dim3(256), 0, (hipStream_t)stream, colptrAT,
                       rowindAT, permAT, valA, rowptrB, colB, rowptrC, colC, gradC, gradB, (int)k, nnzB);
    return launch_status();
}
