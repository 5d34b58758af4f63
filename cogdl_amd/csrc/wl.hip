// wl.hip -- Weisfeiler-Lehman subtree relabelling on a batch of graphs for gfx950: the refinement behind the reference's
// Graph2Vec.wl_iterations (cogdl/models/emb/graph2vec.py:63-78), on a CSR that is already on the device.  The law is
// wl_law.h; the result is exact (it does not depend on the hash) and equals the host twin's (host_wl.cpp) bit for bit.
//
// Per round, on one stream, no read-back:
//   rows       gather labels[r][col] and sort it inside each row into an [E] workspace, and hash (own label, degree, sorted
//              list) per node.  Rows of up to 64 neighbours: one wave per row, ranking in registers (64 shuffles).  Longer
//              rows: one workgroup per row and a bitonic sort in LDS, in two sizes (up to 2048 and up to 32768 entries =
//              128 KiB of the 160 KiB); the long rows are listed once by the validation pass, which also raises
//              kRowTooLong, and the two kernels stride over their lists.
//   insert     open addressing, at least 2 N slots, a slot holds a node id: atomicCAS from empty; against an occupied slot
//              the two nodes' 128-bit hashes are compared; equal: atomicMin the id, else probe on.  The probes are bounded
//              by the table size (kTableFull); nothing spins.  All ids that ever sit in one slot have one hash.
//   look up    (after the kernel boundary) rep(v) = the id in the slot of v's hash, then, for every v != rep(v), own label,
//              degree and sorted list are compared element for element: a difference is a hash collision and raises
//              kCollision, never a wrong label.
//   number     exclusive scan (scan.h) of rep(v) == v, labels[r + 1][v] = scan[rep(v)].
// A validation pass runs first in the stream; every later kernel reads the flags word and does nothing when the structure
// is malformed or a row is too long, so nothing is read out of bounds.
#include "common.h"

#include "scan.h"
#include "wl_law.h"

namespace cogdl {

namespace wl = cogdl_wl;

constexpr int kWlMid = 2048, kWlMidThreads = 256, kWlBigThreads = 1024;
constexpr int kWlStop = wl::kBadPtr | wl::kBadIndex | wl::kRowTooLong;

__device__ __forceinline__ bool wl_stopped(const int *flags) { return (*(const volatile int *)flags & kWlStop) != 0; }

__device__ __forceinline__ uint64_t wl_wave_sum(uint64_t v) {
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, s, kWave), hi = __shfl_xor((uint32_t)(v >> 32), s, kWave);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ uint32_t wl_slot(const wl::Hash &h, uint32_t mask) { return (uint32_t)wl::mix(h.lo ^ (h.hi * wl::kPos)) & mask; }

// structure checks, and the lists of the rows that need a workgroup (counts[0] mid rows, counts[1] big rows)
__global__ void wl_check_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t N, int64_t E,
                                int32_t *__restrict__ mid, int32_t *__restrict__ big, int32_t *__restrict__ counts,
                                int *__restrict__ flags) {
    int err = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t v = first; v <= N; v += stride) {
        const int64_t a = indptr[v];
        if ((v == 0 && a != 0) || (v == N && a != E) || a < 0 || a > E) err |= wl::kBadPtr;
        if (v < N) {
            const int64_t deg = (int64_t)indptr[v + 1] - a;
            if (deg < 0) err |= wl::kBadPtr;
            else if (deg > wl::kMaxDegree) err |= wl::kRowTooLong;
            else if (deg > kWlMid) big[atomicAdd(&counts[1], 1)] = (int32_t)v;
            else if (deg > kWave) mid[atomicAdd(&counts[0], 1)] = (int32_t)v;
        }
    }
    for (int64_t k = first; k < E; k += stride) {
        const int32_t c = indices[k];
        if (c < 0 || c >= N) err |= wl::kBadIndex;
    }
    raise_flags(flags, err);
}

__global__ void wl_hash0_kernel(const int64_t *__restrict__ label0, int64_t N, uint64_t salt, int hash_bits, wl::Hash *__restrict__ hash) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += stride)
        hash[v] = wl::finish(salt, label0[v], 0, 0, 0, hash_bits);
}

// rows of at most 64 neighbours: one wave per row, the rank of every element from 64 shuffles
__global__ __launch_bounds__(256) void wl_rows_wave_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                           const int32_t *__restrict__ prev, int64_t N, uint64_t salt, int hash_bits,
                                                           int32_t *__restrict__ sorted, wl::Hash *__restrict__ hash,
                                                           const int *__restrict__ flags) {
    if (wl_stopped(flags)) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t v = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); v < N; v += n_waves) {
        const int32_t a = indptr[v];
        const int deg = indptr[v + 1] - a;
        if (deg > kWave) continue;
        const int32_t x = lane < deg ? prev[indices[a + lane]] : 0x7fffffff;
        int rank = 0;
        for (int j = 0; j < deg; ++j) {
            const int32_t xj = __shfl(x, j, kWave);
            rank += (xj < x || (xj == x && j < lane)) ? 1 : 0;
        }
        uint64_t s0 = 0, s1 = 0;
        if (lane < deg) {
            sorted[a + rank] = x;
            s0 = wl::element(salt, 0, rank, x);
            s1 = wl::element(salt, 1, rank, x);
        }
        s0 = wl_wave_sum(s0);
        s1 = wl_wave_sum(s1);
        if (lane == 0) hash[v] = wl::finish(salt, prev[v], deg, s0, s1, hash_bits);
    }
}

// longer rows: one workgroup per listed row, a bitonic sort of the padded row in LDS
template <int CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void wl_rows_block_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                                const int32_t *__restrict__ prev, const int32_t *__restrict__ list,
                                                                const int32_t *__restrict__ count, uint64_t salt, int hash_bits,
                                                                int32_t *__restrict__ sorted, wl::Hash *__restrict__ hash,
                                                                const int *__restrict__ flags) {
    __shared__ int32_t buf[CAP];
    __shared__ uint64_t red[2][THREADS / kWave];
    if (wl_stopped(flags)) return;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int n = *count;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t v = list[i], a = indptr[v];
        int deg = indptr[v + 1] - a;
        deg = deg > CAP ? CAP : deg;  // (the list holds rows of this size only)
        int P = kWave * 2;
        while (P < deg) P <<= 1;
        for (int k = tid; k < P; k += THREADS) buf[k] = k < deg ? prev[indices[a + k]] : 0x7fffffff;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const int32_t x = buf[lo], y = buf[hi];
                    if ((x > y) == ((lo & k) == 0)) {
                        buf[lo] = y;
                        buf[hi] = x;
                    }
                }
                __syncthreads();
            }
        uint64_t s0 = 0, s1 = 0;
        for (int k = tid; k < deg; k += THREADS) {
            const int32_t x = buf[k];
            sorted[a + k] = x;
            s0 += wl::element(salt, 0, k, x);
            s1 += wl::element(salt, 1, k, x);
        }
        s0 = wl_wave_sum(s0);
        s1 = wl_wave_sum(s1);
        if (lane == 0) red[0][wave] = s0, red[1][wave] = s1;
        __syncthreads();
        if (tid == 0) {
            uint64_t t0 = 0, t1 = 0;
            for (int w = 0; w < THREADS / kWave; ++w) t0 += red[0][w], t1 += red[1][w];
            hash[v] = wl::finish(salt, prev[v], deg, t0, t1, hash_bits);
        }
        __syncthreads();  // (buf and red are reused by the next row)
    }
}

__global__ void wl_insert_kernel(const wl::Hash *__restrict__ hash, int64_t N, int32_t *__restrict__ table, uint32_t mask,
                                 int *__restrict__ flags) {
    if (wl_stopped(flags)) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int err = 0;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += stride) {
        const wl::Hash h = hash[v];
        uint32_t slot = wl_slot(h, mask);
        bool done = false;
        for (uint32_t probe = 0; probe <= mask && !done; ++probe) {
            const int32_t cur = atomicCAS(&table[slot], -1, (int32_t)v);
            if (cur == -1) done = true;
            else {
                const wl::Hash o = hash[cur];  // (every id that ever sits in this slot has this hash)
                if (o.lo == h.lo && o.hi == h.hi) {
                    atomicMin(&table[slot], (int32_t)v);
                    done = true;
                } else slot = (slot + 1) & mask;
            }
        }
        if (!done) err |= wl::kTableFull;
    }
    raise_flags(flags, err);
}

// one wave per node: rep(v) from the table, then v against rep(v) element for element
template <typename Own>
__global__ __launch_bounds__(256) void wl_lookup_kernel(const int32_t *__restrict__ indptr, const Own *__restrict__ own,
                                                        const int32_t *__restrict__ sorted, const wl::Hash *__restrict__ hash,
                                                        const int32_t *__restrict__ table, uint32_t mask, int64_t N, int use_rows,
                                                        int32_t *__restrict__ rep, int32_t *__restrict__ isrep, int *__restrict__ flags) {
    if (wl_stopped(flags)) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    int err = 0;
    for (int64_t v = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); v < N; v += n_waves) {
        const wl::Hash h = hash[v];
        uint32_t slot = wl_slot(h, mask);
        int32_t r = -1;
        for (uint32_t probe = 0; probe <= mask; ++probe) {
            const int32_t u = table[slot];
            if (u < 0 || u >= N) break;
            const wl::Hash o = hash[u];
            if (o.lo == h.lo && o.hi == h.hi) {
                r = u;
                break;
            }
            slot = (slot + 1) & mask;
        }
        if (r < 0) {  // (the insert pass ran out of probes for v and said so)
            err |= wl::kTableFull;
            r = (int32_t)v;
        }
        if (r != v) {
            bool differ = own[v] != own[r];
            if (use_rows) {
                const int32_t av = indptr[v], ar = indptr[r];
                const int dv = indptr[v + 1] - av, dr = indptr[r + 1] - ar;
                differ |= dv != dr;
                const int m = dv < dr ? dv : dr;
                for (int k = lane; k < m; k += kWave) differ |= sorted[av + k] != sorted[ar + k];
            }
            if (__any(differ)) err |= wl::kCollision;
        }
        if (lane == 0) {
            rep[v] = r;
            isrep[v] = r == v ? 1 : 0;
        }
    }
    raise_flags(flags, err);
}

__global__ void wl_number_kernel(const int32_t *__restrict__ rep, const int32_t *__restrict__ isrep, const int32_t *__restrict__ scan,
                                 int64_t N, int32_t *__restrict__ labels, int64_t *__restrict__ classes, const int *__restrict__ flags) {
    if (wl_stopped(flags)) return;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += stride) {
        labels[v] = scan[rep[v]];
        if (v == N - 1) *classes = (int64_t)scan[v] + isrep[v];
    }
}

inline size_t wl_up(size_t b) { return (b + 255) / 256 * 256; }

struct WlWs {
    int32_t *sorted, *table, *rep, *isrep, *scan, *mid, *big, *counts;
    wl::Hash *hash;
    void *scan_temp;
    size_t bytes;
};

static WlWs wl_carve(void *ws, int64_t N, int64_t E) {
    char *p = (char *)ws;
    WlWs w;
    auto take = [&](size_t b) {
        char *q = p;
        p += wl_up(b);
        return (void *)q;
    };
    w.hash = (wl::Hash *)take((size_t)N * sizeof(wl::Hash));
    w.sorted = (int32_t *)take((size_t)E * 4);
    w.table = (int32_t *)take((size_t)wl::table_slots(N) * 4);
    w.rep = (int32_t *)take((size_t)N * 4);
    w.isrep = (int32_t *)take((size_t)N * 4);
    w.scan = (int32_t *)take((size_t)N * 4);
    w.mid = (int32_t *)take((size_t)N * 4);
    w.big = (int32_t *)take((size_t)N * 4);
    w.counts = (int32_t *)take(8);
    w.scan_temp = take(device_scan_temp_bytes(N, sizeof(int32_t)));
    w.bytes = (size_t)(p - (char *)ws);
    return w;
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_wl_max_degree(void) { return wl::kMaxDegree; }

extern "C" size_t cogdl_hip_wl_workspace_bytes(int64_t N, int64_t E) {
    if (wl::args_status(N, E, 0, 128) != 0) return 0;
    return wl_carve(nullptr, N, E).bytes;
}

extern "C" int cogdl_hip_wl_labels(const int32_t *indptr, const int32_t *indices, const int64_t *label0, int64_t N, int64_t E,
                                   int64_t rounds, int hash_bits, uint64_t salt, int32_t *labels, int64_t *classes, int *flags,
                                   void *ws, size_t ws_bytes, void *stream) {
    const int rc = wl::args_status(N, E, rounds, hash_bits);
    if (rc) return rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (!indptr || !flags || !classes || (E > 0 && !indices) || (N > 0 && (!label0 || !labels || !ws))) return COGDL_HIP_EINVAL;
    if (N > 0 && !aligned_to(ws, 16)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int cleared = clear_flags_async(flags, s);
    if (cleared != COGDL_HIP_OK) return cleared;
    if (fill_u32_async(classes, 0u, (size_t)(rounds + 1) * 2, s) != hipSuccess) return launch_status();
    if (N == 0) return launch_status();
    const WlWs w = wl_carve(ws, N, E);
    if (ws_bytes < w.bytes) return COGDL_HIP_EINVAL;
    const uint32_t mask = (uint32_t)(wl::table_slots(N) - 1);
    const unsigned flat = (unsigned)std::min<int64_t>((N + 255) / 256, 8192);
    const unsigned waves = (unsigned)std::min<int64_t>((N + 3) / 4, 65536);
    if (fill_u32_async(w.counts, 0u, 2, s) != hipSuccess) return launch_status();
    hipLaunchKernelGGL(wl_check_kernel, dim3((unsigned)std::min<int64_t>((std::max<int64_t>(N + 1, E) + 255) / 256, 8192)), dim3(256), 0, s,
                       indptr, indices, N, E, w.mid, w.big, w.counts, flags);
    int st = launch_status();
    if (st != COGDL_HIP_OK) return st;
    for (int64_t r = 0; r <= rounds; ++r) {
        const int32_t *prev = r > 0 ? labels + (r - 1) * N : nullptr;
        if (fill_u32_async(w.table, 0xffffffffu, (size_t)mask + 1, s) != hipSuccess) return launch_status();
        if (r == 0) {
            hipLaunchKernelGGL(wl_hash0_kernel, dim3(flat), dim3(256), 0, s, label0, N, salt, hash_bits, w.hash);
        } else {
            hipLaunchKernelGGL(wl_rows_wave_kernel, dim3(waves), dim3(256), 0, s, indptr, indices, prev, N, salt, hash_bits, w.sorted,
                               w.hash, flags);
            hipLaunchKernelGGL((wl_rows_block_kernel<kWlMid, kWlMidThreads>), dim3(2048), dim3(kWlMidThreads), 0, s, indptr, indices, prev,
                               w.mid, w.counts, salt, hash_bits, w.sorted, w.hash, flags);
            hipLaunchKernelGGL((wl_rows_block_kernel<wl::kMaxDegree, kWlBigThreads>), dim3(256), dim3(kWlBigThreads), 0, s, indptr,
                               indices, prev, w.big, w.counts + 1, salt, hash_bits, w.sorted, w.hash, flags);
        }
        hipLaunchKernelGGL(wl_insert_kernel, dim3(flat), dim3(256), 0, s, w.hash, N, w.table, mask, flags);
        if (r == 0)
            hipLaunchKernelGGL((wl_lookup_kernel<int64_t>), dim3(waves), dim3(256), 0, s, indptr, label0, w.sorted, w.hash, w.table, mask, N,
                               0, w.rep, w.isrep, flags);
        else
            hipLaunchKernelGGL((wl_lookup_kernel<int32_t>), dim3(waves), dim3(256), 0, s, indptr, prev, w.sorted, w.hash, w.table, mask, N, 1,
                               w.rep, w.isrep, flags);
        st = launch_status();
        if (st != COGDL_HIP_OK) return st;
        st = device_exclusive_sum((const int32_t *)w.isrep, w.scan, N, w.scan_temp, s);
        if (st != COGDL_HIP_OK) return st;
        hipLaunchKernelGGL(wl_number_kernel, dim3(flat), dim3(256), 0, s, w.rep, w.isrep, w.scan, N, labels + r * N, classes + r, flags);
        st = launch_status();
        if (st != COGDL_HIP_OK) return st;
    }
    return COGDL_HIP_OK;
}
