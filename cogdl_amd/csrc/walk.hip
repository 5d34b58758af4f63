// walk.hip -- random walks on a GPU-resident CSR graph (int64 indptr / indices) for gfx950:
//   cogdl_hip_random_walk     first-order walk with restart  (the contract of cogdl/utils/sampling.py:46-67)
//   cogdl_hip_node2vec_walk   second-order walk with return parameter p and in-out parameter q, unweighted
//                             (the transition weights of cogdl/models/emb/node2vec.py:143-156)
// The draws and the rules of a step live in walk_draw.h, which the host twin (host_ops.cpp) includes too: for equal
// inputs and seed both return the same array.
//
// Shape.  A step is two dependent random loads (the indptr pair, one indices entry) and a handful of integer
// instructions: the kernel is bound by memory latency, so throughput is walkers in flight.  One lane owns one walker (50
// VGPRs, 18 KiB of LDS per workgroup: 8 waves per SIMD; two walkers per lane were measured and were slower).
// Writing walks[w, i] straight from the lanes would make every store instruction touch 64 cache lines 8 L bytes apart
// (measured: 1.7x to 2x slower), so a wave stages kWalkTile steps of its walkers in LDS (rows padded by one entry against
// bank conflicts) and then writes each walker's kWalkTile consecutive steps as one contiguous 64-byte piece, 8 walkers
// per store instruction.  Tiles start at columns that
// are multiples of kWalkTile, so the pieces are 64-byte aligned whenever L is a multiple of 8.  The LDS region is private to
// a wave (no workgroup barrier: waves of a workgroup drift freely, which is what hides the latency).
// Error flags are raised with a plain read-or-write of the flags word (no atomics): concurrent writers of DIFFERENT bits
// may lose one of them, never the fact that the word is non-zero; the result is invalid either way.
#include "common.h"

#include "walk_draw.h"

namespace cogdl {

namespace wk = cogdl_walk;

constexpr int kWalkTile = 8;    // steps staged per walker: 64-byte pieces
constexpr int kWalkBlock = 256;

__device__ __forceinline__ void walk_raise(int *flags, int err) {
    if (err) {
        volatile int *f = flags;
        *f = *f | err;
    }
}

// Wave-private LDS hand-over: LDS operations of a wave complete in order; the compiler must not move them across.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Writes the staged tile of this wave: stage[walker_local][s], columns tile0 .. tile0 + ncols - 1.
__device__ __forceinline__ void walk_flush(const int64_t (*stage)[kWalkTile + 1], int lane, int64_t wave_base, int64_t n_walkers,
                                           int64_t length, int64_t tile0, int ncols, int64_t *__restrict__ walks) {
#pragma unroll
    for (int it = 0; it < kWalkTile; ++it) {
        const int idx = it * kWave + lane;
        const int wl = idx / kWalkTile, s = idx % kWalkTile;
        const int64_t w = wave_base + wl;
        if (w < n_walkers && s < ncols) walks[w * length + tile0 + s] = stage[wl][s];
    }
}

__global__ __launch_bounds__(kWalkBlock) void random_walk_kernel(wk::Graph g, const int64_t *__restrict__ start,
                                                                 int64_t n_walkers, int64_t length, uint64_t restart_t,
                                                                 uint64_t seed, int64_t *__restrict__ walks,
                                                                 int *__restrict__ flags) {
    __shared__ int64_t lds[kWalkBlock / kWave][kWave][kWalkTile + 1];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int64_t(*stage)[kWalkTile + 1] = lds[wave];
    const int64_t wave_base = ((int64_t)blockIdx.x * (kWalkBlock / kWave) + wave) * kWave;
    const int64_t w = wave_base + lane;
    int64_t first = 0, cur = 0;
    int err = -1;  // no walker: parked from the start, nothing raised
    if (w < n_walkers) {
        first = cur = start[w];
        err = wk::valid_id(g, cur) ? 0 : wk::kBadStart;
    }
    for (int64_t tile0 = 0; tile0 < length; tile0 += kWalkTile) {
        const int ncols = (int)(length - tile0 < kWalkTile ? length - tile0 : kWalkTile);
        for (int s = 0; s < ncols; ++s) {
            const int64_t i = tile0 + s;
            if (i > 0) cur = wk::step_first_order(g, seed, w, i, first, cur, restart_t, err);
            stage[lane][s] = cur;
        }
        wave_lds_sync();
        walk_flush(stage, lane, wave_base, n_walkers, length, tile0, ncols, walks);
        wave_lds_sync();
    }
    walk_raise(flags, err > 0 ? err : 0);
}

__global__ __launch_bounds__(kWalkBlock) void node2vec_walk_kernel(wk::Graph g, const int64_t *__restrict__ start,
                                                                   int64_t n_walkers, int64_t length, wk::N2vWeights wt,
                                                                   int max_trials, uint64_t seed, int64_t *__restrict__ walks,
                                                                   int32_t *__restrict__ fallback_steps,
                                                                   int *__restrict__ flags) {
    __shared__ int64_t lds[kWalkBlock / kWave][kWave][kWalkTile + 1];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int64_t(*stage)[kWalkTile + 1] = lds[wave];
    const int64_t wave_base = ((int64_t)blockIdx.x * (kWalkBlock / kWave) + wave) * kWave;
    const int64_t w = wave_base + lane;
    int64_t prev = 0, cur = 0;
    int err = -1;
    int32_t n_fallback = 0;
    if (w < n_walkers) {
        prev = cur = start[w];
        err = wk::valid_id(g, cur) ? 0 : wk::kBadStart;
    }
    for (int64_t tile0 = 0; tile0 < length; tile0 += kWalkTile) {
        const int ncols = (int)(length - tile0 < kWalkTile ? length - tile0 : kWalkTile);
        for (int s = 0; s < ncols; ++s) {
            const int64_t i = tile0 + s;
            if (i > 0) {
                bool fell_back;
                const int64_t nxt = wk::step_node2vec(g, seed, w, i, prev, cur, wt, max_trials, err, fell_back);
                n_fallback += fell_back ? 1 : 0;
                prev = cur;
                cur = nxt;
            }
            stage[lane][s] = cur;
        }
        wave_lds_sync();
        walk_flush(stage, lane, wave_base, n_walkers, length, tile0, ncols, walks);
        wave_lds_sync();
    }
    if (fallback_steps && w < n_walkers) fallback_steps[w] = n_fallback;
    walk_raise(flags, err > 0 ? err : 0);
}

// The metapath walk: random_walk_kernel with the typed step.  A step reads seg[cur * T + t] (and its successor) and one entry
// of indices_t: the same two dependent random loads.  The wanted type does not depend on where the walker stands, so its
// load (4 bytes of a table of a few dozen entries: an L1/L2 hit) is issued one step ahead and is in flight together with the
// two loads of the step before it; a copy of the table in LDS would buy a shorter latency for a load that is not on the
// dependent chain, at the price of a staging pass per wave.  A walker whose walk has ended (or that raised a flag) holds
// cur = -1, reads nothing and still writes its -1 into the tile: the flush stays one full-width pass.
__global__ __launch_bounds__(kWalkBlock) void metapath_walk_kernel(wk::TypedGraph g, const int32_t *__restrict__ node_type,
                                                                   const int64_t *__restrict__ start,
                                                                   const int32_t *__restrict__ walker_path, int64_t n_walkers,
                                                                   int64_t length, const int32_t *__restrict__ pattern,
                                                                   const int32_t *__restrict__ path_off, int32_t n_paths,
                                                                   uint64_t seed, int64_t *__restrict__ walks,
                                                                   int32_t *__restrict__ lengths, int *__restrict__ flags) {
    __shared__ int64_t lds[kWalkBlock / kWave][kWave][kWalkTile + 1];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int64_t(*stage)[kWalkTile + 1] = lds[wave];
    const int64_t wave_base = ((int64_t)blockIdx.x * (kWalkBlock / kWave) + wave) * kWave;
    const int64_t w = wave_base + lane;
    int64_t first = -1, cur = -1;
    int err = -1;  // no walker: parked from the start, nothing raised
    int32_t n_held = 0, t_next = 0;
    wk::PathCursor pc = {pattern, 1, 0};
    if (w < n_walkers) {
        err = 0;
        first = start[w];
        pc = wk::metapath_begin(g, node_type, first, walker_path[w], pattern, path_off, n_paths, err);
        n_held = 1;
        if (err == 0) {
            cur = first;
            t_next = wk::metapath_next_type(pc);  // the type wanted at position 1
        }
    }
    for (int64_t tile0 = 0; tile0 < length; tile0 += kWalkTile) {
        const int ncols = (int)(length - tile0 < kWalkTile ? length - tile0 : kWalkTile);
        for (int s = 0; s < ncols; ++s) {
            const int64_t i = tile0 + s;
            if (i > 0) {
                if (err == 0 && cur >= 0) {
                    const int32_t t = t_next;
                    t_next = wk::metapath_next_type(pc);
                    cur = wk::step_metapath(g, t, seed, w, i, cur, err);
                    n_held += cur >= 0 ? 1 : 0;
                } else {
                    cur = -1;
                }
            }
            stage[lane][s] = i == 0 ? first : cur;
        }
        wave_lds_sync();
        walk_flush(stage, lane, wave_base, n_walkers, length, tile0, ncols, walks);
        wave_lds_sync();
    }
    if (lengths && w < n_walkers) lengths[w] = n_held;
    walk_raise(flags, err > 0 ? err : 0);
}

static int walk_args_status(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                            const int64_t *start, int64_t n_walkers, int64_t length, const int64_t *walks, const int *flags) {
    if (num_nodes < 0 || num_edges < 0 || n_walkers < 0 || length < 1 || !flags) return COGDL_HIP_EINVAL;
    if (n_walkers > 0 && (!indptr || !start || !walks)) return COGDL_HIP_EINVAL;
    if (num_edges > 0 && !indices) return COGDL_HIP_EINVAL;
    if (length > 0x7fffffff) return COGDL_HIP_ERANGE;  // (the step index is one 32-bit word of the Philox counter)
    if (n_walkers > (int64_t)0x7fffffff * kWave) return COGDL_HIP_ERANGE;
    return COGDL_HIP_OK;
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_random_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                     const int64_t *start, int64_t n_walkers, int64_t length, double restart_p,
                                     uint64_t seed, int64_t *walks, int *flags, void *stream) {
    const int rc = walk_args_status(indptr, indices, num_nodes, num_edges, start, n_walkers, length, walks, flags);
    if (rc != COGDL_HIP_OK) return rc;
    if (!(restart_p >= 0.0 && restart_p <= 1.0)) return COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = fill_u32_async(flags, 0u, 1, s);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return COGDL_HIP_ELAUNCH;
    }
    if (n_walkers == 0) return COGDL_HIP_OK;
    const wk::Graph g = {indptr, indices, num_nodes, num_edges};
    const uint64_t restart_t = wk::fixed32(restart_p);
    hipLaunchKernelGGL(random_walk_kernel, dim3((unsigned)((n_walkers + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, s, g,
                       start, n_walkers, length, restart_t, seed, walks, flags);
    return launch_status();
}

extern "C" int cogdl_hip_node2vec_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                       const int64_t *start, int64_t n_walkers, int64_t length, double p, double q,
                                       int max_trials, uint64_t seed, int64_t *walks, int32_t *fallback_steps, int *flags,
                                       void *stream) {
    const int rc = walk_args_status(indptr, indices, num_nodes, num_edges, start, n_walkers, length, walks, flags);
    if (rc != COGDL_HIP_OK) return rc;
    if (!(p > 0.0) || !(q > 0.0) || !(p < 1e300) || !(q < 1e300) || max_trials < 0 || max_trials > (1 << 20)) return COGDL_HIP_EINVAL;
    if (max_trials == 0) max_trials = wk::kDefaultTrials;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = fill_u32_async(flags, 0u, 1, s);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return COGDL_HIP_ELAUNCH;
    }
    if (n_walkers == 0) return COGDL_HIP_OK;
    const wk::Graph g = {indptr, indices, num_nodes, num_edges};
    hipLaunchKernelGGL(node2vec_walk_kernel, dim3((unsigned)((n_walkers + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, s, g,
                       start, n_walkers, length, wk::n2v_weights(p, q), max_trials, seed, walks, fallback_steps, flags);
    return launch_status();
}

extern "C" int cogdl_hip_metapath_walk(const int64_t *seg, const int64_t *indices_t, int64_t num_nodes, int32_t num_types,
                                       int64_t num_edges, const int32_t *node_type, const int64_t *start,
                                       const int32_t *walker_path, int64_t n_walkers, int64_t length, const int32_t *pattern,
                                       const int32_t *path_off, int32_t n_paths, uint64_t seed, int64_t *walks,
                                       int32_t *lengths, int *flags, void *stream) {
    const int rc = walk_args_status(seg, indices_t, num_nodes, num_edges, start, n_walkers, length, walks, flags);
    if (rc != COGDL_HIP_OK) return rc;
    if (num_types < 1 || num_types > 64 || n_paths < 1) return COGDL_HIP_EINVAL;
    if (n_walkers > 0 && (!walker_path || !pattern || !path_off)) return COGDL_HIP_EINVAL;
    if (num_nodes > ((int64_t)1 << 56)) return COGDL_HIP_ERANGE;  // (cur * num_types stays a 64-bit offset)
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = fill_u32_async(flags, 0u, 1, s);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return COGDL_HIP_ELAUNCH;
    }
    if (n_walkers == 0) return COGDL_HIP_OK;
    const wk::TypedGraph g = {seg, indices_t, num_nodes, num_edges, num_types};
    hipLaunchKernelGGL(metapath_walk_kernel, dim3((unsigned)((n_walkers + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, s, g,
                       node_type, start, walker_path, n_walkers, length, pattern, path_off, n_paths, seed, walks, lengths, flags);
    return launch_status();
}
