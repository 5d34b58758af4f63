// walk.hip -- random walks on a GPU-resident CSR graph (int64 indptr / indices) for gfx950:
//   cogdl_hip_random_walk     first-order walk with restart  (the contract of cogdl/utils/sampling.py:46-67)
//   cogdl_hip_node2vec_walk   second-order walk with return parameter p and in-out parameter q, unweighted
//                             (the transition weights of cogdl/models/emb/node2vec.py:143-156)
//   cogdl_hip_metapath_walk   walk that follows a node-type schema on the typed row layout (metapath2vec.py:87-106)
// What a walk kind IS -- its draws, its step, what a walker carries, counts and stores -- is a rule of walk_draw.h, which the
// host twin (host_ops.cpp) runs too: for equal inputs and seed both return the same array.  This file is the scaffold that
// runs a rule on the GPU, written once: walk_kernel<Rule>, launch_walk<Rule>, and three entry points that check their own
// parameters and build their rule.
//
// Shape.  A step is two dependent random loads (the indptr pair, one indices entry) and a handful of integer
// instructions: the kernel is bound by memory latency, so throughput is walkers in flight.  One lane owns one walker (50
// VGPRs, 18 KiB of LDS per workgroup: 8 waves per SIMD; two walkers per lane were measured and were slower).
// Writing walks[w, i] straight from the lanes would make every store instruction touch 64 cache lines 8 L bytes apart
// (measured: 1.7x to 2x slower), so a wave stages kWalkTile steps of its walkers in LDS (rows padded by one entry against
// bank conflicts) and then writes each walker's kWalkTile consecutive steps as one contiguous 64-byte piece, 8 walkers
// per store instruction.  Tiles start at columns that are multiples of kWalkTile, so the pieces are 64-byte aligned whenever
// L is a multiple of 8.  The LDS region is private to a wave (no workgroup barrier: waves of a workgroup drift freely, which
// is what hides the latency).
// Error flags are raised with raise_flags (common.h): a plain read-or-write of the flags word, no atomics.
#include "common.h"

#include "walk_draw.h"

namespace cogdl {

namespace wk = cogdl_walk;

constexpr int kWalkTile = 8;    // steps staged per walker: 64-byte pieces
constexpr int kWalkBlock = 256;

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

// A lane without a walker is parked from the start (err = -1): it reads nothing, raises nothing and still takes part in the
// flush, which stays one full-width pass.  A walker whose err is up reads nothing more (the step functions see to that).
template <class Rule>
__global__ __launch_bounds__(kWalkBlock) void walk_kernel(Rule rule, int64_t n_walkers, int64_t length, uint64_t seed,
                                                          int64_t *__restrict__ walks, int *__restrict__ flags) {
    __shared__ int64_t lds[kWalkBlock / kWave][kWave][kWalkTile + 1];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int64_t(*stage)[kWalkTile + 1] = lds[wave];
    const int64_t wave_base = ((int64_t)blockIdx.x * (kWalkBlock / kWave) + wave) * kWave;
    const int64_t w = wave_base + lane;
    typename Rule::State st = {};
    int64_t at = 0;
    int err = -1;
    if (w < n_walkers) {
        err = 0;
        at = rule.begin(st, w, err);
    }
    for (int64_t tile0 = 0; tile0 < length; tile0 += kWalkTile) {
        const int ncols = (int)(length - tile0 < kWalkTile ? length - tile0 : kWalkTile);
        for (int s = 0; s < ncols; ++s) {
            const int64_t i = tile0 + s;
            if (i > 0) at = rule.advance(st, seed, w, i, err);
            stage[lane][s] = at;
        }
        wave_lds_sync();
        walk_flush(stage, lane, wave_base, n_walkers, length, tile0, ncols, walks);
        wave_lds_sync();
    }
    if (w < n_walkers) rule.finish(st, w);
    raise_flags(flags, err > 0 ? err : 0);
}

static int walk_args_rc(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges, const int64_t *start,
                        int64_t n_walkers, int64_t length, const int64_t *walks, const int *flags) {
    const int rc = wk::walk_args_status(indptr, indices, num_nodes, num_edges, start, n_walkers, length, walks, flags,
                                        (int64_t)0x7fffffff * kWave);
    return rc == wk::kArgsOk ? COGDL_HIP_OK : rc == wk::kArgsRange ? COGDL_HIP_ERANGE : COGDL_HIP_EINVAL;
}

template <class Rule>
static int launch_walk(const Rule &rule, int64_t n_walkers, int64_t length, uint64_t seed, int64_t *walks, int *flags, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const int rc = clear_flags_async(flags, s);
    if (rc != COGDL_HIP_OK || n_walkers == 0) return rc;
    hipLaunchKernelGGL(walk_kernel<Rule>, dim3((unsigned)((n_walkers + kWalkBlock - 1) / kWalkBlock)), dim3(kWalkBlock), 0, s, rule,
                       n_walkers, length, seed, walks, flags);
    return launch_status();
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_random_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                     const int64_t *start, int64_t n_walkers, int64_t length, double restart_p,
                                     uint64_t seed, int64_t *walks, int *flags, void *stream) {
    const int rc = walk_args_rc(indptr, indices, num_nodes, num_edges, start, n_walkers, length, walks, flags);
    if (rc != COGDL_HIP_OK) return rc;
    if (!(restart_p >= 0.0 && restart_p <= 1.0)) return COGDL_HIP_EINVAL;
    const wk::FirstOrderRule rule = {{indptr, indices, num_nodes, num_edges}, start, wk::fixed32(restart_p)};
    return launch_walk(rule, n_walkers, length, seed, walks, flags, stream);
}

extern "C" int cogdl_hip_node2vec_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                       const int64_t *start, int64_t n_walkers, int64_t length, double p, double q,
                                       int max_trials, uint64_t seed, int64_t *walks, int32_t *fallback_steps, int *flags,
                                       void *stream) {
    const int rc = walk_args_rc(indptr, indices, num_nodes, num_edges, start, n_walkers, length, walks, flags);
    if (rc != COGDL_HIP_OK) return rc;
    if (!(p > 0.0) || !(q > 0.0) || !(p < 1e300) || !(q < 1e300) || max_trials < 0 || max_trials > (1 << 20)) return COGDL_HIP_EINVAL;
    const wk::Node2vecRule rule = {{indptr, indices, num_nodes, num_edges}, start, wk::n2v_weights(p, q),
                                   max_trials == 0 ? wk::kDefaultTrials : max_trials, fallback_steps};
    return launch_walk(rule, n_walkers, length, seed, walks, flags, stream);
}

extern "C" int cogdl_hip_metapath_walk(const int64_t *seg, const int64_t *indices_t, int64_t num_nodes, int32_t num_types,
                                       int64_t num_edges, const int32_t *node_type, const int64_t *start,
                                       const int32_t *walker_path, int64_t n_walkers, int64_t length, const int32_t *pattern,
                                       const int32_t *path_off, int32_t n_paths, uint64_t seed, int64_t *walks,
                                       int32_t *lengths, int *flags, void *stream) {
    const int rc = walk_args_rc(seg, indices_t, num_nodes, num_edges, start, n_walkers, length, walks, flags);
    if (rc != COGDL_HIP_OK) return rc;
    if (num_types < 1 || num_types > 64 || n_paths < 1) return COGDL_HIP_EINVAL;
    if (n_walkers > 0 && (!walker_path || !pattern || !path_off)) return COGDL_HIP_EINVAL;
    if (num_nodes > ((int64_t)1 << 56)) return COGDL_HIP_ERANGE;  // (cur * num_types stays a 64-bit offset)
    const wk::MetapathRule rule = {{seg, indices_t, num_nodes, num_edges, num_types}, node_type, start, walker_path, pattern,
                                   path_off, n_paths, lengths};
    return launch_walk(rule, n_walkers, length, seed, walks, flags, stream);
}
