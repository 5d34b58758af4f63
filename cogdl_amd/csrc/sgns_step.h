// sgns_step.h -- the wave-level step of the embedding trainers (sgns.hip, pvdbow.hip, line.hip): score an input row against
// a target row (wave_dot), accumulate the input row's gradient and update the target row, on table rows that other waves, on other
// XCDs, update at the same time.  Lane l owns the elements d = l, l + 64, .. of every row (KD = 1, 2, 4 or 8 per lane); a
// row pointer handed to these helpers already points at the lane's first element.  The law of the step is sgns_law.h's; the
// host twins run it through sgns_host.h.
//
// Coherence.  The eight XCDs' L2s are not coherent with each other and a CU's vector L1 is refreshed by nobody, so:
//   * every load of a table row is an agent-scope atomic load (global_load ... sc1): it bypasses L1, where a line this wave
//     updated a moment ago (skip-gram re-reads the input row for ~2 * window consecutive centres) would still be the old one;
//   * a row update is a no-return atomicAdd(float) (STORES = false, the default: executed at the memory side, no add is
//     ever lost whichever XCDs the adders sit on, the line leaves this XCD's L2) or, for skip-gram and PV-DBOW under tuning
//     key 17, an agent-scope atomic store of (loaded + delta) (STORES = true: a write-through store; concurrent writers of
//     one row overwrite each other as in CPU Hogwild).  In the serial mode both are the law's rounded product plus rounded
//     sum.  profiles/sgns_bench.txt has the two measured against each other;
//   * the wave waits for its own updates (s_waitcnt vmcnt(0)) before it re-reads a row it has already updated: a repeated
//     target inside one pair / position / sample (here and in line.hip), and at the end of every pair or position, or sample
//     of the serial mode (the kernels), so its own earlier updates are in memory before the re-read is issued;
//   * what ANOTHER XCD added to a row can stay invisible here for as long as this XCD's L2 keeps its copy, at most until
//     the launch ends: the kernel boundary bounds the staleness, which is why the throughput modes go in launches of a
//     bounded number of rows / documents / samples and not in one persistent grid.
#pragma once
#include <type_traits>

#include "common.h"
#include "sgns_law.h"

namespace cogdl {

// agent-scope atomic load: bypasses the CU's vector L1, where a line this wave updated a moment ago would still be the old one
__device__ __forceinline__ float row_load(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// STORES = false: a no-return atomicAdd(float), executed at the memory side; true: a write-through store of (loaded + delta)
template <bool STORES>
__device__ __forceinline__ void row_add(float *p, float old, float delta) {
    if constexpr (STORES) __hip_atomic_store(p, old + delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else atomicAdd(p, delta);
}

// every vector memory operation of this wave has completed (vmcnt(0); expcnt and lgkmcnt left alone)
__device__ __forceinline__ void wait_own_updates() { __builtin_amdgcn_s_waitcnt(0x0F70); }

__device__ __forceinline__ float uniform_f32(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// The sigmoid table into LDS (all threads of the workgroup call this, first thing).  False: the validation pass that ran
// before in the stream found bad input, and the kernel returns without touching the tables.
__device__ __forceinline__ bool stage_exp_table(float *exp_lds, const float *exp_table, const int *flags) {
    for (int k = threadIdx.x; k < cogdl_sgns::kExpTable; k += blockDim.x) exp_lds[k] = exp_table[k];
    __syncthreads();
    return *(const volatile int *)flags == 0;
}

template <int KD>
__device__ __forceinline__ void load_row(float (&r)[KD], const float *row, int lane, int D) {
#pragma unroll
    for (int q = 0; q < KD; ++q) r[q] = lane + q * kWave < D ? row_load(row + q * kWave) : 0.0f;
}

// sgns_law.h's dot product: the lane's sum in ascending q, then the butterfly of width B; the same value in every lane
template <int KD>
__device__ __forceinline__ float wave_dot(const float (&x)[KD], const float (&y)[KD], int lane, int D, int B) {
    float p = 0.0f;
#pragma unroll
    for (int q = 0; q < KD; ++q)
        if (lane + q * kWave < D) p = p + x[q] * y[q];
#pragma unroll
    for (int sft = kWave / 2; sft > 0; sft >>= 1)
        if (sft < B) p = p + __shfl_xor(p, sft, kWave);
    return uniform_f32(p);
}

// One target, scored f = wave_dot(x, y): where Rule applies, acc += g * y (the row as loaded) and the target row += g * x.
// (f is the caller's to compute: with the dot product in here, line.hip's prefetch kernel goes from 110 registers to 128
// and 76 bytes of scratch under its four-wave bound.)
template <int KD, class Rule, bool STORES>
__device__ __forceinline__ void update_target(float f, const float (&x)[KD], const float (&y)[KD], float *yrow, float (&acc)[KD],
                                              float label, float lr, const float *exp_lds, int lane, int D) {
    if (!Rule::applies(f)) return;
    const float g = Rule::gradient(f, label, lr, exp_lds);
#pragma unroll
    for (int q = 0; q < KD; ++q)
        if (lane + q * kWave < D) {
            acc[q] = acc[q] + g * y[q];
            row_add<STORES>(yrow + q * kWave, y[q], g * x[q]);
        }
}

// The targets of one input row, held in lanes 0..K of `tl` (target 0 has label 1; -1: skipped), taken in order against
// rows of `table`.  A target this call has already updated is read again after that update has completed.
template <int KD, class Rule, bool STORES>
__device__ __forceinline__ void update_lane_targets(int32_t tl, int K, const float (&x)[KD], float (&acc)[KD], float *table, float lr,
                                                    const float *exp_lds, int lane, int D, int B) {
    for (int k = 0; k <= K; ++k) {
        const int32_t t = __builtin_amdgcn_readlane(tl, k);
        if (t < 0) continue;
        if (__any(lane < k && tl == t)) wait_own_updates();
        float *yrow = table + (int64_t)t * D + lane;
        float y[KD];
        load_row<KD>(y, yrow, lane, D);
        update_target<KD, Rule, STORES>(wave_dot<KD>(x, y, lane, D, B), x, y, yrow, acc, k == 0 ? 1.0f : 0.0f, lr, exp_lds, lane, D);
    }
}

// ---- host side of the three launchers

// The kernel instantiation of a launch: D -> the elements per lane KD in {1, 2, 4, 8}, and the trainer's one run-time switch
// (the row-update variant, or LINE's ordered mode), as launch(std::integral_constant<int, KD>, std::bool_constant<flag>).
template <class Launch>
static void with_row_width(int D, bool flag, Launch &&launch) {
    const auto with_flag = [&](auto kd) {
        if (flag) launch(kd, std::true_type());
        else launch(kd, std::false_type());
    };
    if (D <= 64) with_flag(std::integral_constant<int, 1>());
    else if (D <= 128) with_flag(std::integral_constant<int, 2>());
    else if (D <= 256) with_flag(std::integral_constant<int, 4>());
    else with_flag(std::integral_constant<int, 8>());
}

// The throughput mode's launches: items [0, n) in order, at most `chunk` per launch(first, count); stops at a failed launch.
template <class Launch>
static int launch_chunks(int64_t n, int64_t chunk, Launch &&launch) {
    for (int64_t first = 0; first < n; first += chunk) {
        launch(first, std::min<int64_t>(chunk, n - first));
        const int st = launch_status();
        if (st != COGDL_HIP_OK) return st;
    }
    return COGDL_HIP_OK;
}

}  // namespace cogdl
