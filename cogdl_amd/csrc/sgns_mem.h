// sgns_mem.h -- the memory helpers of the embedding trainers (sgns.hip, pvdbow.hip): how a wave reads and updates a table
// row that other waves, on other XCDs, update at the same time.  The rules are spelled out in sgns.hip ("Coherence").
#pragma once
#include "common.h"

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

}  // namespace cogdl
