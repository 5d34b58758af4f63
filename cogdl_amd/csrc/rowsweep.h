// rowsweep.h -- csr_spmm over a SWEEP layout: every wave owns a group of consecutive rows and walks the edges of ALL of them
// merged in an order in which the gathered row (almost) only ascends.
//
// Why.  The fp32 F = 128 launch of the arxiv-sized graph gathers 512-byte rows of an 87 MB table uniformly at random: an XCD's
// 4 MiB L2 holds 4.6 % of it, the launch runs at the fabric rate.  When every wave of the chip walks the table top to bottom
// at about the same pace, all waves of an XCD gather from the same few MB of it at any moment, and a row wanted by several
// edges of the XCD's rows is fetched across the fabric once.  Nothing enforces the pace -- no wave waits for another, there is
// no atomic and no flag: correctness never depends on it, only the hit rate does.
//
// What stays the same.  The merged walk is a STABLE sort of a group's edges on a key that never decreases inside a row, so it
// visits the edges of each row in exactly the row's own order: acc = acc + w * x, separately rounded (-ffp-contract=off),
// bit-identical to rowreduce_main_kernel<SpmmOp<float, 2, 64, 8, ...>> on the same structure.  Backward: the rows of a stable
// transpose list their gathered rows ascending, the key is the gathered row itself.  Forward: the caller's rows need not be
// column-sorted; the key is the running maximum of the column inside the row (cogdl_amd/sweepplan.py: build_forward) -- an
// edge behind its row's running maximum is walked where that maximum is, i.e. gathered out of table order: it costs hit rate
// (the policy asks for few of them), never bits.
//
// Guarded launches (rowreduce_sweep_guarded_kernel, cogdl_hip_csr_spmm_sweep_guarded).  The forward's layout belongs to a
// structure seen EARLIER; whether the call at hand passes that structure is known to the device only (the call's hash is
// still in flight to the host).  The guarded kernel compares the hash the stream has just computed with the layout's key in
// every wave's prologue (common.h: HashGuard) and walks the layout on a match; otherwise it leaves at once and the ordinary
// launch, guarded the other way round, does the work.  The walk itself is the same code.
//
// Layout (cogdl_amd/sweepplan.py), group g = rows [g * r, min((g + 1) * r, m)), r <= kSweepRows:
//   goff [n_groups + 1]   edge offsets of the groups
//   src  [nnz]            per edge: gathered row (low 24 bits) | local row inside the group (high 8 bits)
//   w    [nnz]            edge weights in layout order, or NULL
// The states of a group stay on the chip for the whole walk: registers for 32 rows (2 VGPRs per row at F = 128 fp32), LDS for 16.
#pragma once
#include "common.h"

namespace cogdl {

constexpr int kSweepRows = 48;       // rows per wave (32 in registers, 16 in LDS); 4 waves per SIMD
constexpr int kSweepWavesPerCu = 16;
constexpr int kSweepUnroll = 8;

struct SweepArgs {
    const int32_t *goff;
    const uint32_t *src;
    const float *w;
    const float *x;
    float *out;
    int64_t m, n_groups;
    int r;          // rows per group (<= kSweepRows)
    uint32_t row_bytes;
};

typedef float SweepF32x32 __attribute__((ext_vector_type(32)));
constexpr int kSweepRegRows = 32;                          // rows whose state is a pair of 32-register tuples ...
constexpr int kSweepLdsRows = kSweepRows - kSweepRegRows;  // ... and the rest: 8 bytes per lane and row in LDS (8 KB per wave)

// The states of a wave's kSweepRows rows, two columns per lane.  The local row of an edge is wave-uniform: rows 0..31 live in
// two register tuples and are picked with an indexed register move, rows 32..47 in the wave's own LDS slab (every lane reads
// and writes only its own words: no barrier).  (A dynamically indexed ARRAY goes to scratch memory; a `switch` over constant
// indices in an unrolled batch, and a third register tuple, each made the register allocator spill.)
// Fold one gathered row into the state of local row `lr`.  Unconditional: a slot past the chunk's end comes with w = 0 and
// v = 0, and acc + 0 * 0 == acc exactly (acc is never -0).
template <bool WEIGHTED>
__device__ __forceinline__ void sweep_fold(SweepF32x32 &lo0, SweepF32x32 &lo1, float2 *hi, int lr, float w, float2 v) {
    if (lr < kSweepRegRows) {
        const float s0 = lo0[lr], s1 = lo1[lr];
        lo0[lr] = WEIGHTED ? s0 + w * v.x : s0 + v.x;
        lo1[lr] = WEIGHTED ? s1 + w * v.y : s1 + v.y;
    } else {
        float2 *p = hi + (lr - kSweepRegRows) * kWave;
        const float2 s = *p;
        *p = WEIGHTED ? make_float2(s.x + w * v.x, s.y + w * v.y) : make_float2(s.x + v.x, s.y + v.y);
    }
}

// One wave per row group, four waves per workgroup; groups beyond one round of the grid are walked by the same waves,
// grid-stride (correct, only less local).  Rows of 128 fp32 columns: one float2 per lane.
// (The body of both kernels below: the unguarded one is this and nothing else.)
template <bool WEIGHTED>
__device__ __forceinline__ void sweep_walk(const SweepArgs &a) {
    constexpr int UNROLL = kSweepUnroll;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t lane_off = (uint32_t)lane * (uint32_t)sizeof(float2);
    const char *const table = reinterpret_cast<const char *>(a.x);
    __shared__ float2 slab[4][kSweepLdsRows][kWave];
    float2 *const hi = &slab[threadIdx.x >> 6][0][lane];
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t g = wave0; g < a.n_groups; g += n_waves) {  // (a wave past the last group exits)
        SweepF32x32 lo0 = 0.f, lo1 = 0.f;
#pragma unroll
        for (int c = 0; c < kSweepLdsRows; ++c) hi[c * kWave] = make_float2(0.f, 0.f);
        const int start = __builtin_amdgcn_readfirstlane(a.goff[g]);
        const int end = __builtin_amdgcn_readfirstlane(a.goff[g + 1]);
        if (start < end) {
            const int last = end - 1;
            // The next chunk's words are requested before the current chunk's gathers; the loads are unconditional (index
            // clamped into the group's range: a load inside a per-lane branch parks the wave at the join).
            uint32_t my_p = a.src[min(start + lane, last)];
            float my_w = 1.f;
            if constexpr (WEIGHTED) my_w = a.w[min(start + lane, last)];
            for (int base = start; base < end; base += kWave) {
                const int cnt = min(kWave, end - base);
                const int nidx = min(base + kWave + lane, last);
                const uint32_t next_p = a.src[nidx];
                float next_w = 1.f;
                if constexpr (WEIGHTED) next_w = a.w[nidx];
                for (int j = 0; j < cnt; j += UNROLL) {
                    float2 v[UNROLL];
                    float w[UNROLL];
                    int lr[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {  // (a slot past the chunk's end re-reads the chunk's last row: an L1 hit)
                        const int jj = min(j + u, cnt - 1);
                        const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)my_p, jj);
                        w[u] = WEIGHTED ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), jj)) : 1.f;
                        lr[u] = (int)(p >> 24);
                        // (tables of < 2^24 rows and < 4 GiB: a 32-bit byte offset on the table's uniform base)
                        const uint32_t off = (p & 0xffffffu) * a.row_bytes + lane_off;
                        v[u] = *reinterpret_cast<const float2 *>(table + off);
                    }
                    // (all UNROLL gathers are in flight before the first fold: without this the compiler sinks seven of them
                    //  behind the first fold's branch -- DESIGN section 5, lesson 5)
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const bool valid = j + u < cnt;
                        sweep_fold<WEIGHTED>(lo0, lo1, hi, lr[u], valid ? w[u] : 0.f, valid ? v[u] : make_float2(0.f, 0.f));
                    }
                }
                my_p = next_p;
                my_w = next_w;
            }
        }
        // (rows of a partial last group that do not exist are never stored)
        const int64_t row0 = g * a.r;
        const int n_rows = __builtin_amdgcn_readfirstlane((int)min((int64_t)a.r, a.m - row0));
        char *dst = reinterpret_cast<char *>(a.out) + (uint64_t)row0 * (uint64_t)a.row_bytes + lane_off;
#pragma unroll
        for (int c = 0; c < kSweepRows; ++c) {
            if (c < n_rows) {
                const float2 o = c < kSweepRegRows ? make_float2(lo0[c & 31], lo1[c & 31]) : hi[(c & 15) * kWave];
                *reinterpret_cast<float2 *>(dst + (uint64_t)c * (uint64_t)a.row_bytes) = o;
            }
        }
    }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256, 4) void rowreduce_sweep_kernel(const SweepArgs a) {
    sweep_walk<WEIGHTED>(a);
}

// The same walk, taken only if the guard says so (see the header comment); a wave that stands down has written nothing.
template <bool WEIGHTED>
__global__ __launch_bounds__(256, 4) void rowreduce_sweep_guarded_kernel(const SweepArgs a, const HashGuard guard) {
    if (!guard_runs(guard)) return;
    sweep_walk<WEIGHTED>(a);
}

// Waves of one round on the current device (CU count x waves that fit), capped by tuning key 18 (tests: rows per round).
inline int64_t sweep_round_waves() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
        cus[dev] = n;
    }
    int64_t waves = (int64_t)cus[dev] * kSweepWavesPerCu;
    if (g_tuning[kTuneSweepRows] > 0) waves = std::max<int64_t>(1, std::min<int64_t>(waves, g_tuning[kTuneSweepRows] / kSweepRows));
    return waves;
}

}  // namespace cogdl
