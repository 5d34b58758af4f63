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
//
// The gather ring (sweep_walk).  A wave keeps kSweepRing gathers in flight at every moment of a group's walk: a prologue
// requests the first kSweepRing rows; then edge i waits for its slot (i % kSweepRing) with `s_waitcnt vmcnt(kSweepRing - 1)`
// -- the counter retires loads in order, so that leaves exactly the younger gathers outstanding --, is folded, and edge
// i + kSweepRing is requested into the register pair the fold has just freed.  Requests past the group's end name its last
// edge again (an L1 hit, never folded: a wave-uniform branch skips the slot); the ring is drained once per group.
// hipcc cannot be left to count this: its wait insertion falls back to vmcnt(0..2) at every loop header, which empties the ring
// once per batch.  So the gathers, the loads of the layout words and every wait on them are `asm volatile` statements the
// compiler does not see as memory operations; what it must not do with a register in flight is said through operands: a
// slot is an output of its request, an in/out operand of its wait (no read moves above it), and every slot and the words on
// their way are operands of the drain (no register is reused under a load that has not landed).  After every compiler or
// flag change look at the ISA: no instruction may touch a slot between its request and its wait (profiles/sweep_pipeline.txt).
// The layout words of 64 edges sit in one VGPR each; the next 64 are requested, on the same counter, right after the batch
// that took the current ones up, and are long retired (64 edges of counted waits) when their turn comes.  With them behind
// the ring a wait retires up to three gathers instead of one for kSweepRing edges: once in 64.
// Depth.  More in flight is NOT better here: every gather in flight holds a line of the XCD's L2 that the walk wants for
// rows other waves are about to ask for.  512 waves x 8 rows x 512 bytes are 2 of an XCD's 4 MiB: at depth 8 the launch's L2 hit
// rate falls from 0.30 to 0.21 and the launch is 12 % SLOWER than the batches of 8 it replaced (which drained to nothing while
// folding: 4 in flight on average); depth 2 is latency-bound (+7 %); depth 4 keeps the hit rate and is the fastest measured.
#pragma once
#include "common.h"

namespace cogdl {

constexpr int kSweepRows = 48;       // rows per wave (32 in registers, 16 in LDS); 4 waves per SIMD
constexpr int kSweepWavesPerCu = 16;
constexpr int kSweepUnroll = 8;      // edges per unrolled batch (one v_readlane pass over the words at hand)
constexpr int kSweepRing = 4;        // gathers a wave keeps in flight (measured: 2, 4, 8 -- see the header comment)

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
// Fold one gathered row into the state of local row `lr`.
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

// One gather of the ring: the 512-byte row at byte offset `off` (+ the lane's own 8 bytes) of the table, requested into `slot`.
// The compiler takes `slot` for written when this returns; it is not, until sweep_wait has named it.
typedef float SweepF32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void sweep_request(SweepF32x2 &slot, uint32_t off, const char *table) {
    asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(slot) : "v"(off), "s"(table));
}
// Wait for the oldest gather of the ring and leave the kSweepRing - 1 younger ones in flight.  `slot` is an operand so that
// no read of it can be moved above the wait.
__device__ __forceinline__ void sweep_wait(SweepF32x2 &slot) {
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(slot) : "n"(kSweepRing - 1));
}
// Drain the ring.  Every slot and the words on their way are operands: the over-run loads still write their registers until here.
__device__ __forceinline__ void sweep_drain(SweepF32x2 (&v)[kSweepRing], uint32_t &np, float &nw) {
    static_assert(kSweepRing == 4, "one operand per slot");
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(np), "+v"(nw));
}

// The layout words of edge `i` (per lane), requested like a gather: the same counter, the same hand-kept count.
template <bool WEIGHTED>
__device__ __forceinline__ void sweep_words(uint32_t &p, float &w, const uint32_t *src, const float *wgt, int i) {
    asm volatile("global_load_dword %0, %1, off" : "=v"(p) : "v"(src + i));
    if constexpr (WEIGHTED) asm volatile("global_load_dword %0, %1, off" : "=v"(w) : "v"(wgt + i));
}
// The first words of a group, before its ring starts: everything but the one or two loads behind them has landed.
template <bool WEIGHTED>
__device__ __forceinline__ void sweep_words_landed(uint32_t &p, float &w) {
    if constexpr (WEIGHTED) asm volatile("s_waitcnt vmcnt(2)" : "+v"(p), "+v"(w));
    else asm volatile("s_waitcnt vmcnt(1)" : "+v"(p));
}
// Take up the next words.  An operand of a statement of its own, so that no read of them moves above the waits before it.
__device__ __forceinline__ void sweep_words_turn(uint32_t &p, float &w, uint32_t &np, float &nw) {
    asm volatile("" : "+v"(np), "+v"(nw));
    p = np;
    w = nw;
}

// One wave per row group, four waves per workgroup; groups beyond one round of the grid are walked by the same waves,
// grid-stride (correct, only less local).  Rows of 128 fp32 columns: one float2 per lane.
// (The body of both kernels below: the unguarded one is this and nothing else.)
template <bool WEIGHTED>
__device__ __forceinline__ void sweep_walk(const SweepArgs &a) {
    constexpr int UNROLL = kSweepUnroll;
    static_assert(UNROLL % kSweepRing == 0 && kWave % UNROLL == 0, "a slot is an edge's place in its batch, a batch never straddles the words at hand");
    typedef const __attribute__((address_space(4))) int32_t *ConstI32;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t lane_off = (uint32_t)lane * (uint32_t)sizeof(float2);
    const char *const table = reinterpret_cast<const char *>(a.x);
    // (the group offsets are read-only for the launch and their index is wave-uniform: scalar loads, counted on lgkmcnt)
    const ConstI32 goff = (ConstI32)(uintptr_t)a.goff;
    __shared__ float2 slab[4][kSweepLdsRows][kWave];
    float2 *const hi = &slab[threadIdx.x >> 6][0][lane];
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t g = wave0; g < a.n_groups; g += n_waves) {  // (a wave past the last group exits)
        SweepF32x32 lo0 = 0.f, lo1 = 0.f;
#pragma unroll
        for (int c = 0; c < kSweepLdsRows; ++c) hi[c * kWave] = make_float2(0.f, 0.f);
        const int start = goff[g];
        const int end = goff[g + 1];
        if (start < end) {
            const int last = end - 1;
            // The layout words of 64 edges sit in one VGPR each, lane i = edge cbase + i (an index past the group's end is
            // clamped to its last edge: that row is requested again, an L1 hit, and never folded); the next 64 are on their way.
            // A batch reads its words out of them with v_readlane: p/w of the batch being folded, np/nw of the one being requested.
            uint32_t cp, ncp;
            float cw = 1.f, ncw = 1.f;
            sweep_words<WEIGHTED>(cp, cw, a.src, a.w, min(start + lane, last));
            sweep_words<WEIGHTED>(ncp, ncw, a.src, a.w, min(start + kWave + lane, last));
            sweep_words_landed<WEIGHTED>(cp, cw);
            int cbase = start;
            uint32_t p[UNROLL], np[UNROLL];
            float w[UNROLL], nw[UNROLL];
            SweepF32x2 v[kSweepRing];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                p[u] = (uint32_t)__builtin_amdgcn_readlane((int)cp, u);
                w[u] = WEIGHTED ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cw), u)) : 1.f;
            }
            // Prologue: the first kSweepRing gathers.
#pragma unroll
            for (int u = 0; u < kSweepRing; ++u) sweep_request(v[u], (p[u] & 0xffffffu) * a.row_bytes + lane_off, table);
            for (int e = start; e < end; e += UNROLL) {
                int k = e + UNROLL - cbase;  // the next batch's place in the words at hand
                const bool turn = k == kWave;
                if (turn) {  // (requested 64 edges ago: the counted waits since have retired them, in order)
                    sweep_words_turn(cp, cw, ncp, ncw);
                    cbase += kWave;
                    k = 0;
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    np[u] = (uint32_t)__builtin_amdgcn_readlane((int)cp, k + u);
                    nw[u] = WEIGHTED ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cw), k + u)) : 1.f;
                }
                // Steady state: edge i waits for slot i % kSweepRing alone, is folded, and edge i + kSweepRing is requested into
                // the slot the fold has just freed -- its words are further down this batch's or at the head of the next one's.
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    SweepF32x2 &slot = v[u % kSweepRing];
                    sweep_wait(slot);
                    // (wave-uniform: a slot past the group's end is skipped, not folded as 0 * 0)
                    if (e + u < end) sweep_fold<WEIGHTED>(lo0, lo1, hi, (int)(p[u] >> 24), w[u], make_float2(slot.x, slot.y));
                    const uint32_t rq = u + kSweepRing < UNROLL ? p[(u + kSweepRing) % UNROLL] : np[(u + kSweepRing) % UNROLL];
                    sweep_request(slot, (rq & 0xffffffu) * a.row_bytes + lane_off, table);
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    p[u] = np[u];
                    w[u] = nw[u];
                }
                // The words after those just taken up: two more loads behind the ring's.  The counted wait stays what it is, so
                // for the next kSweepRing edges a wait retires up to three gathers instead of one -- once in 64 edges.
                if (turn) sweep_words<WEIGHTED>(ncp, ncw, a.src, a.w, min(cbase + kWave + lane, last));
            }
            sweep_drain(v, ncp, ncw);
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
