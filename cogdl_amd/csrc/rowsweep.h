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
//   rows [n_groups * r]   optional (SweepArgs::rows, template argument MAPPED): the output row of local row l of group g at
//                         g * r + l, < 0 for a pad slot.  Then a group is ANY r rows.  Which rows share a wave decides where the
//                         waves are in the table at the same edge index: groups of consecutive rows differ by +-4 % in edges,
//                         which is more of the table than an XCD's L2 holds; cogdl_amd/sweepplan.py: deal_by_degree gives
//                         every wave the same number of edges and the same mean place in the table (measured on the
//                         benchmark's graph: L2 hit rate 0.345 -> 0.506, the backward launch 134 -> 105 us;
//                         profiles/sweep_groups.txt).  The map is read where a group's rows are stored, never per edge.
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
// flag change look at the ISA: no instruction may touch a slot between its request and its wait (profiles/sweep_issue.txt).
// The layout words of 64 edges sit in one VGPR each; the next 64 are requested, on the same counter, at the word turn (the
// place in a batch from which the requests belong to the next 64 edges), and are long retired (64 edges of counted waits)
// when their turn comes.  With them behind the ring a wait retires up to three gathers instead of one for kSweepRing edges:
// once in 64.
// The instruction stream.  The walk is bound by instruction issue, not by the fabric (profiles/sweep_issue.txt: the issue
// cycles of a SIMD's four waves add up to the launch's length, every instruction costs its wave about four cycles), so an
// edge is held to about 16 instructions (it was 32):
//   request    s_lshl (word << 9, the row's byte offset) + buffer_load with that scalar offset (sweep_request)
//   words      two v_readlane where the gather is requested; they stay in the SGPRs the slot's fold reads kSweepRing edges
//              later (a static rotation over the batch: no copies), + one s_add for the lane
//   row kind   s_cmp + s_cbranch, twice (register row / LDS row)
//   fold       one v_pk_mul, then s_lshr, s_set_gpr_idx_on, two v_add ON the indexed registers, s_set_gpr_idx_off (sweep_fold)
//   end test   none in a batch that lies inside the group; the group's last, partial batch runs a tested copy of the body
// Depth.  More in flight is NOT better here: every gather in flight holds a line of the XCD's L2 that the walk wants for
// rows other waves are about to ask for.  512 waves x 8 rows x 512 bytes are 2 of an XCD's 4 MiB: at depth 8 the launch's L2 hit
// rate falls from 0.30 to 0.21 and the launch is 12 % SLOWER than the batches of 8 it replaced (which drained to nothing while
// folding: 4 in flight on average); depth 2 is latency-bound (+7 %); depth 4 keeps the hit rate and is the fastest measured.
#pragma once
#include "common.h"

namespace cogdl {

constexpr int kSweepRows = 48;       // rows per wave (32 in registers, 16 in LDS); 4 waves per SIMD
constexpr int kSweepWavesPerCu = 16;
constexpr int kSweepUnroll = 8;      // edges per unrolled batch (the words of its edges rotate through 8 SGPR pairs)
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
    uint32_t table_bytes;  // the gathered table's size, for the descriptor's range check (0 for a table of 2^32 bytes: sweep_args)
    const int32_t *rows;   // [n_groups * r] the output row of local row l of group g at g * r + l (< 0: a pad slot, never
                           // written), or NULL: row g * r + l.  Read only where a group's rows are stored (MAPPED).
};

typedef float SweepF32x32 __attribute__((ext_vector_type(32)));
constexpr int kSweepRegRows = 32;                          // rows whose state is a pair of 32-register tuples ...
constexpr int kSweepLdsRows = kSweepRows - kSweepRegRows;  // ... and the rest: 8 bytes per lane and row in LDS (8 KB per wave)

// The states of a wave's kSweepRows rows, two columns per lane.  The local row of an edge is wave-uniform: rows 0..31 live in
// two register tuples and are picked with the register index mode, rows 32..47 in the wave's own LDS slab (every lane reads
// and writes only its own words: no barrier).  (A dynamically indexed ARRAY goes to scratch memory; a `switch` over constant
// indices in an unrolled batch, and a third register tuple, each made the register allocator spill.)
// Fold one gathered row into the state of local row `lr`.
// A register row is added to IN PLACE: both tuples sit on fixed registers (v[64:95], v[96:127]: the upper half of the kernel's
// 128) and one s_set_gpr_idx_on (SRC0 | DST) makes `v_add_f32 v64, v64, t` read and write v[64 + lr].  The index mode is on for
// these two instructions only, inside one statement; it goes through m0.  The product w * x is rounded by a v_mul of its own
// in front (-ffp-contract=off), the sum by the v_add: the same two roundings as `s + w * x`.
template <bool WEIGHTED>
__device__ __forceinline__ void sweep_fold(SweepF32x32 &lo0, SweepF32x32 &lo1, float2 *hi, uint32_t word, float w, float2 v) {
    // (two tests, not if / else: the compiler lays a wave-uniform if / else out through a mask in vcc, five instructions)
    const float t0 = WEIGHTED ? w * v.x : v.x, t1 = WEIGHTED ? w * v.y : v.y;
    if (word < ((uint32_t)kSweepRegRows << 24)) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // ("clobber list contains reserved registers: m0" -- it is written here)
        asm volatile("s_set_gpr_idx_on %2, gpr_idx(SRC0,DST)\n\t"
                     "v_add_f32_e32 v64, v64, %3\n\t"
                     "v_add_f32_e32 v96, v96, %4\n\t"
                     "s_set_gpr_idx_off"
                     : "+{v[64:95]}"(lo0), "+{v[96:127]}"(lo1)
                     : "s"(word >> 24), "v"(t0), "v"(t1)
                     : "m0");
#pragma clang diagnostic pop
    }
    if (word >= ((uint32_t)kSweepRegRows << 24)) {
        float2 *p = hi + ((int)(word >> 24) - kSweepRegRows) * kWave;
        const float2 s = *p;
        *p = make_float2(s.x + t0, s.y + t1);
    }
}

// Zero both tuples where they live.  (As two plain assignments the equal values become ONE tuple elsewhere and 32 register
// copies into each pinned one, at every group's start.)
__device__ __forceinline__ void sweep_zero(SweepF32x32 &lo0, SweepF32x32 &lo1) {
    asm volatile(".set .Lsweep_zero_reg, 64\n\t"
                 ".rept 64\n\t"
                 "v_mov_b32_e32 v[.Lsweep_zero_reg], 0\n\t"
                 ".set .Lsweep_zero_reg, .Lsweep_zero_reg + 1\n\t"
                 ".endr"
                 : "={v[64:95]}"(lo0), "={v[96:127]}"(lo1));
}

// The table as a buffer descriptor, built once per launch (wave-uniform values only).  The range check of a raw buffer sees
// the scalar offset too (measured on gfx950: with `num_records` of one row every row but the first reads as zero), so
// `num_records` is the table's size in bytes and an offset beyond the table loads zero instead of faulting.  32 bits: a table
// of exactly 2^23 rows ends at byte 2^32, one more than the field can say -- that table alone keeps the global_load request
// (SweepArgs::wide; 2^23 rows are the most a layout names, cogdl_amd/sweepplan.py: MAX_TABLE_ROWS).
typedef int SweepRsrc __attribute__((ext_vector_type(4)));
__device__ __forceinline__ SweepRsrc sweep_table(const void *x, uint32_t bytes) {
    const uint64_t base = (uint64_t)(uintptr_t)x;
    SweepRsrc t;
    t.x = (int)(uint32_t)base;
    t.y = (int)(uint32_t)((base >> 32) & 0xffffu);  // (stride 0: a raw buffer)
    t.z = (int)bytes;
    t.w = 0x00020000;
    return t;
}

// One gather of the ring: the 512-byte row named by the layout word `word` (+ the lane's own 8 bytes), requested into `slot`.
// `word << 9` is the row's byte offset: the table has at most 2^23 rows, the local row in the top 8 bits falls out.  It is the
// load's scalar offset (one s_lshl; the lane's offset is a VGPR that never changes); WIDE: a VALU add and a global_load.
// The compiler takes `slot` for written when this returns; it is not, until sweep_wait has named it.
typedef float SweepF32x2 __attribute__((ext_vector_type(2)));
template <bool WIDE>
__device__ __forceinline__ void sweep_request(SweepF32x2 &slot, uint32_t word, uint32_t lane_off, const SweepRsrc &table, const char *x) {
    static_assert(kWave * sizeof(float2) == 512, "word << 9");
    if constexpr (WIDE) asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(slot) : "v"((word << 9) + lane_off), "s"(x));
    else asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=v"(slot) : "v"(lane_off), "s"(table), "s"(word << 9));
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
// MAPPED: the group's rows are named by a.rows (any rows of the structure, dealt to the groups by the layout's builder) instead of
// being consecutive; only the stores at the group's end differ.
template <bool WEIGHTED, bool WIDE, bool MAPPED>
__device__ __forceinline__ void sweep_walk(const SweepArgs &a) {
    constexpr int UNROLL = kSweepUnroll;
    static_assert(UNROLL % kSweepRing == 0 && kWave % UNROLL == 0, "a slot is an edge's place in its batch, a batch never straddles the words at hand");
    typedef const __attribute__((address_space(4))) int32_t *ConstI32;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t lane_off = (uint32_t)lane * (uint32_t)sizeof(float2);
    const char *const xb = reinterpret_cast<const char *>(a.x);
    const SweepRsrc table = sweep_table(a.x, a.table_bytes);
    // (the group offsets are read-only for the launch and their index is wave-uniform: scalar loads, counted on lgkmcnt)
    const ConstI32 goff = (ConstI32)(uintptr_t)a.goff;
    __shared__ float2 slab[4][kSweepLdsRows][kWave];
    float2 *const hi = &slab[threadIdx.x >> 6][0][lane];
    const int64_t wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t g = wave0; g < a.n_groups; g += n_waves) {  // (a wave past the last group exits)
        SweepF32x32 lo0, lo1;
        sweep_zero(lo0, lo1);
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
            int nbase = start + 2 * kWave;  // the words to ask for at the next turn
            int k = 0;                      // the batch's place in the words at hand
            // The words of an edge are read where its gather is requested and stay in the SGPRs that its fold reads
            // kSweepRing edges later: P[q] / W[q] belong to the edges at place q of a batch, a static rotation without copies.
            uint32_t P[UNROLL];
            float W[UNROLL];
            SweepF32x2 v[kSweepRing];
            // Prologue: the first kSweepRing gathers.
#pragma unroll
            for (int u = 0; u < kSweepRing; ++u) {
                P[u] = (uint32_t)__builtin_amdgcn_readlane((int)cp, u);
                W[u] = WEIGHTED ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cw), u)) : 1.f;
                sweep_request<WIDE>(v[u], P[u], lane_off, table, xb);
            }
            // Steady state: edge i waits for slot i % kSweepRing alone, is folded, and edge i + kSweepRing is requested into the
            // slot the fold has just freed.  `tested`: the batch may reach past the group's end (its last one only).
            int e = start;
            auto batch = [&](auto tested) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (u == UNROLL - kSweepRing && k == kWave - UNROLL) {
                        // The word turn: the requests from here on belong to the next 64 edges.  (Their words were requested
                        // 64 edges ago: the counted waits since have retired them, in order.)  The words after those: two
                        // more loads behind the ring's.  The counted wait stays what it is, so for the next kSweepRing edges a
                        // wait retires up to three gathers instead of one -- once in 64 edges.
                        sweep_words_turn(cp, cw, ncp, ncw);
                        sweep_words<WEIGHTED>(ncp, ncw, a.src, a.w, min(nbase + lane, last));
                        nbase += kWave;
                        k = -UNROLL;
                    }
                    SweepF32x2 &slot = v[u % kSweepRing];
                    sweep_wait(slot);
                    // (wave-uniform: a slot past the group's end is skipped, not folded as 0 * 0)
                    if (!decltype(tested)::value || e + u < end) sweep_fold<WEIGHTED>(lo0, lo1, hi, P[u], W[u], make_float2(slot.x, slot.y));
                    const int q = (u + kSweepRing) % UNROLL;
                    P[q] = (uint32_t)__builtin_amdgcn_readlane((int)cp, k + u + kSweepRing);
                    W[q] = WEIGHTED ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cw), k + u + kSweepRing)) : 1.f;
                    sweep_request<WIDE>(slot, P[q], lane_off, table, xb);
                }
                k += UNROLL;
                e += UNROLL;
            };
            while (e + UNROLL <= end) batch(std::false_type{});  // every slot inside the group: no test per edge
            if (e < end) batch(std::true_type{});
            sweep_drain(v, ncp, ncw);
        }
        if constexpr (MAPPED) {
            // (the map is read-only for the launch and its index is wave-uniform: scalar loads; every group has a.r slots)
            const ConstI32 rows = (ConstI32)(uintptr_t)a.rows + g * a.r;
            char *const dst = reinterpret_cast<char *>(a.out) + lane_off;
#pragma unroll
            for (int c = 0; c < kSweepRows; ++c) {
                if (c < a.r) {
                    const int row = rows[c];
                    if (row >= 0) {
                        const float2 o = c < kSweepRegRows ? make_float2(lo0[c & 31], lo1[c & 31]) : hi[(c & 15) * kWave];
                        *reinterpret_cast<float2 *>(dst + (uint64_t)row * (uint64_t)a.row_bytes) = o;
                    }
                }
            }
        } else {
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
}

template <bool WEIGHTED, bool WIDE, bool MAPPED>
__global__ __launch_bounds__(256, 4) void rowreduce_sweep_kernel(const SweepArgs a) {
    sweep_walk<WEIGHTED, WIDE, MAPPED>(a);
}

// The same walk, taken only if the guard says so (see the header comment); a wave that stands down has written nothing.
template <bool WEIGHTED, bool WIDE, bool MAPPED>
__global__ __launch_bounds__(256, 4) void rowreduce_sweep_guarded_kernel(const SweepArgs a, const HashGuard guard) {
    if (!guard_runs(guard)) return;
    sweep_walk<WEIGHTED, WIDE, MAPPED>(a);
}

// The arguments of either kernel for a table of n_src rows; -> WIDE, whether the table's end is beyond a descriptor's reach.
inline bool sweep_args(SweepArgs &a, const int32_t *goff, const int32_t *src, const void *w, const void *x, void *out, int64_t m,
                       int64_t n_src, int64_t n_groups, int r, int64_t k, const int32_t *rows) {
    const uint64_t bytes = (uint64_t)n_src * (uint64_t)k * sizeof(float);
    const bool wide = bytes > 0xffffffffull;
    a = SweepArgs{goff, (const uint32_t *)src, (const float *)w, (const float *)x, (float *)out, m, n_groups, r,
                  (uint32_t)(k * sizeof(float)), wide ? 0u : (uint32_t)bytes, rows};
    return wide;
}

// Launch the kernel that the arguments ask for: weighted or not, the wide request or the descriptor's, mapped rows or consecutive
// ones; guarded if `guard` is given.
template <bool WEIGHTED, bool WIDE, bool MAPPED>
inline void sweep_launch_as(const SweepArgs &a, const HashGuard *guard, unsigned blocks, hipStream_t s) {
    if (guard) hipLaunchKernelGGL((rowreduce_sweep_guarded_kernel<WEIGHTED, WIDE, MAPPED>), dim3(blocks), dim3(256), 0, s, a, *guard);
    else hipLaunchKernelGGL((rowreduce_sweep_kernel<WEIGHTED, WIDE, MAPPED>), dim3(blocks), dim3(256), 0, s, a);
}
template <bool WEIGHTED, bool WIDE>
inline void sweep_launch_rows(const SweepArgs &a, const HashGuard *guard, unsigned blocks, hipStream_t s) {
    if (a.rows) sweep_launch_as<WEIGHTED, WIDE, true>(a, guard, blocks, s);
    else sweep_launch_as<WEIGHTED, WIDE, false>(a, guard, blocks, s);
}
inline void sweep_launch(const SweepArgs &a, bool wide, const HashGuard *guard, unsigned blocks, hipStream_t s) {
    if (a.w && !wide) sweep_launch_rows<true, false>(a, guard, blocks, s);
    else if (a.w) sweep_launch_rows<true, true>(a, guard, blocks, s);
    else if (!wide) sweep_launch_rows<false, false>(a, guard, blocks, s);
    else sweep_launch_rows<false, true>(a, guard, blocks, s);
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
