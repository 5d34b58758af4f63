// readout_law.h -- the law of the batched graph readout (segment sum / mean / max pooling and sort-pool), shared by the HIP
// kernels (readout.hip) and their host twin (host_readout.cpp).  Plain C++: no HIP runtime, libcogdl_host.so includes it and
// stays HIP-free.  Every order of additions and every comparison is fixed here, so both sides return the same bytes.
//
// Segments.  Graph g owns the rows [lo, hi) of x[N, F] with lo = clamp(ptr[g], 0, N), hi = clamp(ptr[g + 1], lo, N): a
// malformed ptr gives wrong numbers, never an access outside x.  n = hi - lo.
//
// Sum.  Per column, float32 additions starting from +0.0f:
//     n <= kExactNodes   the rows in increasing order: the sequential sum (what torch's CPU scatter_add_ computes);
//     n >  kExactNodes   the rows are cut into chunks of kChunkRows consecutive rows; chunk c belongs to way c % kWays; a way
//                        adds the rows of its chunks in increasing row order into one accumulator that starts at +0.0f;
//                        the sum is ((way 0 + way 1) + way 2) + way 3.  Fixed, so equal from run to run, but no longer the
//                        sequential association.
// Mean.  The sum, then one rounded division by (float)n; an empty segment gives 0.
// Max.   best = -inf, arg = lo; for the rows in increasing order: x > best takes the row.  Ties therefore go to the
//        smallest row, a NaN is never taken, and a column that holds nothing above -inf gives -inf with arg = lo.  An empty
//        segment gives 0 and arg = -1.  Long segments use the ways as well; `better` below combines two candidates and is
//        order-independent, so the result is that of the sequential scan.
//
// Sort-pool.  Row i of a graph has the sort word  word(x[i, key_col], i - lo):  the key mapped to an unsigned integer that
// DEcreases as the key grows (-0.0f counts as +0.0f, every NaN as the largest key), in the high half, the row's position
// inside the graph in the low half.  Words of one graph are distinct; ascending word order is descending key order with equal
// keys in increasing row order -- the stable descending sort.  Both sides keep the min(k, n) smallest words.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define READOUT_HD __host__ __device__ __forceinline__
#else
#define READOUT_HD inline
#endif

namespace cogdl_readout {

enum : int { kSum = 0, kMean = 1, kMax = 2 };

constexpr int kExactNodes = 4096;  // segments up to this many rows: sequential sum
constexpr int kChunkRows = 1024;   // longer ones: chunks of this many rows ...
constexpr int kWays = 4;           // ... dealt round-robin to this many accumulators
constexpr int kLdsNodes = 2048;    // graphs up to this many rows are sorted in LDS by the kernel
constexpr uint64_t kPadWord = ~(uint64_t)0;

READOUT_HD int64_t clamp_row(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// way of the row at position j (0-based inside its segment) of a long segment
READOUT_HD int way_of(int64_t j) { return (int)((j / kChunkRows) % kWays); }

// (value, row) candidate a is replaced by b
READOUT_HD bool better(float bv, int64_t bi, float av, int64_t ai) { return bv > av || (bv == av && bi < ai); }

READOUT_HD uint32_t float_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return u;
#endif
}

READOUT_HD uint64_t word(float key, int64_t pos) {
    uint32_t u;
    if (key != key) {
        u = 0xffffffffu;
    } else {
        u = float_bits(key + 0.0f);  // (-0.0f + 0.0f is +0.0f)
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((uint64_t)(~u) << 32) | (uint64_t)(uint32_t)pos;
}

// What an entry point checks before anything else: 0 ok, 1 invalid, 2 beyond the int32 indexing
READOUT_HD int sizes_status(int64_t N, int64_t B, int64_t F, int64_t k) {
    if (N < 0 || B < 0 || F < 1 || k < 1) return 1;
    const int64_t lim = 0x7fffffff;
    if (N > lim || B >= lim || F > lim || k > lim || B * ((F + 63) / 64) > lim) return 2;
    return 0;
}

}  // namespace cogdl_readout
