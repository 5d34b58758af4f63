// ppr_fixed.h -- the arithmetic and the rules of the top-k personalised PageRank ("forward push"), shared by the HIP
// kernel (ppr.hip) and its host twin (host_ppr.cpp).  Plain C++: no HIP runtime; libcogdl_host.so includes it and must stay
// HIP-free.  Both sides run the SAME integer functions in the same round structure, so they return the same arrays.
//
// Process (one source s).  r[s] = alpha.  Round 0 pushes s; round t >= 1 pushes exactly F_t = {v : r_t[v] pushable}, where
// pushable(v) means r[v] > 0 and r[v] >= alpha * eps * deg[v].  Pushing u: res = r[u]; p[u] += res; r[u] = 0; every
// out-neighbour v (an entry of u's row; deg[u] = indptr[u + 1] - indptr[u]) receives share = floor((1 - alpha) * res / deg[u]).
// All pushes of a round read the residuals of the round's start and their additions commute, so neither the order of
// the nodes inside a round nor the order of the additions can show.  The process ends when F_t is empty.
//
// Fixed point.  r and p are unsigned 64-bit counts of the quantum q = 2^-62:
//     r0   = floor(alpha * 2^62)            the initial residual
//     beta = floor((1 - alpha) * 2^64)      share = mulhi64(res, beta) / deg   (integer division)
//     thr  = floor(alpha * eps * 2^62)      pushable: r > 0 and r >= thr * deg (128-bit product; thr >= 1 is required)
// sum(p) <= 2^62 and sum(r) < 2^62, so nothing overflows.
//
// Bounded work (P3).  Every push but the first moves at least thr * deg[u] quanta into p and sum(p) <= 2^62, hence over
// one source   sum of deg[u] over pushes <= deg[s] + budget,   budget = floor(2^62 / thr) + 1 >= 1 / (alpha * eps),
// and at most 1 + deg[s] + budget distinct nodes are touched.  A round that pushes only nodes of degree 0 follows a round
// that pushed a node of degree >= 1 (they received their mass there), so there are at most 2 * budget + 3 rounds.
//
// Loss (P2).  Flooring only removes mass, so p never exceeds the exact PPR.  A push of u loses < 1 quantum in mulhi64,
// < 1 in the rounding of beta and <= deg[u] - 1 in the division; r0 loses < 1.  Over one source that is fewer than
// 3 * (deg[s] + budget + 1) quanta of residual, which would have become at most 1 / alpha times as much score.  A parameter
// set is accepted only if   4 * (E + budget + 2) / alpha * 2^-62 < 2^-24   (E >= deg[s]), so that the score lost to
// flooring is below 2^-24 in every entry.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define COGDL_PPR_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define COGDL_PPR_FN inline
#endif

namespace cogdl_ppr {

enum : int {
    kBadSource = 1,     // a source id outside [0, N)
    kBadNeighbour = 2,  // a neighbour id outside [0, N)
    kBadRowPtr = 4,     // a row of indptr that is not inside [0, E] or runs backwards
    kTableFull = 8,     // more nodes touched than the table was sized for (max_source_degree too small)
    kRoundCap = 16      // the round bound of (P3) was reached
};

constexpr int kFracBits = 62;
constexpr int64_t kMinCap = 1024;    // table slots: a power of two, at least twice the touched-node bound
constexpr int64_t kLdsCap = 2048;    // the GPU keeps tables of up to this many slots in LDS (68 KiB with its lists)
constexpr int64_t kMaxCap = (int64_t)1 << 23;

struct Params {
    uint64_t r0, beta, thr;
    int64_t budget;       // floor(2^62 / thr) + 1
    int64_t cap;          // table slots (power of two)
    int64_t max_touched;  // cap / 2: the touched list's length and the table's load limit
    int64_t max_rounds;   // 2 * budget + 3
};

struct Graph {
    const int64_t *indptr, *indices;
    int64_t num_nodes, num_edges;
};

// High 64 bits of a 64 x 64 -> 128-bit product, from 32-bit halves (the same code on both compilers).
COGDL_PPR_FN uint64_t mulhi64(uint64_t a, uint64_t b) {
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

COGDL_PPR_FN uint64_t share(uint64_t res, uint64_t beta, int64_t deg) {
    return deg > 0 ? mulhi64(res, beta) / (uint64_t)deg : 0;
}

// Did the addition old -> now (now > old) make a node of degree `deg` pushable?  Exactly one addition of a round does,
// whatever their order: pushable is monotone in r.
COGDL_PPR_FN bool crossed(uint64_t old, uint64_t now, uint64_t thr, int64_t deg) {
    if (mulhi64(thr, (uint64_t)deg) != 0) return false;  // thr * deg >= 2^64 > r
    const uint64_t t = thr * (uint64_t)deg;
    return now >= t && (old < t || old == 0);
}

COGDL_PPR_FN bool valid_id(const Graph &g, int64_t v) { return v >= 0 && v < g.num_nodes; }

// The row of a valid id; false (and an empty row) when indptr does not describe a range inside [0, E].
COGDL_PPR_FN bool row_of(const Graph &g, int64_t v, int64_t &lo, int64_t &hi) {
    lo = g.indptr[v];
    hi = g.indptr[v + 1];
    if (lo < 0 || hi < lo || hi > g.num_edges) {
        lo = hi = 0;
        return false;
    }
    return true;
}

// The float32 the caller sees: the fixed-point score rounded to nearest (ties to even), then scaled exactly.
COGDL_PPR_FN float to_f32(uint64_t p) { return (float)p * 0x1p-62f; }

// Output order: larger score first, ties by smaller node id.  Node ids are distinct, so the order is total.
COGDL_PPR_FN bool before(uint64_t pa, int64_t ka, uint64_t pb, int64_t kb) { return pa > pb || (pa == pb && ka < kb); }

COGDL_PPR_FN uint64_t hash_id(int64_t v) {  // splitmix64 finaliser
    uint64_t x = (uint64_t)v + 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// 0: accepted; 1: a parameter outside its domain; 2: accepted domain, but the loss bound or the table limit fails.
inline int make_params(double alpha, double eps, int64_t num_nodes, int64_t num_edges, int64_t max_source_degree, Params *out) {
    if (!(alpha > 0.0 && alpha < 1.0) || !(eps > 0.0) || !(eps < 1e300) || num_nodes < 0 || num_edges < 0 || max_source_degree < 0)
        return 1;
    if (!(1.0 - alpha < 1.0)) return 2;
    const double ae = alpha * eps;
    if (!(ae >= 0x1p-20) || !(ae < 1.0)) return 2;
    Params P;
    P.r0 = (uint64_t)floor(ldexp(alpha, kFracBits));
    P.beta = (uint64_t)floor(ldexp(1.0 - alpha, 64));
    P.thr = (uint64_t)floor(ldexp(ae, kFracBits));
    if (P.thr < 1 || P.r0 < 1) return 2;
    P.budget = (int64_t)((((uint64_t)1) << kFracBits) / P.thr) + 1;
    if (!(4.0 * ((double)num_edges + (double)P.budget + 2.0) < alpha * 0x1p38)) return 2;
    int64_t need = 1 + P.budget;
    need = max_source_degree > kMaxCap ? kMaxCap : need + max_source_degree;
    if (need > num_nodes) need = num_nodes;
    int64_t cap = kMinCap;
    while (cap < 2 * need && cap < kMaxCap) cap *= 2;
    if (cap < 2 * need) return 2;
    P.cap = cap;
    P.max_touched = cap / 2;
    P.max_rounds = 2 * P.budget + 3;
    *out = P;
    return 0;
}

}  // namespace cogdl_ppr
