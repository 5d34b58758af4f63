// line_law.h -- the law of edge-sampled skip-gram training with negative sampling (LINE, orders 1 and 2), shared by the HIP
// kernel (line.hip) and its host twin (host_line.cpp).  Plain C++ on top of walk_draw.h (Philox4x32-10, mulhi64) and
// sgns_law.h (dot-product tree, sigmoid table, initialisation): no HIP runtime.  Every draw and every rounding is fixed here,
// so wherever execution is serial (workers == 1) the tables are a function of the inputs alone and equal on both sides, bit
// for bit.
//
// Inputs.  eu, ev int64 [M]: the endpoints of M >= 1 undirected edges, ids in [0, V).  ecum int64 [M] or null: the cumulative
// edge weights, non-decreasing, first entry >= 0, last entry in [1, 2^52]; null means unit weights.  ncum uint32 [V]: the node
// noise table in sgns_law.h's format (non-decreasing, last entry >= 1).  exp_table float [1000].  D in [1, 512], K in [1, 16],
// order in {1, 2}, S >= 0 samples, alpha > 0, a 64-bit seed.  Tables emb [V, D] and, for order 2, ctx [V, D].
//
// Draws.  (x, y, z, w)(s, slot) = philox4x32_10(counter = (s lo, s hi, slot, 0x4c494e45), key = seed) for sample s.
//     edge       slot 0: r = mulhi64((y << 32) | x, T), T = M (unit weights) or ecum[M - 1]; e = r (unit weights), else the first
//                index with ecum[e] > r, by a binary search that stays inside [0, M - 1] whatever the table holds (an edge of
//                weight 0 is never drawn); (u, v) = (eu[e], ev[e]), swapped iff z & 1 (the fair coin that orients the edge)
//     negative   slot d in 1..K: t = the first index with ncum[t] > x % ncum[V - 1] (the rule of sgns_law.h's draw_negative)
// A negative equal to u or to v is skipped: word2vec's rule, which sgns_law.h follows.  (The original LINE program does not
// skip; it trains such a draw with label 0.)
//
// Per sample s, in order: lr = (float)(alpha * max(1.0 - (double)s / (double)S, 1e-4)) in double; the input row x = emb[u] is
// read ONCE, at the start of the sample; err = 0; the target table T is emb (order 1) or ctx (order 2); target 0 is v with
// label 1, targets 1..K are the negatives with label 0; per target f = dot(x, T[t]) by sgns_law.h's dot-product rule; a NaN f
// skips the target; sig = 1 for f >= 6, 0 for f <= -6, else exp_table[min(999, (int)((f + 6) * (1000 / 12)))]: outside the
// bound THE UPDATE STILL APPLIES, as in the original program (word2vec, and sgns_law.h, skip there); g = (label - sig) * lr;
// err += g * T[t] (the old row), then T[t] += g * x; after the last target emb[u] += err (added to what memory holds then: for
// a self-loop in order 1, T[v] is emb[u] and has already received g * x).  A target row that the same sample has already
// updated (two equal negatives) is read again after that update.
//
// Arithmetic.  float32 with contraction off on both sides, as sgns_law.h states.
//
// Initialisation.  emb = sgns_law.h's init_value ((u24 / 2^24 - 0.5) / D: the reference's (random - 0.5) / dimension); ctx = 0.
#pragma once
#include <stdint.h>

#include "sgns_law.h"
#include "walk_draw.h"

namespace cogdl_line {

enum : int {
    kBadEndpoint = 1,   // an endpoint outside [0, V)
    kBadNodeTable = 2,  // ncum runs backwards or ends in 0
    kBadEdgeTable = 4   // ecum starts below 0, runs backwards or ends outside [1, 2^52]
};

constexpr uint32_t kStream = 0x4c494e45u;
constexpr int64_t kEdgeTotalMax = (int64_t)1 << 52;
constexpr int kMaxDim = cogdl_sgns::kMaxDim, kMaxNegative = cogdl_sgns::kMaxNegative;

COGDL_WALK_FN cogdl_walk::Draw draw(uint64_t seed, int64_t s, uint32_t slot) {
    return cogdl_walk::philox4x32_10((uint32_t)(uint64_t)s, (uint32_t)((uint64_t)s >> 32), slot, kStream, (uint32_t)seed,
                                     (uint32_t)(seed >> 32));
}

// the edge of sample s and its orientation; e is inside [0, M - 1] whatever ecum holds
COGDL_WALK_FN int64_t draw_edge(uint64_t seed, int64_t s, const int64_t *ecum, int64_t M, bool &swapped) {
    const cogdl_walk::Draw d = draw(seed, s, 0u);
    swapped = (d.z & 1u) != 0;
    const uint64_t x64 = ((uint64_t)d.y << 32) | d.x;
    if (!ecum) return (int64_t)cogdl_walk::mulhi64(x64, (uint64_t)M);
    return cogdl_sgns::first_above(ecum, M, (int64_t)cogdl_walk::mulhi64(x64, (uint64_t)ecum[M - 1]));
}

// what negative d in 1..K of sample s looks up in ncum
COGDL_WALK_FN uint32_t negative_key(uint64_t seed, int64_t s, int d, const uint32_t *ncum, int64_t V) {
    return draw(seed, s, (uint32_t)d).x % ncum[V - 1];
}

// the first index with ncum[t] > the key
COGDL_WALK_FN int64_t draw_negative(uint64_t seed, int64_t s, int d, const uint32_t *ncum, int64_t V) {
    return cogdl_sgns::first_above(ncum, V, negative_key(seed, s, d, ncum, V));
}

COGDL_WALK_FN float learning_rate(double alpha, int64_t s, int64_t S) {
    const double left = 1.0 - (double)s / (double)S;
    return (float)(alpha * (left > 1e-4 ? left : 1e-4));
}

// LINE's rule for sgns_law.h's inner step: only a NaN skips the target; outside -6 < f < 6 the sigmoid saturates
struct Saturate {
    static COGDL_WALK_FN bool applies(float f) { return f == f; }
    static COGDL_WALK_FN float gradient(float f, float label, float lr, const float *exp_table) {
        float sig;
        if (f >= 6.0f) sig = 1.0f;
        else if (f <= -6.0f) sig = 0.0f;
        else {
            int idx = (int)((f + 6.0f) * (1000.0f / 12.0f));
            idx = idx > cogdl_sgns::kExpTable - 1 ? cogdl_sgns::kExpTable - 1 : idx;
            sig = exp_table[idx];
        }
        return (label - sig) * lr;
    }
};

// argument checks both entry points share (0 = fine, 1 = invalid, 2 = out of range)
inline int args_status(int64_t M, int64_t V, int D, int negative, int order, int64_t S, double alpha) {
    if (M < 1 || V < 1 || D < 1 || negative < 1 || S < 0 || (order != 1 && order != 2)) return 1;
    if (!(alpha > 0.0) || alpha - alpha != 0.0) return 1;
    if (D > kMaxDim || negative > kMaxNegative || V > 0x7fffffff) return 2;
    return 0;
}

}  // namespace cogdl_line
