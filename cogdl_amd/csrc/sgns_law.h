// sgns_law.h -- the law of skip-gram training with negative sampling (SGNS), shared by the HIP kernel (sgns.hip) and its
// host twin (host_sgns.cpp).  Plain C++ on top of walk_draw.h (Philox4x32-10): no HIP runtime, libcogdl_host.so includes it
// and stays HIP-free.  Every draw and every rounding is fixed here, so wherever execution is serial (workers == 1) the two
// tables are a function of the inputs alone and equal on both sides, bit for bit.
//
// Inputs.  walks int64 [W, L] (ids in [0, V); a negative id is padding), D in [1, 512], window in [1, 32], negative K in
// [1, 16], epochs >= 1, alpha / min_alpha, keep uint32 [V], cum uint32 [V] (non-decreasing, last entry >= 1; the caller
// builds 2^31 - 1), exp_table float [1000] (word2vec.c's sigmoid table, built by the caller in double), a 64-bit seed.
//
// Draws.  x(c2, c3) = philox4x32_10(counter = (row w, epoch e, c2, c3), key = seed).x
//     subsample   position p of row w is kept iff x(p, 0) <= keep[id]     (keep = 2^32 - 1: always; floor(prob * 2^32) else)
//     window      centre i (index among the kept tokens): b = x(i, 1) % window
//     negative    pair (centre i, context j), target d in 1..K: r = x(i | j << 16, 1 + d) % cum[V - 1], t = the first index
//                 with cum[t] > r (binary search on [0, V - 1])
//
// Per epoch e, per row w in order: lr = (float)(alpha - (alpha - min_alpha) * (e W + w) / (epochs W)) in double; the kept
// tokens are compacted into s[0, n) in order; per centre i in order, per j ascending over [max(0, i - window + b),
// min(n - 1, i + window - b)], j != i: the input row is syn0[s[j]], neu = 0; target 0 is s[i] with label 1, targets 1..K
// are the negatives with label 0, skipped when t == s[i]; per target f = dot(syn0[in], syn1[t]); the target is applied iff
// -6 < f < 6 (a NaN is skipped); g = (label - exp_table[min(999, (int)((f + 6) * (1000 / 12)))]) * lr;
// neu += g * syn1[t], then syn1[t] += g * syn0[in] (the old syn1[t] enters neu); after the last target syn0[in] += neu.
//
// Arithmetic.  float32; CONTRACTION IS OFF ON BOTH SIDES: every a * b + c is a rounded product, then a rounded sum (both
// libraries are built with -ffp-contract=off; a memory-side atomic add of the rounded product is the same sum).  The dot
// product: element d belongs to lane d % 64; lane l sums its products in ascending d starting from 0.0f + (first product);
// lanes without an element hold 0; the lane sums are combined by a butterfly of width B = the power of two >= min(D, 64):
// for s = B/2, B/4, .., 1: p[l] = p[l] + p[l ^ s]; f is p[0].  (x + y is commutative, so the host evaluates the same tree
// on the lower half only.)
//
// Initialisation.  syn0[v][d] = (u24 / 2^24 - 0.5) / D with u24 = philox(counter = (v lo, v hi, d, 0x53474e53), key = seed).x
// >> 8, in float: u24 * 2^-24 is exact, the subtraction is exact, one rounded division.  syn1 = 0.
#pragma once
#include <stdint.h>

#include "walk_draw.h"

namespace cogdl_sgns {

enum : int {
    kBadId = 1,    // an id >= V in walks
    kBadTable = 2  // cum runs backwards or ends in 0
};

constexpr int kMaxDim = 512, kMaxWindow = 32, kMaxNegative = 16, kMaxLength = 1024, kExpTable = 1000, kLanes = 64;
constexpr uint32_t kInitStream = 0x53474e53u;

COGDL_WALK_FN uint32_t draw_x(uint64_t seed, int64_t row, int64_t epoch, uint32_t c2, uint32_t c3) {
    return cogdl_walk::philox4x32_10((uint32_t)(uint64_t)row, (uint32_t)(uint64_t)epoch, c2, c3, (uint32_t)seed,
                                     (uint32_t)(seed >> 32))
        .x;
}

COGDL_WALK_FN bool keep_token(uint64_t seed, int64_t row, int64_t epoch, int pos, uint32_t keep_t) {
    return draw_x(seed, row, epoch, (uint32_t)pos, 0u) <= keep_t;
}

COGDL_WALK_FN int window_shrink(uint64_t seed, int64_t row, int64_t epoch, int centre, int window) {
    return (int)(draw_x(seed, row, epoch, (uint32_t)centre, 1u) % (uint32_t)window);
}

// The first index with table[index] > r, by a binary search that stays inside [0, n - 1] whatever the table holds.  Every
// cumulative table of the trainers is searched by this one function (noise tables are uint32, LINE's edge table int64).
template <typename T>
COGDL_WALK_FN int64_t first_above(const T *table, int64_t n, T r) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (table[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// cum[V - 1] >= 1 is checked before any row runs.
COGDL_WALK_FN int64_t draw_negative(uint64_t seed, int64_t row, int64_t epoch, int centre, int context, int d,
                                    const uint32_t *cum, int64_t V) {
    return first_above(cum, V, draw_x(seed, row, epoch, (uint32_t)centre | ((uint32_t)context << 16), 1u + (uint32_t)d) % cum[V - 1]);
}

// `flag` if cum runs backwards or ends in 0, over the entries first, first + stride, .. that the caller walks (a thread of a
// check kernel its own, the host all of them)
COGDL_WALK_FN int noise_table_flags(const uint32_t *cum, int64_t V, int64_t first, int64_t stride, int flag) {
    int err = 0;
    for (int64_t v = first; v < V; v += stride) {
        if (v > 0 && cum[v] < cum[v - 1]) err |= flag;
        if (v == V - 1 && cum[v] == 0) err |= flag;
    }
    return err;
}

COGDL_WALK_FN float learning_rate(double alpha, double min_alpha, int64_t epoch, int64_t row, int64_t W, int64_t epochs) {
    return (float)(alpha - (alpha - min_alpha) * (double)(epoch * W + row) / (double)(epochs * W));
}

// Which targets are applied, and with what gradient: the one thing the trainers' inner step differs in.  word2vec's rule
// (skip-gram, PV-DBOW): outside -6 < f < 6 the target is skipped (a NaN too).  LINE's rule is line_law.h's Saturate.
struct Skip {
    static COGDL_WALK_FN bool applies(float f) { return f > -6.0f && f < 6.0f; }
    static COGDL_WALK_FN float gradient(float f, float label, float lr, const float *exp_table) {
        int idx = (int)((f + 6.0f) * (1000.0f / 12.0f));
        idx = idx > kExpTable - 1 ? kExpTable - 1 : idx;
        return (label - exp_table[idx]) * lr;
    }
};

// `stream` separates the tables that are initialised this way (pvdbow_law.h has one of its own)
COGDL_WALK_FN float init_value(uint64_t seed, int64_t v, int d, int D, uint32_t stream = kInitStream) {
    const uint32_t u24 = cogdl_walk::philox4x32_10((uint32_t)(uint64_t)v, (uint32_t)((uint64_t)v >> 32), (uint32_t)d, stream,
                                                   (uint32_t)seed, (uint32_t)(seed >> 32))
                             .x >>
                         8;
    return ((float)u24 * (1.0f / 16777216.0f) - 0.5f) / (float)D;
}

// width of the butterfly: the power of two >= min(D, 64)
COGDL_WALK_FN int butterfly_width(int D) {
    int b = 1;
    while (b < D && b < kLanes) b <<= 1;
    return b;
}

// argument checks both entry points share (0 = fine, 1 = invalid, 2 = out of range)
inline int args_status(int64_t W, int64_t L, int64_t V, int D, int window, int negative, int64_t epochs, double alpha,
                       double min_alpha) {
    if (W < 0 || L < 1 || V < 1 || D < 1 || window < 1 || negative < 1 || epochs < 1) return 1;
    if (!(alpha == alpha) || !(min_alpha == min_alpha)) return 1;
    if (D > kMaxDim || window > kMaxWindow || negative > kMaxNegative || L > kMaxLength) return 2;
    if (V > 0x7fffffff || W > 0x7fffffff || epochs > 0x7fffffff) return 2;
    return 0;
}

}  // namespace cogdl_sgns
