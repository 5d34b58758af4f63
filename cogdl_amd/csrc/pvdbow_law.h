// pvdbow_law.h -- the law of PV-DBOW training (gensim's Doc2Vec(dm=0): skip-gram with negative sampling whose input row is
// the document's vector) over ragged documents, shared by the HIP kernel (pvdbow.hip) and its host twin (host_pvdbow.cpp).
// On top of sgns_law.h: draw_x, draw_negative's binary search, learning_rate, the Skip rule (applies, gradient),
// butterfly_width, init_value and the order of the dot product are used unchanged.  There is no cap on a document's length and no window draw.
//
// Inputs.  doc_ptr int64 [G + 1], non-decreasing from 0 to at most T; words int64 [T] with ids in [0, V) (a negative id is
// padding); D in [1, 512], negative K in [1, 16], epochs >= 1, alpha / min_alpha, keep / cum uint32 [V] and exp_table as in
// sgns_law.h, a 64-bit seed.
//
// Draws.  x(c2, c3) = philox4x32_10(counter = (document g, epoch e, c2, c3), key = seed).x
//     subsample   position p of document g (p < 2^32) is kept iff x(p, 0) <= keep[id]
//     negative    position p, target d in 1..K: r = x(p, 1 + d) % cum[V - 1], t = the first index with cum[t] > r
//
// Per epoch e, per document g in order: lr = learning_rate(alpha, min_alpha, e, g, G, epochs); per kept position p ascending:
// the input row is dv[g], neu = 0; target 0 is the word with label 1, targets 1..K are the negatives with label 0, skipped
// when equal to the word; per target f = dot(dv[g], syn1[t]); the target is applied iff -6 < f < 6; g = gradient(f, label,
// lr); neu += g * syn1[t], then syn1[t] += g * dv[g]; after the last target dv[g] += neu.
//
// Initialisation.  dv[g][d] = (u24 / 2^24 - 0.5) / D with u24 = philox(counter = (g lo, g hi, d, kDocStream), key = seed).x >> 8
// (sgns_law.h's init_value under a stream constant of its own).  syn1 = 0.  Contraction is off on both sides.
#pragma once
#include <stdint.h>

#include "sgns_law.h"

namespace cogdl_pvdbow {

namespace sg = cogdl_sgns;

enum : int {
    kBadId = 1,     // an id >= V in words
    kBadTable = 2,  // cum runs backwards or ends in 0
    kBadPtr = 4     // doc_ptr starts below 0, runs backwards or ends past T
};

constexpr uint32_t kDocStream = 0x50564442u;

COGDL_WALK_FN bool keep_position(uint64_t seed, int64_t doc, int64_t epoch, uint32_t pos, uint32_t keep_t) {
    return sg::draw_x(seed, doc, epoch, pos, 0u) <= keep_t;
}

// draw_negative packs (centre | context << 16) into the counter word: the two halves of p give c2 = p
COGDL_WALK_FN int64_t draw_negative(uint64_t seed, int64_t doc, int64_t epoch, uint32_t pos, int d, const uint32_t *cum, int64_t V) {
    return sg::draw_negative(seed, doc, epoch, (int)(pos & 0xffffu), (int)(pos >> 16), d, cum, V);
}

COGDL_WALK_FN float init_value(uint64_t seed, int64_t g, int d, int D) { return sg::init_value(seed, g, d, D, kDocStream); }

// argument checks both entry points share (0 = fine, 1 = invalid, 2 = out of range)
inline int args_status(int64_t G, int64_t T, int64_t V, int D, int negative, int64_t epochs, double alpha, double min_alpha) {
    if (G < 0 || T < 0 || V < 1 || D < 1 || negative < 1 || epochs < 1) return 1;
    if (!(alpha == alpha) || !(min_alpha == min_alpha)) return 1;
    if (D > sg::kMaxDim || negative > sg::kMaxNegative) return 2;
    if (V > 0x7fffffff || G > 0x7fffffff || epochs > 0x7fffffff) return 2;
    return 0;
}

}  // namespace cogdl_pvdbow
