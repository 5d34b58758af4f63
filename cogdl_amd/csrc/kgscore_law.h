// kgscore_law.h -- the law of sampled triple scoring (knowledge-graph embedding training), shared by the HIP kernels
// (kgscore.hip) and their host twin (host_kgscore.cpp).  Plain C++: no HIP runtime, libcogdl_host.so includes it and stays
// HIP-free.  Both libraries are built with -ffp-contract=off: an fma happens where fmaf is written.
//
// Score.  A query row q[D] and a table row t[D] have one score s(q, t), a pure function of the two rows.  The three kinds and
// their per-term steps are kgrank_law.h's (dot_step, l1_step, cl2_step, finish); the ORDER of the sum is not: kgrank_law.h
// walks k sequentially (one thread owns a pair of rows there), here a wave of 64 lanes owns a pair of rows, so the order is one
// a wave can execute.  This difference is intended; the two operators never compare scores with each other.
//   term index k runs over D for dot and l1, over the D/2 complex pairs (q[k], q[k + D/2]) for cl2;
//   term k belongs to slot (k >> 2) & 63: slot l owns the groups of four consecutive terms 4 (l + 64 i) .. 4 (l + 64 i) + 3;
//   each of the 64 slots adds its terms from +0 in ascending k;
//   the partials are combined by the butterfly  p[l] = p[l] + p[l ^ off]  for off = 32, 16, 8, 4, 2, 1 (all l at once: float
//   addition commutes, so every l ends with the same bits);
//   s = finish(kind, gamma, p[0]).
// The slot map does not depend on how a row is loaded (float4 or scalars), on K, on the position j or on the launch.
//
// Partial derivatives, one rounding per operation.
//   dot   ds/dq_k = t_k                       ds/dt_k = q_k
//   l1    d = q_k - t_k                       ds/dq_k = -sgn(d), ds/dt_k = +sgn(d), sgn(0) = 0 (a NaN d gives 0 as well)
//   cl2   re, im the differences, m = sqrtf(re * re + im * im):
//                                             ds/dq_re = -(re / m), ds/dq_im = -(im / m), the negatives of these for t;
//                                             all four 0 where m == 0
//   (torch gives the same zeros for norm(p=1) and for stack([re, im]).norm(dim=0) at a zero difference.)
//   A contribution is g * partial, rounded once.
//
// Gradient sums.
//   grad_q[b, k]      adds the contributions of j = 0 .. K-1 from +0 in ascending j.
//   grad_table[e, k]  adds the contributions of the occurrences of e in ascending flat position b K + j: sequentially from +0
//                     inside chunks of kChunk = 512 occurrences, the chunk partials then added to +0 in ascending chunk order.
//                     An entity with no occurrence gets +0.
// Ids.  An idx entry outside [0, N) scores NaN and contributes to no gradient.  Malformed indices (idx, occ_ptr, occ_pos) give
// wrong numbers, never an access outside the operands.
#pragma once
#include <math.h>
#include <stdint.h>

#include "kgrank_law.h"

namespace cogdl_kgscore {

namespace kg = cogdl_kgrank;

constexpr int kSlots = 64;
constexpr int64_t kChunk = 512;   // occurrences of one entity summed sequentially before a partial is closed
constexpr int64_t kMaxD = 16384;  // the widest row the kernels serve (a query row is held in LDS)

KGRANK_HD int slot_of(int64_t k) { return (int)((k >> 2) & (kSlots - 1)); }

// the number of terms the sum runs over
KGRANK_HD int64_t terms_of(int kind, int64_t D) { return kind == kg::kCl2 ? D / 2 : D; }

// one term into a slot's accumulator; `half` is D / 2 (read for cl2 only)
KGRANK_HD float term_step(int kind, float acc, const float *q, const float *t, int64_t k, int64_t half) {
    if (kind == kg::kDot) return kg::dot_step(acc, q[k], t[k]);
    if (kind == kg::kL1) return kg::l1_step(acc, q[k], t[k]);
    return kg::cl2_step(acc, q[k], q[k + half], t[k], t[k + half]);
}

// p[64] -> every entry the butterfly's sum
KGRANK_HD void butterfly(float *p) {
    for (int off = kSlots / 2; off >= 1; off >>= 1) {
        float n[kSlots];
        for (int l = 0; l < kSlots; ++l) n[l] = p[l] + p[l ^ off];
        for (int l = 0; l < kSlots; ++l) p[l] = n[l];
    }
}

// s(q, t) for rows of D floats, as one thread computes it
KGRANK_HD float score(int kind, float gamma, const float *q, const float *t, int64_t D) {
    float p[kSlots];
    for (int l = 0; l < kSlots; ++l) p[l] = 0.0f;
    const int64_t terms = terms_of(kind, D), half = D / 2;
    for (int64_t k = 0; k < terms; ++k) {
        const int l = slot_of(k);
        p[l] = term_step(kind, p[l], q, t, k, half);
    }
    butterfly(p);
    return kg::finish(kind, gamma, p[0]);
}

// ds/dq of term k: one value for dot and l1 (d_a), two for cl2 (d_a for column k, d_b for column k + D/2).  ds/dt is
// partial_t below.
KGRANK_HD void partial_q(int kind, float q_a, float q_b, float t_a, float t_b, float *d_a, float *d_b) {
    if (kind == kg::kDot) {
        *d_a = t_a;
        *d_b = 0.0f;
    } else if (kind == kg::kL1) {
        const float d = q_a - t_a;
        *d_a = d > 0.0f ? -1.0f : (d < 0.0f ? 1.0f : 0.0f);
        *d_b = 0.0f;
    } else {
        const float re = q_a - t_a, im = q_b - t_b;
        const float rr = re * re, ii = im * im;
        const float m = sqrtf(rr + ii);
        if (m == 0.0f) {
            *d_a = 0.0f;
            *d_b = 0.0f;
        } else {
            *d_a = -(re / m);
            *d_b = -(im / m);
        }
    }
}

KGRANK_HD void partial_t(int kind, float q_a, float q_b, float t_a, float t_b, float *d_a, float *d_b) {
    if (kind == kg::kDot) {
        *d_a = q_a;
        *d_b = 0.0f;
    } else {
        partial_q(kind, q_a, q_b, t_a, t_b, d_a, d_b);
        *d_a = -*d_a;
        *d_b = -*d_b;
    }
}

// acc + g * partial: the contribution rounded once, then the sum
KGRANK_HD float add_contribution(float acc, float g, float partial) {
    const float c = g * partial;
    return acc + c;
}

// What an entry point checks before anything else: 0 ok, 1 invalid, 2 beyond the int32 indexing (B K included)
KGRANK_HD int sizes_status(int64_t B, int64_t K, int64_t N, int64_t D, int kind) {
    if (B < 0 || K < 0 || N < 0 || D < 0 || kind < kg::kDot || kind > kg::kCl2) return 1;
    if (kind == kg::kCl2 && (D & 1)) return 1;
    const int64_t lim = 0x7fffffff;
    if (B >= lim || K >= lim || N >= lim || D >= lim) return 2;
    if (B * K >= lim) return 2;
    return 0;
}

}  // namespace cogdl_kgscore
