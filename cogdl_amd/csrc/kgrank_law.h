// kgrank_law.h -- the law of all-entity ranking (knowledge-graph link prediction), shared by the HIP kernels (kgrank.hip) and
// their host twin (host_kgrank.cpp).  Plain C++: no HIP runtime, libcogdl_host.so includes it and stays HIP-free.
//
// A query row q[D] and a candidate row t[D] have one score s(q, t).  It is a pure function of the two rows with one fixed
// order of float32 operations over k; it does not depend on the tile, the workgroup or the launch that computes it, there is
// no split over k, and the target's score comes from the same operations as every candidate's.  That is what makes `==`
// between two scores meaningful.  Both libraries are built with -ffp-contract=off: an fma happens where fmaf is written.
// (kgscore_law.h, the law of sampled scoring for training, reuses the per-term steps below but sums them in another order --
// 64 slot partials and a butterfly, which a wave can execute; here one thread owns a pair of rows and walks k sequentially.
// The difference is intended: the two operators never compare scores with each other.)
//
//   dot   acc = +0;  for k = 0 .. D-1:    acc = fmaf(q[k], t[k], acc);                                           s = acc
//         (bit for bit what v_mfma_f32_32x32x2_f32 computes from a zero accumulator with k ascending; fmaf(q, t, .) and
//          fmaf(t, q, .) are equal, and a zero-padded k adds fmaf(0, 0, acc) = acc, acc never being -0)
//   l1    acc = +0;  for k = 0 .. D-1:    acc = acc + |q[k] - t[k]|;                                              s = gamma - acc
//   cl2   acc = +0;  for k = 0 .. D/2-1:  re = q[k] - t[k];  im = q[k + D/2] - t[k + D/2];
//                                         acc = acc + sqrtf(re * re + im * im);                                   s = gamma - acc
//         (every operation rounded once to float32; sqrtf correctly rounded on both sides; D even)
//
// Counting.  Candidate e of query i with target t falls into bucket  0: s_e > s_t,  1: s_e == s_t and e < t,  2: s_e == s_t
// and e > t,  none otherwise.  A NaN compares false both ways: a NaN candidate is counted nowhere, and under a NaN target
// score nothing is counted.  The target itself is not a candidate.
//
// Filter lists.  At the C ABI the ids of one query are in non-decreasing order; an id equal to its predecessor in the list is
// a duplicate and is passed over, so is the target, so is an id outside [0, N).  Every remaining entry is scored under the
// same law and taken out of the bucket it was counted in.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KGRANK_HD __host__ __device__ __forceinline__
#else
#define KGRANK_HD inline
#endif

namespace cogdl_kgrank {

enum : int { kDot = 0, kL1 = 1, kCl2 = 2 };

KGRANK_HD float dot_step(float acc, float q, float t) { return fmaf(q, t, acc); }
KGRANK_HD float l1_step(float acc, float q, float t) { return acc + fabsf(q - t); }
KGRANK_HD float cl2_step(float acc, float q_re, float q_im, float t_re, float t_im) {
    const float re = q_re - t_re, im = q_im - t_im;
    const float rr = re * re, ii = im * im;
    return acc + sqrtf(rr + ii);
}
KGRANK_HD float finish(int kind, float gamma, float acc) { return kind == kDot ? acc : gamma - acc; }

// s(q, t) for rows of D floats
KGRANK_HD float score(int kind, float gamma, const float *q, const float *t, int64_t D) {
    float acc = 0.0f;
    if (kind == kDot) {
        for (int64_t k = 0; k < D; ++k) acc = dot_step(acc, q[k], t[k]);
    } else if (kind == kL1) {
        for (int64_t k = 0; k < D; ++k) acc = l1_step(acc, q[k], t[k]);
    } else {
        const int64_t h = D / 2;
        for (int64_t k = 0; k < h; ++k) acc = cl2_step(acc, q[k], q[k + h], t[k], t[k + h]);
    }
    return finish(kind, gamma, acc);
}

// bucket of candidate e (score s) against target t (score st): 0, 1, 2, or -1 for none
KGRANK_HD int bucket(float s, float st, int64_t e, int64_t t) {
    if (e == t) return -1;
    if (s > st) return 0;
    if (s == st) return e < t ? 1 : 2;
    return -1;
}

// What an entry point checks before anything else: 0 ok, 1 invalid, 2 beyond the int32 indexing
KGRANK_HD int sizes_status(int64_t M, int64_t N, int64_t D, int kind, int64_t filt_len) {
    if (M < 0 || N < 0 || D < 0 || filt_len < 0 || kind < kDot || kind > kCl2) return 1;
    if (kind == kCl2 && (D & 1)) return 1;
    const int64_t lim = 0x7fffffff;
    if (M >= lim || N >= lim || D >= lim || filt_len >= lim) return 2;
    return 0;
}

}  // namespace cogdl_kgrank
