// actq_law.h -- the law of activation compression: group-wise stochastic quantisation to 1, 2, 4 or 8 bits, the packed ReLU
// mask and the regenerated dropout, shared by the HIP kernels (actq.hip) and their host twin (host_actq.cpp).  Plain C++: no
// HIP runtime, libcogdl_host.so includes it and stays HIP-free.  Both libraries are built with -ffp-contract=off, every
// float32 expression below is written once and rounds the same on both sides: codes, metadata and dequantised values are
// equal bit for bit.  (Philox4x32-10 is walk_draw.h's restatement of philox.h's round function, which pulls in the HIP runtime.)
//
// Groups.  A tensor of n elements is quantised as its row-major flattening; group g holds the elements [g G, min((g + 1) G, n)),
// G in {64, 128, 256}.  (Not ActNN's per-sample groups, which pad every row to the group size: a 64-wide row would spend 256
// slots.)  The last group may be partial; slots beyond n take no part in min / max and their code bits are zero.
//
// Bounds.  x is canonicalised first: xc = x + 0.0f (-0 becomes +0; every other value, NaN payloads aside, is unchanged).
//     mn = the smallest, mx = the largest xc of the group that is not a NaN;  bad = "the group holds a NaN"
// Without -0 and NaN the values are totally ordered, so mn and mx do not depend on the order in which they are combined: the
// butterfly over 16, 32 or 64 lanes and the serial host loop agree.  With r = mx - mn (float32):
//     a group is FINITE when it holds no NaN and r is finite (r < inf): no infinite element, and bounds no further apart
//     than FLT_MAX.  Every other group (a NaN, an infinity, an overflowing range) is NOT REPRESENTABLE: it is stored as
//     (mn, step) = (NaN, NaN) with all codes zero, and dequantises to NaN throughout -- the failure stays visible.
// For a finite group, with L = 2^b - 1 (b in {1, 2, 4, 8}):
//     step  = r / L
//     scale = (mx > mn) ? min(L / r, FLT_MAX) : 0        (L / r overflows for r below L / FLT_MAX < 2^-119)
//
// Code.   u = (w >> 8) * 2^-24 in [0, 1), where w is word (i % 4) of
//             philox4x32_10(counter = (q_lo, q_hi, call_lo, call_hi), key = (seed_lo, seed_hi)),   q = i / 4
//         (i: the element's index in the flattening; q: the 64-bit number of its aligned quadruple, so one Philox call yields
//         the four draws of one lane's float4)
//     code = 0                                              when mx == mn (a constant group), and for a group not representable
//          = L                                              when xc == mx
//          = min(L, (uint32) floorf((xc - mn) * scale + u)) otherwise
// (xc - mn) * scale + u lies in [0, L + 2): the conversion is exact and no code leaves [0, L].  The maximum takes L by
// definition, not by rounding: fl(r * fl(L / r)) may fall just short of L.
//
// Storage.  Codes are packed little-endian into uint32 words: element i sits at bit b * (i % (32 / b)) of word i / (32 / b);
// ceil(n b / 32) words, the unused high bits of the last word are zero.  One (mn, step) float32 pair per group: 2 ceil(n / G)
// floats.  (ActNN keeps bf16 pairs; 8 bytes are 3 % of a 2-bit group of 256 and keep the bound below sharp.)
//
// Dequantise.  x' = mn + code * step  (float32: one product, one sum).
//   * a constant group returns mn exactly; the group's minimum returns mn and its maximum mn + L * step;
//   * E[x'] = x up to the roundings below (stochastic rounding with a uniform u);
//   * for a finite group, with U = 2^-24 and A = max(|mn|, |mn + L * step|):
//         |x' - xc|  <=  step * (1 + 16 L U)  +  2 U A  +  2^-119                                  (error_bound below)
//     Derivation.  Let R be the exact mx - mn and p = (xc - mn) L / R the element's exact position in [0, L].  The computed
//     t = fl(fl(fl(xc - mn) * fl(L / fl(R))) + u) carries four relative roundings of a value <= L and one of a value < L + 2:
//     |t - (p + u)| <= 4.1 U L + U (L + 2) <= 8 U L.  floorf takes off less than 1 and the clamp at L moves towards p, so
//     |code - p| < 1 + 8 U L.  The stored step is R / L within 2 U relative; code * step adds one relative rounding of a value
//     <= R = L step, the final sum one of a value <= A + step.  Together: step (1 + 8 U L) (1 + 2.1 U) + 3 U L step + U (A + step),
//     which the formula bounds.  Where L / r overflowed (r < 2^-119) the codes are compressed and the error is at most r: the
//     absolute term, which also covers the roundings of subnormal intermediates.
//
// ReLU mask.  Bit i % 64 of uint64 word i / 64 is (x[i] > 0); ceil(n / 64) words, the unused high bits of the last word are
// zero.  y[i] = x[i] > 0 ? x[i] : (x[i] is a NaN ? x[i] : +0): torch.relu elementwise, NaN included.
// mask_apply: out[i] = bit ? g[i] : +0.
//
// Dropout.  Nothing is stored but (seed, call, p).  With (thresh, scale) = drop_params(p) of philox.h -- thresh =
// round(p * 65536) clamped to [0, 65536], scale = 65536 / (65536 - thresh), or 0 when nothing is kept -- and w the word of
// element i as above:     keep = (w & 0xffff) >= thresh        y[i] = keep ? x[i] * scale : +0
// P[keep] = 1 - thresh / 65536 exactly; thresh = 0 keeps everything with scale = 1 (the identity, bit for bit), thresh = 65536
// keeps nothing.  A dropped NaN becomes 0 (torch's x * mask would keep it).  The backward is the same function of the
// gradient.  The quantiser and the dropout never share a `call` value in the Python layer (one counter serves both).
#pragma once
#include <stdint.h>

#include "walk_draw.h"

namespace cogdl_actq {

constexpr float kFltMax = 3.402823466e+38f;
constexpr int kTile = 256;  // elements a wave handles at a time: 64 lanes x one float4; every group size divides it

COGDL_WALK_FN bool valid_bits(int bits) { return bits == 1 || bits == 2 || bits == 4 || bits == 8; }
COGDL_WALK_FN bool valid_group(int group) { return group == 64 || group == 128 || group == 256; }

inline int64_t num_groups(int64_t n, int group) { return (n + group - 1) / group; }
inline int64_t num_code_words(int64_t n, int bits) { return (n * bits + 31) / 32; }
inline int64_t num_mask_words(int64_t n) { return (n + 63) / 64; }

// What an entry point checks before anything else: 0 ok, 1 invalid.  n * bits must not wrap: n < 2^59.
inline int sizes_status(int64_t n, int bits, int group) {
    return (n < 0 || n >= ((int64_t)1 << 59) || !valid_bits(bits) || !valid_group(group)) ? 1 : 0;
}

COGDL_WALK_FN bool is_nan(float x) { return x != x; }
COGDL_WALK_FN float canon(float x) { return x + 0.0f; }
COGDL_WALK_FN float quiet_nan() {
    union {
        uint32_t u;
        float f;
    } v;
    v.u = 0x7fc00000u;
    return v.f;
}

// The running bounds of a group: combine() is commutative and associative on them.
struct Bounds {
    float mn, mx;
    int bad;
};
COGDL_WALK_FN Bounds empty_bounds() {
    union {
        uint32_t u;
        float f;
    } p, m;
    p.u = 0x7f800000u;
    m.u = 0xff800000u;
    return {p.f, m.f, 0};
}
COGDL_WALK_FN void take(Bounds &b, float x) {  // x: as loaded
    const float xc = canon(x);
    if (is_nan(xc)) {
        b.bad = 1;
    } else {
        b.mn = xc < b.mn ? xc : b.mn;
        b.mx = xc > b.mx ? xc : b.mx;
    }
}
COGDL_WALK_FN Bounds combine(const Bounds &a, const Bounds &b) {
    return {b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx, a.bad | b.bad};
}

// A group's quantiser, from its bounds
struct Quant {
    float mn, step, mx, scale;
    uint32_t L;
    int finite, constant;
};
COGDL_WALK_FN Quant make_quant(const Bounds &b, int bits) {
    Quant q;
    q.L = (1u << bits) - 1u;
    const float r = b.mx - b.mn;
    q.finite = (!b.bad && r < empty_bounds().mn) ? 1 : 0;  // (r is a NaN for a group of equal infinities: not finite)
    if (!q.finite) {
        q.mn = q.step = q.mx = quiet_nan();
        q.scale = 0.0f;
        q.constant = 1;
        return q;
    }
    const float Lf = (float)q.L;
    q.mn = b.mn;
    q.mx = b.mx;
    q.step = r / Lf;
    q.constant = b.mx > b.mn ? 0 : 1;
    float s = 0.0f;
    if (!q.constant) {
        s = Lf / r;
        s = s < kFltMax ? s : kFltMax;
    }
    q.scale = s;
    return q;
}

// the four words of quadruple q of call `call`
COGDL_WALK_FN cogdl_walk::Draw draw4(uint64_t seed, uint64_t call, uint64_t q) {
    return cogdl_walk::philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)call, (uint32_t)(call >> 32), (uint32_t)seed,
                                     (uint32_t)(seed >> 32));
}
COGDL_WALK_FN uint32_t word_of(const cogdl_walk::Draw &d, int k) { return k == 0 ? d.x : (k == 1 ? d.y : (k == 2 ? d.z : d.w)); }

COGDL_WALK_FN uint32_t code_of(const Quant &q, float x, uint32_t w) {
    if (q.constant) return 0u;
    const float xc = canon(x);
    if (xc >= q.mx) return q.L;
    const float u = (float)(w >> 8) * 5.9604644775390625e-08f;  // 2^-24: exact
    const uint32_t c = (uint32_t)__builtin_floorf((xc - q.mn) * q.scale + u);
    return c < q.L ? c : q.L;
}

COGDL_WALK_FN float dequant(float mn, float step, uint32_t code) { return mn + (float)code * step; }

COGDL_WALK_FN uint32_t extract_code(const uint32_t *codes, int64_t i, int bits) {
    const int per = 32 / bits;
    return (codes[i / per] >> (bits * (int)(i % per))) & ((1u << bits) - 1u);
}

COGDL_WALK_FN float relu_of(float x) { return x > 0.0f ? x : (is_nan(x) ? x : 0.0f); }
COGDL_WALK_FN bool drop_keep(uint32_t w, uint32_t thresh) { return (w & 0xffffu) >= thresh; }
COGDL_WALK_FN float drop_of(float x, uint32_t w, uint32_t thresh, float scale) { return drop_keep(w, thresh) ? x * scale : 0.0f; }

// The guaranteed bound of |x' - xc| for an element of a finite group (double arithmetic: for tests and tools)
inline double error_bound(double mn, double step, int bits) {
    const double L = (double)((1u << bits) - 1u), U = 5.9604644775390625e-08;
    const double hi = mn + L * step;
    const double A = (mn < 0 ? -mn : mn) > (hi < 0 ? -hi : hi) ? (mn < 0 ? -mn : mn) : (hi < 0 ? -hi : hi);
    return step * (1.0 + 16.0 * L * U) + 2.0 * U * A + 1.504632769052528e-36;  // 2^-119
}

}  // namespace cogdl_actq
