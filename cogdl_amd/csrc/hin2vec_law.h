// hin2vec_law.h -- the law of HIN2Vec's training rows and of its score, shared by the HIP kernels (hin2vec.hip) and the host
// twin of the pair builder (host_hin2vec.cpp).  Plain C++: no HIP runtime, libcogdl_host.so includes it and stays HIP-free
// (the Philox round function is walk_draw.h's restatement for that reason).  The pair builder is integers only; the score
// is float32 with one rounding per written operation (both libraries are built with -ffp-contract=off).
//
// Slots.  Walks are int64 [W, L] with -1 from a walk's end on; hop in [1, kMaxHop], L > hop.  A slot is (w, i, j) with
// i in [0, L - hop) and j in [1, hop], numbered s = (w (L - hop) + i) hop + (j - 1).  It is LIVE when walk[w, i + hop] != -1
// (the reference's range(len(walk) - hop) on the true length) and walk[w, i] != walk[w, i + j] (its `if x == y: continue`;
// cogdl/models/emb/hin2vec.py:94-100).  Rows appear in slot order, a slot's positive first and its negatives behind it.
//
// Positive row.  (x, y, key, 1) with x = walk[w, i], y = walk[w, i + j] and
//     key = (j << 54) | SUM_{k = 0 .. j} type(walk[w, i + k]) << (6 k)            (types in [0, 64), j + 1 <= 9 of them)
// so two slots share a key exactly when their type sequences are equal.
//
// Negative rows.  Negative n of slot s keeps the key, has label 0 and replaces one side:
//     (a, b, c, d) = philox4x32_10(counter = (s_lo, s_hi, n, kTag), key = (seed_lo, seed_hi))
//     side         = a & 1: 1 replaces x, 0 replaces y
//     t, c         = the replaced node's type and the number of nodes of that type
//     u            = mulhi64((b << 32) | c_word, c - 1)                            in [0, c - 1)
//     replacement  = type_nodes[type_ptr[t] + u + (u >= rank[node])]               (rank: the node's place in its type's list)
// uniform over the nodes of type t other than the node itself (bias below c / 2^64), two dependent loads, no rejection loop,
// and a pure function of (seed, s, n): rows do not depend on launch geometry or thread count.  A type with a single node
// cannot be corrupted (the reference loops forever); the operator refuses it before anything is launched, and the law writes
// -1 and raises kBadTables where it meets one all the same.
//
// Validation.  Position p of a walk is staged as (id, type): -1 stays -1; an id outside [0, N) raises kBadNode, a type outside
// [0, 64) raises kBadType, and either is staged as -1; a -1 followed by anything else raises kBadTail.  A slot that touches a
// staged -1 is not live, so nothing is ever indexed with a refused value; what a flagged call returns is unspecified.
//
// Score (hin2vec.hip only: expf differs between two libms, so there is no host twin).  For a sample (x, y, r) over rows of d
// floats, term k is  (Wx[x, k] * Wx[y, k]) * f(Wr[r, k]),  f(w) = s (1 - s) with s = 1 / (1 + expf(-clamp(w, -6, 6))).  Term
// k belongs to slot (k >> 2) & 63 (kgscore_law.h's map); every slot adds its terms from +0 in ascending k, the 64 partials
// are folded by the butterfly p[l] = p[l] + p[l ^ off], off = 32 .. 1, and p = 1 / (1 + expf(-sum)).
// Gradients, with g_b = grad_p[b] * (p_b * (1 - p_b)):
//     grad_Wx[n, k]  adds  g_b * (Wx[other_b, k] * f(Wr[r_b, k]))  over the occurrences of n among (x_0 .. x_{B-1}, y_0 ..
//                    y_{B-1}) in ascending position (other: the sample's other side; x_b == y_b contributes twice);
//     grad_Wr[r, k]  adds  g_b * (Wx[x_b, k] * Wx[y_b, k])  over the occurrences of r in ascending b, and the sum is
//                    multiplied once by f'(Wr[r, k]) = f (1 - 2 s) for -6 <= w <= 6 and 0 outside (torch's clamp gradient).
// Occurrences are summed sequentially from +0 inside chunks of kChunk = 512; the chunk partials are added to +0 in ascending
// chunk order.  A row without occurrences gets +0.  An id outside its table scores NaN and contributes to no gradient.
#pragma once
#include <math.h>
#include <stdint.h>

#include "walk_draw.h"

namespace cogdl_hin2vec {

constexpr int kMaxHop = 8;
constexpr int kMaxTypes = 64;
constexpr int kTypeBits = 6;
constexpr int kHopShift = kTypeBits * (kMaxHop + 1);  // 54
constexpr uint32_t kTag = 0x48494E4Eu;                 // "HINN"
constexpr int64_t kChunk = 512;
constexpr int64_t kMaxD = 16384;

enum : int {
    kBadNode = 1,   // a walk entry that is neither -1 nor in [0, N)
    kBadType = 2,   // a node type outside [0, 64)
    kBadTail = 4,   // a -1 that is followed by a node
    kBadTables = 8  // a type list that cannot give a replacement (fewer than two nodes, or bounds outside the tables)
};

// One walk entry and the raw entry behind it (-1 at the row's end) -> what is staged; raises into err.
COGDL_WALK_FN void stage(int64_t v, int64_t next, const int32_t *node_type, int64_t N, int32_t &id, int32_t &type, int &err) {
    id = -1;
    type = -1;
    if (v == -1) {
        if (next != -1) err |= kBadTail;
        return;
    }
    if ((uint64_t)v >= (uint64_t)N) {
        err |= kBadNode;
        return;
    }
    const int32_t t = node_type[v];
    if ((uint32_t)t >= (uint32_t)kMaxTypes) {
        err |= kBadType;
        return;
    }
    id = (int32_t)v;
    type = t;
}

// Is slot (i, j) of a staged walk live?  id(p) returns the staged id of position p; p runs up to i + hop.
template <typename Id>
COGDL_WALK_FN bool slot_live(Id id, int64_t i, int j, int hop) {
    if (id(i + hop) < 0 || id(i) == id(i + j)) return false;
    for (int k = 0; k <= j; ++k)
        if (id(i + k) < 0) return false;  // (cannot happen in a validated walk: -1 is a suffix)
    return true;
}

template <typename Type>
COGDL_WALK_FN int64_t slot_key(Type type, int64_t i, int j) {
    uint64_t key = (uint64_t)j << kHopShift;
    for (int k = 0; k <= j; ++k) key |= (uint64_t)(uint32_t)type(i + k) << (kTypeBits * k);
    return (int64_t)key;
}

COGDL_WALK_FN uint64_t slot_number(int64_t w, int64_t i, int j, int64_t L, int hop) {
    return ((uint64_t)w * (uint64_t)(L - hop) + (uint64_t)i) * (uint64_t)hop + (uint64_t)(j - 1);
}

struct TypeTables {
    const int32_t *type_ptr;    // [kMaxTypes + 1]
    const int32_t *type_nodes;  // [N]: node ids grouped by type, ascending inside a type
    const int32_t *rank;        // [N]: type_nodes[type_ptr[type[v]] + rank[v]] == v
    int64_t N;
};

// Negative n of slot s for the positive (x, y) with types (tx, ty): the law's five lines.
COGDL_WALK_FN void negative_row(const TypeTables &tb, uint64_t seed, uint64_t s, int64_t n, int32_t x, int32_t y, int32_t tx,
                                int32_t ty, int64_t &nx, int64_t &ny, int &err) {
    const cogdl_walk::Draw d = cogdl_walk::philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)n, kTag, (uint32_t)seed,
                                                         (uint32_t)(seed >> 32));
    const bool side_x = (d.x & 1u) != 0;
    const int32_t node = side_x ? x : y, t = side_x ? tx : ty;
    const int64_t lo = tb.type_ptr[t], c = (int64_t)tb.type_ptr[t + 1] - lo;
    int64_t got = -1;
    if (c < 2 || lo < 0 || lo + c > tb.N) {
        err |= kBadTables;
    } else {
        const int64_t u = (int64_t)cogdl_walk::mulhi64(((uint64_t)d.y << 32) | d.z, (uint64_t)(c - 1));
        const int64_t at = lo + u + (u >= (int64_t)tb.rank[node] ? 1 : 0);
        if (at < lo + c) got = tb.type_nodes[at];
        else err |= kBadTables;
    }
    nx = side_x ? got : (int64_t)x;
    ny = side_x ? (int64_t)y : got;
}

// What the pair entry points check first: 0 ok, 1 invalid, 2 out of range
inline int pairs_status(int64_t W, int64_t L, int hop, int64_t negative, int64_t N) {
    if (W < 0 || L < 1 || N < 0 || negative < 0 || hop < 1 || hop > kMaxHop || L <= hop) return 1;
    const int64_t lim = 0x7fffffff;
    if (W >= lim * 64 || L >= (1 << 27) || N >= lim || negative >= lim) return 2;
    if ((uint64_t)W * (uint64_t)(L - hop) >= ((uint64_t)1 << 59) / ((uint64_t)hop * (uint64_t)(negative + 1))) return 2;
    return 0;
}

// ---------------------------------------------------------------- the score
COGDL_WALK_FN float sigmoid_of(float v) { return 1.0f / (1.0f + expf(-v)); }

// f(w) and f'(w): one expf for both
COGDL_WALK_FN void regularise(float w, float &f, float &df) {
    const float c = w < -6.0f ? -6.0f : (w > 6.0f ? 6.0f : w);
    const float s = sigmoid_of(c);
    f = s * (1.0f - s);
    df = (w >= -6.0f && w <= 6.0f) ? f * (1.0f - 2.0f * s) : 0.0f;
}

COGDL_WALK_FN float regularise_f(float w) {
    float f, df;
    regularise(w, f, df);
    return f;
}

COGDL_WALK_FN float term_step(float acc, float xk, float yk, float wk) {
    const float xy = xk * yk;
    const float t = xy * regularise_f(wk);
    return acc + t;
}

// g_b from the incoming gradient and the saved p
COGDL_WALK_FN float sample_grad(float grad_p, float p) {
    const float q = 1.0f - p;
    const float pq = p * q;
    return grad_p * pq;
}

// acc + g * v: the contribution rounded once, then the sum
COGDL_WALK_FN float add_contribution(float acc, float g, float v) {
    const float c = g * v;
    return acc + c;
}

// 0 ok, 1 invalid, 2 beyond the int32 indexing (2 B included: the node occurrences)
inline int score_status(int64_t B, int64_t N, int64_t R, int64_t D) {
    if (B < 0 || N < 0 || R < 0 || D < 0) return 1;
    const int64_t lim = 0x3fffffff;
    if (B >= lim || N >= lim || R >= lim || D > kMaxD) return 2;
    return 0;
}

}  // namespace cogdl_hin2vec
