// kgsample_law.h -- the law of filtered negative sampling for knowledge-graph embedding training, shared by the HIP kernel
// (kgsample.hip) and its host twin (host_kgsample.cpp).  Plain C++: no HIP runtime, libcogdl_host.so includes it and stays
// HIP-free.  Integers only: nothing here depends on a compiler's floating point.
//
// What is sampled.  The reference draws 2 K ids uniformly from [0, N), drops the ones that are true for the positive, repeats
// until K survive and keeps the first K (cogdl/datasets/kg_data.py:106-121): K independent draws, uniform over the entities
// that are NOT in the positive's true list, repeats allowed.  The same distribution is produced here without rejection.  For a
// positive whose sorted, distinct true list is a[0 .. L), with M = N - L free entities, negative j is the r-th free entity:
//     (x, y, z, w) = philox4x32_10(counter = (j >> 1, sid_lo, sid_hi, tag), key = (seed_lo, seed_hi))    (cogdl_walk)
//     u64 = (x << 32) | y  for even j,   (z << 32) | w  for odd j
//     r   = mulhi64(u64, M)                                in [0, M)
//     neg = r + #{ i : a[i] - i <= r }                     in [0, N), never an a[i]
// a[i] - i is the number of free entities below a[i]; it is non-decreasing in i, so the count is one upper-bound binary search
// (at most ceil(log2(L + 1)) probes, a bound that depends on L alone).  Every output element is a pure function of
// (seed, tag, sid, j) and the list: there is no rejection loop, and a list that leaves one entity free costs what an empty one
// costs.
//     tag   kTagHead for a head-batch (the list holds the true heads of (relation, tail)), kTagTail for a tail-batch
//     sid   the 64-bit ordinal of the positive in its mode's stream: first_sid + b for row b of a batch (modulo 2^64), so a
//           positive's negatives do not depend on how the stream is cut into batches
// Bias.  mulhi64(u, M) maps 2^64 equally likely words onto M values; each value gets floor(2^64 / M) or one more of them, so a
// probability differs from 1 / M by less than 2^-64 and the total variation from uniform is at most M / 2^64 (below 2^-33 for
// every M an int32 entity id allows).
//
// Refusals.  A triple id outside [0, T) raises kBadOrder; a group id or list bounds that do not lie inside the tables raise
// kBadTables; a list that leaves no entity free (M <= 0: the reference would loop forever) raises kNoFreeEntity.  Such a row is
// written as -1 (positive and negatives; weight 0) and nothing is indexed with the offending value.  A list that is not sorted
// and distinct gives wrong numbers, never an access outside the operands.
#pragma once
#include <stdint.h>

#include "walk_draw.h"

namespace cogdl_kgsample {

constexpr uint32_t kTagHead = 0x4B474E48u;  // "KGNH"
constexpr uint32_t kTagTail = 0x4B474E54u;  // "KGNT"
constexpr int kLdsList = 1024;              // the kernel stages lists of at most this many ids in LDS (as a[i] - i)

enum : int {
    kBadOrder = 1,      // an order id outside [0, T)
    kNoFreeEntity = 2,  // a true list that holds all N entities
    kBadTables = 4      // a group id outside [0, G) or list bounds outside [0, list_len]
};

// the 64-bit word of negative j of positive sid
COGDL_WALK_FN uint64_t draw_word(uint64_t seed, uint32_t tag, uint64_t sid, int64_t j) {
    const cogdl_walk::Draw d = cogdl_walk::philox4x32_10((uint32_t)((uint64_t)j >> 1), (uint32_t)sid, (uint32_t)(sid >> 32), tag,
                                                         (uint32_t)seed, (uint32_t)(seed >> 32));
    return (j & 1) ? (((uint64_t)d.z << 32) | d.w) : (((uint64_t)d.x << 32) | d.y);
}

// both words of the pair (2 p, 2 p + 1): one Philox call
COGDL_WALK_FN void draw_pair(uint64_t seed, uint32_t tag, uint64_t sid, int64_t p, uint64_t *even, uint64_t *odd) {
    const cogdl_walk::Draw d = cogdl_walk::philox4x32_10((uint32_t)(uint64_t)p, (uint32_t)sid, (uint32_t)(sid >> 32), tag,
                                                         (uint32_t)seed, (uint32_t)(seed >> 32));
    *even = ((uint64_t)d.x << 32) | d.y;
    *odd = ((uint64_t)d.z << 32) | d.w;
}

// The r-th entity that is missing from a list of L ids, r in [0, N - L).  gap(i) returns a[i] - i for i in [0, L).
template <typename Gap>
COGDL_WALK_FN int64_t nth_free(int64_t r, int32_t L, Gap gap) {
    int32_t lo = 0, hi = L;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)gap(mid) <= r) lo = mid + 1;
        else hi = mid;
    }
    return r + lo;
}

// negative j of positive sid from its word: the law's last two lines
template <typename Gap>
COGDL_WALK_FN int64_t negative_of(uint64_t word, int64_t M, int32_t L, Gap gap) {
    return nth_free((int64_t)cogdl_walk::mulhi64(word, (uint64_t)M), L, gap);
}

// What row b of a batch resolves to before anything is drawn: the triple id, its list [lo, lo + L) and M, or a refusal.
struct Row {
    int32_t t, lo, L;
    int64_t M;
    int err;  // 0, or the flag to raise: the row is written as -1
};

COGDL_WALK_FN Row resolve_row(const int32_t *order, int64_t b, const int32_t *group, const int32_t *list_ptr, int64_t T, int64_t G,
                              int64_t list_len, int64_t N) {
    Row row = {0, 0, 0, 0, 0};
    row.t = order[b];
    if (row.t < 0 || (int64_t)row.t >= T) {
        row.err = kBadOrder;
        return row;
    }
    const int32_t g = group[row.t];
    if (g < 0 || (int64_t)g >= G) {
        row.err = kBadTables;
        return row;
    }
    const int32_t lo = list_ptr[g], hi = list_ptr[g + 1];
    if (lo < 0 || hi < lo || (int64_t)hi > list_len) {
        row.err = kBadTables;
        return row;
    }
    row.lo = lo;
    row.L = hi - lo;
    row.M = N - (int64_t)row.L;
    if (row.M <= 0) row.err = kNoFreeEntity;
    return row;
}

// What an entry point checks before anything else: 0 ok, 1 invalid, 2 beyond int32 ids
inline int sizes_status(int64_t T, int64_t G, int64_t list_len, int64_t B, int64_t K, int64_t N) {
    if (T < 0 || G < 0 || list_len < 0 || B < 0 || K < 0 || N < 0) return 1;
    const int64_t lim = 0x7fffffff;
    if (T >= lim || G >= lim || list_len >= lim || B >= lim || K >= lim || N >= lim) return 2;
    return 0;
}

}  // namespace cogdl_kgsample
