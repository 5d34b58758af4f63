// wl_law.h -- the law of Weisfeiler-Lehman subtree relabelling on a batch of graphs, shared by the HIP kernels (wl.hip) and
// the host twin (host_wl.cpp).  Plain C++: no HIP runtime, libcogdl_host.so includes it and stays HIP-free.
//
// Inputs.  The int32 CSR (indptr [N + 1], indices [E]) of the disjoint union of the batch's graphs, taken as given:
// multiplicity counts and a self-loop is a neighbour.  label0 int64 [N] of arbitrary values.  rounds >= 0.
//
// The law.  sig_0(v) = (label0[v]); for r >= 0, sig_{r+1}(v) = (labels[r][v]; the neighbours' labels[r] in ascending order).
// rep_r(v) is the smallest node id with the same signature over the whole batch; labels[r][v] = #{u : rep_r(u) == u and
// u < rep_r(v)} (classes numbered by first occurrence); classes[r] = the number of representatives.  Nothing in the result
// depends on a hash function: the host compares signatures outright, the GPU hashes, then verifies every node against its
// representative element for element and raises kCollision where they differ.
//
// The hash (GPU route, and the host's emulation of a truncated hash): two 64-bit words w in {0, 1} of
//     H_w = mix(mix(own + salt + K_w) + mix(deg ^ K'_w) + sum_i mix((salt + K_w) ^ ((i + 1) * kPos) ^ ((uint64) list[i] << 1 | 1)))
// over the sorted list, all sums modulo 2^64, so the elements may be summed in any order.  `hash_bits` < 128 keeps the low
// bits only (of word 0 first): a test hook that makes collisions happen.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define COGDL_WL_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define COGDL_WL_FN inline
#endif

namespace cogdl_wl {

enum : int {
    kBadPtr = 1,      // indptr does not start at 0, runs backwards or does not end at E
    kBadIndex = 2,    // an index outside [0, N)
    kRowTooLong = 4,  // a row of more than kMaxDegree neighbours
    kCollision = 8,   // two different signatures with one hash (the verification caught it)
    kTableFull = 16   // the probe bound of the hash table was reached
};

constexpr int kMaxDegree = 32768;             // 128 KiB of LDS as int32
constexpr int64_t kMaxNodes = (int64_t)1 << 30;  // the table has the power of two >= 2 N slots, indexed in 32 bits
constexpr uint64_t kPos = 0x9e3779b97f4a7c15ull;

struct Hash {
    uint64_t lo, hi;
};

COGDL_WL_FN uint64_t mix(uint64_t z) {  // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

COGDL_WL_FN uint64_t word_key(uint64_t salt, int w) { return salt + (w ? 0x13198a2e03707344ull : 0x243f6a8885a308d3ull); }

// the contribution of the element at position i of the sorted list to word w
COGDL_WL_FN uint64_t element(uint64_t salt, int w, int64_t i, int32_t label) {
    return mix(word_key(salt, w) ^ ((uint64_t)(i + 1) * kPos) ^ (((uint64_t)(uint32_t)label << 1) | 1u));
}

COGDL_WL_FN uint64_t finish_word(uint64_t salt, int w, int64_t own, int64_t deg, uint64_t sum) {
    const uint64_t kd = w ? 0x082efa98ec4e6c89ull : 0xa4093822299f31d0ull;
    return mix(mix((uint64_t)own + word_key(salt, w)) + mix((uint64_t)deg ^ kd) + sum);
}

COGDL_WL_FN Hash truncate(Hash h, int hash_bits) {
    if (hash_bits >= 128) return h;
    if (hash_bits >= 64) {
        h.hi = hash_bits == 64 ? 0 : h.hi & ((((uint64_t)1) << (hash_bits - 64)) - 1);
        return h;
    }
    h.hi = 0;
    h.lo = hash_bits <= 0 ? 0 : h.lo & ((((uint64_t)1) << hash_bits) - 1);
    return h;
}

COGDL_WL_FN Hash finish(uint64_t salt, int64_t own, int64_t deg, uint64_t sum0, uint64_t sum1, int hash_bits) {
    Hash h = {finish_word(salt, 0, own, deg, sum0), finish_word(salt, 1, own, deg, sum1)};
    return truncate(h, hash_bits);
}

// slots of the open-addressing table: the power of two >= max(2 N, 64)
inline int64_t table_slots(int64_t N) {
    int64_t t = 64;
    while (t < 2 * N) t <<= 1;
    return t;
}

// argument checks both entry points share (0 = fine, 1 = invalid, 2 = out of range)
inline int args_status(int64_t N, int64_t E, int64_t rounds, int hash_bits) {
    if (N < 0 || E < 0 || rounds < 0 || hash_bits < 1 || hash_bits > 128) return 1;
    if (N > kMaxNodes || E > 0x7fffffff || rounds > 0x7fffffff) return 2;
    return 0;
}

}  // namespace cogdl_wl
