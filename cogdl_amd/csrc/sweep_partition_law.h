// sweep_partition_law.h -- the law of the sweep's row-to-XCD partitioner, shared by the HIP kernels (sweep_partition.hip) and
// their host twin (host_sweep_partition.cpp).  Plain C++, integers only: no HIP runtime, libcogdl_host.so includes it.
//
// Rows of a structure (ptr [n_rows + 1], ind [nnz]: the gathered row of every edge, < n_src) carry a label in [0, P): the XCD
// whose L2 their gathers go through.  A gathered row costs an XCD one miss however many of its rows gather it, so rows that
// share gathered rows belong on the same XCD.  One round, from the labels it finds:
//   count      cnt[s, p] = edges with gathered row s in rows labelled p.
//   candidate  row i of label a and d edges, 1 <= d < kDegClasses: score(p) = its edges e with cnt[ind[e], p] - (p == a) > 0
//              (what OTHER edges of part p already gather; the edge itself is taken out, a second edge of the row to the same
//              gathered row is not).  Its best part b is a where no part scores above a, else the lowest part with the highest
//              score; b != a makes the row a candidate of bucket (a, b, d) with gain = score(b) - score(a) >= 1.
//              Rows without edges, rows of kDegClasses edges or more and rows with a label outside [0, P) never move; an edge
//              with a gathered row outside [0, n_src) counts nowhere.
//   accept     inside a bucket the candidates are ranked by key(gain, row): higher gain first, equal gains by ascending row.
//              Bucket (a, b, d) and its mirror (b, a, d) both accept their first quota = ceil(min(size, mirror's size) / 2).
//              An accepted row takes its best part as its label.  A bucket of more than kMaxBucket candidates, and its
//              mirror, accept nobody in that round: a rank is a count over the bucket, so a round costs at most kMaxBucket
//              reads per candidate whatever the graph (a regular graph puts every row of a pair of parts into one bucket).
// Rows therefore only ever swap parts with a row of the SAME edge count: the rows of every part and the edges of every part
// are what the starting labels made them, exactly, after any number of rounds.  Half of the matched candidates move because
// all scores of a round are taken against the labels the round started from.
// Nothing above depends on the order in which anything is computed: counts are sums, a rank is a count of smaller keys, and
// keys are distinct (they hold the row).  Same input, same labels, on either side and on any launch.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SWEEP_PART_HD __host__ __device__ __forceinline__
#define SWEEP_PART_UNROLL _Pragma("unroll")
#else
#define SWEEP_PART_HD inline
#define SWEEP_PART_UNROLL
#endif

namespace cogdl_sweep_part {

constexpr int kMaxParts = 8;
constexpr int kDegClasses = 64;
constexpr int kMaxBucket = 2048;

SWEEP_PART_HD int64_t n_buckets(int P) { return (int64_t)P * P * kDegClasses; }
SWEEP_PART_HD int bucket(int a, int b, int deg, int P) { return (a * P + b) * kDegClasses + deg; }
SWEEP_PART_HD int mirror(int bkt, int P) {
    const int deg = bkt % kDegClasses, ab = bkt / kDegClasses;
    return bucket(ab % P, ab / P, deg, P);
}
SWEEP_PART_HD int quota(int size, int mirror_size) {
    if (size > kMaxBucket || mirror_size > kMaxBucket) return 0;
    return ((size < mirror_size ? size : mirror_size) + 1) / 2;
}

SWEEP_PART_HD uint64_t key(int gain, int row) { return ((uint64_t)(uint32_t)(0x7fffffff - gain) << 32) | (uint32_t)row; }
SWEEP_PART_HD int key_row(uint64_t k) { return (int)(uint32_t)k; }

// a candidate word: best part | gain << 8, or kStays
constexpr int32_t kStays = -1;
SWEEP_PART_HD int cand_part(int32_t c) { return c & 0xff; }
SWEEP_PART_HD int cand_gain(int32_t c) { return c >> 8; }

SWEEP_PART_HD bool counted(int32_t s, int32_t label, int64_t n_src, int P) {
    return (uint32_t)s < (uint64_t)n_src && (uint32_t)label < (uint32_t)P;
}

// the candidate word of row i under the counts cnt [n_src, P] of the labels the round started from
SWEEP_PART_HD int32_t candidate(const int32_t *ptr, const int32_t *ind, const int32_t *cnt, const int32_t *labels, int64_t i,
                                int64_t n_src, int P) {
    const int32_t start = ptr[i], end = ptr[i + 1];
    const int own = labels[i];
    if (end <= start || end - start >= kDegClasses || (uint32_t)own >= (uint32_t)P) return kStays;
    int score[kMaxParts];
SWEEP_PART_UNROLL
    for (int p = 0; p < kMaxParts; ++p) score[p] = 0;
    for (int32_t e = start; e < end; ++e) {
        const int32_t s = ind[e];
        if (!counted(s, own, n_src, P)) continue;
        const int32_t *c = cnt + (int64_t)s * P;
SWEEP_PART_UNROLL
        for (int p = 0; p < kMaxParts; ++p)
            if (p < P) score[p] += (c[p] - (p == own ? 1 : 0)) > 0 ? 1 : 0;
    }
    int own_score = 0;
SWEEP_PART_UNROLL
    for (int p = 0; p < kMaxParts; ++p)
        if (p == own) own_score = score[p];
    int best = own, best_score = own_score;
SWEEP_PART_UNROLL
    for (int p = 0; p < kMaxParts; ++p)
        if (p < P && score[p] > best_score) {
            best = p;
            best_score = score[p];
        }
    return best == own ? kStays : (int32_t)(best | ((best_score - own_score) << 8));
}

// What an entry point checks before anything else: 0 ok, 1 invalid, 2 beyond the 32-bit indexing
SWEEP_PART_HD int sizes_status(int64_t n_rows, int64_t nnz, int64_t n_src, int P, int rounds) {
    if (n_rows < 0 || nnz < 0 || n_src < 0 || rounds < 0 || P < 1 || P > kMaxParts) return 1;
    const int64_t lim = 0x7fffffff;
    if (n_rows >= lim || nnz >= lim || n_src * P >= lim) return 2;
    return 0;
}

}  // namespace cogdl_sweep_part
