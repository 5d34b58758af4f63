// host_sweep_partition.cpp -- the host twin of csrc/sweep_partition.hip: which XCD the rows of a sweep layout run on.  Counts,
// scores, buckets, keys and quotas are sweep_partition_law.h's, the same the kernels follow, so for equal inputs the labels are
// the GPU's.  One thread (a build runs once per structure); no HIP.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/cogdl_host.h"
#include "sweep_partition_law.h"

namespace sp = cogdl_sweep_part;

extern "C" int cogdl_host_sweep_partition(const int32_t *ptr, const int32_t *ind, int64_t n_rows, int64_t nnz, int64_t n_src,
                                          int n_parts, int rounds, int32_t *labels, void *workspace, size_t workspace_bytes) {
    (void)workspace, (void)workspace_bytes;  // (the kernels' scratch: not read here)
    const int rc = sp::sizes_status(n_rows, nnz, n_src, n_parts, rounds);
    if (rc != 0) return rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE;
    if (n_rows == 0) return COGDL_HOST_OK;
    if (!ptr || !labels || (nnz > 0 && !ind)) return COGDL_HOST_EINVAL;
    const int P = n_parts;
    if (ptr[0] != 0 || ptr[n_rows] != nnz) return COGDL_HOST_EINVAL;
    for (int64_t i = 0; i < n_rows; ++i) {
        if (ptr[i + 1] < ptr[i]) return COGDL_HOST_EINVAL;
        if (labels[i] < 0 || labels[i] >= P) return COGDL_HOST_ERANGE;
    }
    for (int64_t e = 0; e < nnz; ++e)
        if (ind[e] < 0 || ind[e] >= n_src) return COGDL_HOST_ERANGE;

    const int64_t B = sp::n_buckets(P);
    std::vector<int32_t> cnt((size_t)n_src * P), cand(n_rows), size(B);
    std::vector<std::pair<int32_t, uint64_t>> list;  // (bucket, key): sorted, a bucket's candidates stand in rank order
    for (int round = 0; round < rounds; ++round) {
        std::fill(cnt.begin(), cnt.end(), 0);
        std::fill(size.begin(), size.end(), 0);
        for (int64_t i = 0; i < n_rows; ++i)
            for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e)
                if (sp::counted(ind[e], labels[i], n_src, P)) ++cnt[(size_t)ind[e] * P + labels[i]];
        list.clear();
        for (int64_t i = 0; i < n_rows; ++i) {
            const int32_t c = cand[i] = sp::candidate(ptr, ind, cnt.data(), labels, i, n_src, P);
            if (c == sp::kStays) continue;
            const int32_t b = sp::bucket(labels[i], sp::cand_part(c), ptr[i + 1] - ptr[i], P);
            ++size[b];
            list.emplace_back(b, sp::key(sp::cand_gain(c), (int)i));
        }
        if (list.empty()) break;  // (no later round would find a candidate either: the labels stay)
        std::sort(list.begin(), list.end());
        int32_t rank = 0;
        for (size_t t = 0; t < list.size(); ++t) {
            const int32_t b = list[t].first;
            rank = (t > 0 && list[t - 1].first == b) ? rank + 1 : 0;
            if (rank < sp::quota(size[b], size[sp::mirror(b, P)])) {
                const int row = sp::key_row(list[t].second);
                labels[row] = sp::cand_part(cand[row]);
            }
        }
    }
    return COGDL_HOST_OK;
}
