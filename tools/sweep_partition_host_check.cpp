// sweep_partition_host_check.cpp -- the host twin of the sweep's row-to-XCD partitioner (csrc/host_sweep_partition.cpp) run on a
// generated graph as a stand-alone program, for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/sweep_partition_host_check.cpp cogdl_amd/csrc/host_sweep_partition.cpp -o /tmp/sweep_partition_host_check && /tmp/sweep_partition_host_check
// Checks what the law promises: rows and edges per part unchanged, two runs equal, fewer distinct (part, gathered row) pairs.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "cogdl_host.h"

static uint64_t next(uint64_t &s) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

static size_t pairs(const std::vector<int32_t> &ptr, const std::vector<int32_t> &ind, const std::vector<int32_t> &labels) {
    std::set<std::pair<int32_t, int32_t>> seen;
    for (size_t i = 0; i + 1 < ptr.size(); ++i)
        for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e) seen.insert({labels[i], ind[e]});
    return seen.size();
}

int main() {
    const int64_t n_rows = 5003, n_src = 3001;
    const int P = 8;
    uint64_t s = 88172645463325252ull;
    std::vector<int32_t> ptr(n_rows + 1, 0), ind;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int deg = i % 97 == 0 ? 70 : (int)(next(s) % 20);  // (rows without edges, and rows too long to move)
        for (int e = 0; e < deg; ++e) ind.push_back((int32_t)(next(s) % n_src));
        ptr[i + 1] = (int32_t)ind.size();
    }
    std::vector<int32_t> start(n_rows);
    for (int64_t i = 0; i < n_rows; ++i) start[i] = (int32_t)(i % P);
    std::vector<int32_t> a = start, b = start;
    const int64_t nnz = (int64_t)ind.size();
    if (cogdl_host_sweep_partition(ptr.data(), ind.data(), n_rows, nnz, n_src, P, 6, a.data(), nullptr, 0) != 0) return 1;
    if (cogdl_host_sweep_partition(ptr.data(), ind.data(), n_rows, nnz, n_src, P, 6, b.data(), nullptr, 0) != 0) return 1;
    if (a != b) return 2;
    std::vector<int64_t> rows0(P, 0), rows1(P, 0), edges0(P, 0), edges1(P, 0);
    for (int64_t i = 0; i < n_rows; ++i) {
        if (a[i] < 0 || a[i] >= P) return 3;
        ++rows0[start[i]], ++rows1[a[i]];
        edges0[start[i]] += ptr[i + 1] - ptr[i], edges1[a[i]] += ptr[i + 1] - ptr[i];
    }
    if (rows0 != rows1 || edges0 != edges1) return 4;
    const size_t before = pairs(ptr, ind, start), after = pairs(ptr, ind, a);
    std::printf("rows %lld edges %lld: distinct (part, gathered row) pairs %zu -> %zu\n", (long long)n_rows, (long long)nnz, before, after);
    if (after >= before) return 5;
    // refused: a label outside the parts, a gathered row outside the table, more parts than the law has
    b[7] = P;
    if (cogdl_host_sweep_partition(ptr.data(), ind.data(), n_rows, nnz, n_src, P, 1, b.data(), nullptr, 0) != COGDL_HOST_ERANGE) return 6;
    if (cogdl_host_sweep_partition(ptr.data(), ind.data(), n_rows, nnz, n_src - 2000, P, 1, a.data(), nullptr, 0) != COGDL_HOST_ERANGE) return 7;
    if (cogdl_host_sweep_partition(ptr.data(), ind.data(), n_rows, nnz, n_src, 9, 1, a.data(), nullptr, 0) != COGDL_HOST_EINVAL) return 8;
    std::printf("ok\n");
    return 0;
}
