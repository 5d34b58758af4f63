// netsmf_host_check.cpp -- a stand-alone driver of cogdl_host_netsmf_sample for sanitizer runs of the HOST code (never
// loaded into Python, never run on a GPU).  Build and run from the repository root:
//     python -c "import sys; sys.path[:0] = ['.', 'tests']; import _netsmf_cases as c; ip, ix, n = c.gd(); \
//                open('/tmp/gd.bin', 'wb').write(ip.numpy().tobytes() + ix.numpy().tobytes()); print(n, ix.numel())"
//     g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DCOGDL_HOST_BUILD \
//         tools/netsmf_host_check.cpp cogdl_amd/csrc/host_netsmf.cpp -o /tmp/netsmf_host_check
//     /tmp/netsmf_host_check /tmp/gd.bin 300 2500
// It samples the graph of the file (int64 indptr[n + 1] then indices[e]) with window 10, then the same graph with a
// neighbour id outside [0, n) and with an indptr that runs backwards, and checks the flags word and the (-1, -1) pairs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/cogdl_host.h"

static int run(const std::vector<int64_t> &indptr, const std::vector<int64_t> &indices, int64_t n, int window, int want_flag) {
    const int64_t e = (int64_t)indices.size(), count = 2 * e + 37;
    std::vector<int32_t> row((size_t)(window * count)), col((size_t)(window * count));
    int flags = -1;
    const int rc = cogdl_host_netsmf_sample(indptr.data(), indices.data(), n, e, 5, count, window, 0x1234567890abcdefULL,
                                            row.data(), col.data(), &flags);
    if (rc != 0) return std::printf("status %d\n", rc), 1;
    int64_t bad = 0;
    for (size_t j = 0; j < row.size(); ++j) {
        if (row[j] == -1 && col[j] == -1) ++bad;
        else if (row[j] < 0 || row[j] >= n || col[j] < 0 || col[j] >= n) return std::printf("pair %zu out of range\n", j), 1;
    }
    std::printf("flags %d, %lld of %zu pairs are (-1, -1)\n", flags, (long long)bad, row.size());
    if (want_flag == 0) return flags != 0 || bad != 0;
    return !(flags & want_flag) || bad == 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return std::printf("usage: %s graph.bin num_nodes num_edges\n", argv[0]), 2;
    const int64_t n = std::atoll(argv[2]), e = std::atoll(argv[3]);
    std::vector<int64_t> indptr((size_t)n + 1), indices((size_t)e);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(indptr.data(), 8, indptr.size(), f) != indptr.size() ||
        std::fread(indices.data(), 8, indices.size(), f) != indices.size())
        return std::printf("cannot read %s\n", argv[1]), 2;
    std::fclose(f);
    int failed = run(indptr, indices, n, 10, 0);
    std::vector<int64_t> bad_ids = indices;
    bad_ids[17] = n;
    bad_ids[18] = -1;
    failed |= run(indptr, bad_ids, n, 10, 2);
    std::vector<int64_t> backwards = indptr;
    for (int i = 0; i < 10; ++i) std::swap(backwards[40 + i], backwards[59 - i]);
    failed |= run(backwards, indices, n, 10, 4);
    std::vector<int64_t> beyond = indptr;
    beyond[n] += 1000;
    beyond[n / 2] = -7;
    failed |= run(beyond, indices, n, 10, 4);
    std::printf(failed ? "FAILED\n" : "ok\n");
    return failed;
}
