// filter_host_check.cpp -- a stand-alone driver of cogdl_host_csr_filter_step for sanitizer runs of the HOST code (never
// loaded into Python, never run on a GPU).  Build and run from the repository root:
//     g++ -O1 -g -std=c++17 -ffp-contract=off -fopenmp -fsanitize=address,undefined -fno-sanitize-recover=undefined -DCOGDL_HOST_BUILD \
//         tools/filter_host_check.cpp cogdl_amd/csrc/host_ops.cpp -o /tmp/filter_host_check
//     /tmp/filter_host_check
// A 400-node structure whose rows have 0, 1 and 129 edges (and a few in between; enough cells for the OpenMP path) is
// stepped with every combination of the optional operands (val, b, z1, z2, dst_scale, acc), at widths 1, 7, 64 and 65
// (one column block, its edge and one past it), with out as its own buffer, as z1 and as z2; every result is compared with a
// plain loop written here.  Then the refusals: out / acc aliasing x, out aliasing acc, a shifted z, a malformed rowptr and
// a column id outside [0, n).  Every buffer has its exact size, so a read or write past an end is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/cogdl_host.h"

namespace {

constexpr int64_t kNodes = 400;

struct Csr {
    std::vector<int32_t> rowptr, colind;
};

Csr make_structure() {
    Csr g;
    uint64_t x = 88172645463325252ULL;
    auto next = [&x]() { return x ^= x << 13, x ^= x >> 7, x ^= x << 17, x; };
    g.rowptr.assign(1, 0);
    for (int64_t v = 0; v < kNodes; ++v) {
        const int64_t deg = v % 7 == 0 ? 0 : v % 7 == 1 ? 1 : v % 7 == 2 ? 129 : 2 + (int64_t)(next() % 20);
        for (int64_t k = 0; k < deg; ++k) g.colind.push_back((int32_t)(next() % kNodes));
        g.rowptr.push_back((int32_t)g.colind.size());
    }
    return g;
}

std::vector<float> noise(size_t n, uint64_t seed) {
    std::vector<float> v(n);
    uint64_t x = seed * 2654435761ULL + 1;
    for (size_t i = 0; i < n; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        v[i] = (float)((int64_t)(x % 2001) - 1000) / 512.0f;
    }
    return v;
}

// the contract, one element at a time (built like the library: no contraction)
void plain(const Csr &g, const float *val, const std::vector<float> &x, int64_t k, float a, float b, const float *z1, float c1,
           const float *z2, float c2, const float *scale, const float *acc, float d, std::vector<float> &out, std::vector<float> &acc_out) {
    for (int64_t i = 0; i < kNodes; ++i)
        for (int64_t j = 0; j < k; ++j) {
            float t = 0.f;
            for (int32_t e = g.rowptr[i]; e < g.rowptr[i + 1]; ++e) {
                const float xv = x[(size_t)g.colind[e] * k + j];
                volatile float p = val ? val[e] * xv : xv;
                t = t + p;
            }
            volatile float s = scale ? scale[i] * t : t;
            volatile float y = a * s;
            if (b != 0.f) { volatile float p = b * x[i * k + j]; y = y + p; }
            if (z1) { volatile float p = c1 * z1[i * k + j]; y = y + p; }
            if (z2) { volatile float p = c2 * z2[i * k + j]; y = y + p; }
            out[i * k + j] = y;
            if (acc) { volatile float p = d * y; acc_out[i * k + j] = acc[i * k + j] + p; }
        }
}

int same(const char *what, const std::vector<float> &a, const std::vector<float> &b) {
    if (a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0)) return 0;
    std::printf("%s: result differs from the plain loop\n", what);
    return 1;
}

int run_width(const Csr &g, int64_t k) {
    const size_t cells = (size_t)(kNodes * k);
    const int64_t nnz = (int64_t)g.colind.size();
    const std::vector<float> x = noise(cells, 1), z1 = noise(cells, 2), z2 = noise(cells, 3), acc0 = noise(cells, 4);
    const std::vector<float> val = noise((size_t)nnz, 5), scale = noise((size_t)kNodes, 6);
    int failed = 0, runs = 0;
    for (int mask = 0; mask < 64; ++mask)
        for (int alias = 0; alias < 3; ++alias) {  // 0: own buffer, 1: out is z1, 2: out is z2
            const bool has_val = mask & 1, has_b = mask & 2, has_z1 = mask & 4, has_z2 = mask & 8, has_scale = mask & 16, has_acc = mask & 32;
            if ((alias == 1 && !has_z1) || (alias == 2 && !has_z2)) continue;
            std::vector<float> want(cells), want_acc(cells), out(cells), b1 = z1, b2 = z2, acc = acc0;
            const float b = has_b ? 0.3f : 0.f;
            plain(g, has_val ? val.data() : nullptr, x, k, -0.7f, b, has_z1 ? z1.data() : nullptr, -2.f, has_z2 ? z2.data() : nullptr, -1.f,
                  has_scale ? scale.data() : nullptr, has_acc ? acc0.data() : nullptr, 0.62f, want, want_acc);
            float *dst = alias == 1 ? b1.data() : alias == 2 ? b2.data() : out.data();
            const int rc = cogdl_host_csr_filter_step(g.rowptr.data(), g.colind.data(), has_val ? val.data() : nullptr, x.data(), dst, kNodes, k,
                                                      nnz, 0, -0.7f, b, has_z1 ? b1.data() : nullptr, -2.f, has_z2 ? b2.data() : nullptr, -1.f,
                                                      has_scale ? scale.data() : nullptr, has_acc ? acc.data() : nullptr, 0.62f);
            char name[96];
            std::snprintf(name, sizeof name, "k %lld mask %d alias %d", (long long)k, mask, alias);
            if (rc != 0) failed |= (std::printf("%s: status %d\n", name, rc), 1);
            failed |= same(name, alias == 1 ? b1 : alias == 2 ? b2 : out, want);
            if (has_acc) failed |= same(name, acc, want_acc);
            ++runs;
        }
    std::printf("width %-3lld %d runs %s\n", (long long)k, runs, failed ? "FAILED" : "ok");
    return failed;
}

int expect(const char *what, int rc, int want) {
    std::printf("%-34s status %d\n", what, rc);
    return rc != want;
}

int refusals(const Csr &g) {
    const int64_t k = 5, nnz = (int64_t)g.colind.size();
    const size_t cells = (size_t)(kNodes * k);
    std::vector<float> x = noise(cells, 1), out(cells), acc = noise(cells, 2), wide(cells + 4);
    auto call = [&](const int32_t *rowptr, const int32_t *colind, float *o, const float *z1, float *a) {
        return cogdl_host_csr_filter_step(rowptr, colind, nullptr, x.data(), o, kNodes, k, nnz, 0, 1.f, 0.f, z1, 1.f, nullptr, 0.f, nullptr, a, 1.f);
    };
    int failed = 0;
    failed |= expect("plain call", call(g.rowptr.data(), g.colind.data(), out.data(), nullptr, acc.data()), COGDL_HOST_OK);
    failed |= expect("out is x", call(g.rowptr.data(), g.colind.data(), x.data(), nullptr, nullptr), COGDL_HOST_EINVAL);
    failed |= expect("acc is x", call(g.rowptr.data(), g.colind.data(), out.data(), nullptr, x.data()), COGDL_HOST_EINVAL);
    failed |= expect("out is acc", call(g.rowptr.data(), g.colind.data(), out.data(), nullptr, out.data()), COGDL_HOST_EINVAL);
    failed |= expect("z1 shifted against out", call(g.rowptr.data(), g.colind.data(), wide.data(), wide.data() + 4, nullptr), COGDL_HOST_EINVAL);
    std::vector<int32_t> bad_ptr = g.rowptr, bad_col = g.colind;
    bad_ptr[3] = bad_ptr[4] + 1;  // a row that ends before it starts
    failed |= expect("malformed rowptr", call(bad_ptr.data(), g.colind.data(), out.data(), nullptr, nullptr), COGDL_HOST_ERANGE);
    for (size_t e = 5; e < bad_col.size(); e += 9) bad_col[e] = e % 2 ? (int32_t)kNodes : -1 - (int32_t)e;
    failed |= expect("column ids outside [0, n)", call(g.rowptr.data(), bad_col.data(), out.data(), nullptr, nullptr), COGDL_HOST_ERANGE);
    failed |= expect("n == 0", cogdl_host_csr_filter_step(nullptr, nullptr, nullptr, nullptr, nullptr, 0, k, 0, 0, 1.f, 0.f, nullptr, 0.f, nullptr, 0.f,
                                                          nullptr, nullptr, 0.f), COGDL_HOST_OK);
    return failed;
}

}  // namespace

int main() {
    const Csr g = make_structure();
    int failed = 0;
    for (int64_t k : {1, 7, 64, 65}) failed |= run_width(g, k);
    failed |= refusals(g);
    std::printf(failed ? "FAILED\n" : "ok\n");
    return failed;
}
