// host_netsmf.cpp -- the host twin of csrc/netsmf.hip: NetSMF path sampling.  The law of a sample is netsmf_law.h's, the
// same functions the kernel runs, so for equal inputs and seed both return the same arrays.  OpenMP over the output
// positions; the result does not depend on the number of threads.  No HIP.
#include <cstdint>

#include "../../include/cogdl_host.h"
#include "netsmf_law.h"

namespace ns = cogdl_netsmf;

extern "C" int cogdl_host_netsmf_sample(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                        int64_t first_sample, int64_t n_samples, int window, uint64_t seed, int32_t *out_row,
                                        int32_t *out_col, int *flags) {
    const int rc = ns::args_status(indptr, indices, num_nodes, num_edges, first_sample, n_samples, window, out_row, out_col, flags);
    if (rc != ns::kArgsOk) return rc == ns::kArgsRange ? COGDL_HOST_ERANGE : COGDL_HOST_EINVAL;
    const cogdl_walk::Graph g = {indptr, indices, num_nodes, num_edges};
    const int64_t total = n_samples * window;
    int all = 0;
#pragma omp parallel for schedule(static) reduction(| : all) if (total >= 4096)
    for (int64_t j = 0; j < total; ++j) {
        const int64_t r = j / n_samples + 1, s = first_sample + j % n_samples;
        int err = 0;
        const ns::Pair p = ns::sample(g, seed, s, r, err);
        out_row[j] = p.u;
        out_col[j] = p.v;
        all |= err;
    }
    *flags = all;
    return COGDL_HOST_OK;
}
