// netsmf.hip -- NetSMF path sampling on a GPU-resident CSR graph (int64 indptr / indices) for gfx950:
//   cogdl_hip_netsmf_sample   pairs (u', v') of the samples first .. first + n - 1, for every path length r = 1 .. T
//                             (the interpreted loop of cogdl/models/emb/netsmf.py:134-159)
// The law of a sample lives in netsmf_law.h, which the host twin (host_netsmf.cpp) includes too: for equal inputs and seed
// both return the same arrays.
//
// Shape.  A sample is a binary search in indptr (log2 N dependent loads that hit in L2: its top levels are shared by all
// lanes) and then r - 1 moves of two dependent random loads each (the indptr pair, one indices entry) around ten Philox
// rounds: bound by memory latency like the walks of walk.hip, so throughput is samples in flight.  One lane owns one
// (s, r); the index j = (r - 1) * n_samples + (s - first) puts the pairs of one r next to each other, so the 64 lanes of a
// wave share r (but for the one wave that straddles a boundary) and run the same number of dependent gathers -- with r
// varying inside a wave every wave would last as long as its r = T lane, T / mean(r) ~ 2x the work.  Consecutive lanes also
// take consecutive entries e, so the reads of indices[e] and both stores are coalesced; no LDS staging is needed.
// No LDS and a register count that admits 8 waves per SIMD (34 VGPRs), blocks of 256: the
// occupancy a latency-bound gather wants.  The grid is a fixed number of blocks per CU striding over the pairs.
// Error flags are raised as in walk.hip, with raise_flags (common.h).
#include "common.h"

#include "netsmf_law.h"

namespace cogdl {

namespace ns = cogdl_netsmf;

constexpr int kNetsmfBlock = 256;
constexpr int64_t kNetsmfMaxBlocks = 256 * 8;  // 8 blocks of 4 waves per CU: every SIMD's 8 wave slots

__global__ __launch_bounds__(kNetsmfBlock) void netsmf_sample_kernel(cogdl_walk::Graph g, int64_t first_sample,
                                                                     int64_t n_samples, int64_t total, uint64_t seed,
                                                                     int32_t *__restrict__ out_row,
                                                                     int32_t *__restrict__ out_col, int *__restrict__ flags) {
    const int64_t stride = (int64_t)gridDim.x * kNetsmfBlock;
    int err = 0;
    for (int64_t j = (int64_t)blockIdx.x * kNetsmfBlock + threadIdx.x; j < total; j += stride) {
        const int64_t r = j / n_samples + 1, s = first_sample + j % n_samples;
        const ns::Pair p = ns::sample(g, seed, s, r, err);
        out_row[j] = p.u;
        out_col[j] = p.v;
    }
    raise_flags(flags, err);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" int cogdl_hip_netsmf_sample(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                       int64_t first_sample, int64_t n_samples, int window, uint64_t seed, int32_t *out_row,
                                       int32_t *out_col, int *flags, void *stream) {
    const int rc = ns::args_status(indptr, indices, num_nodes, num_edges, first_sample, n_samples, window, out_row, out_col, flags);
    if (rc != ns::kArgsOk) return rc == ns::kArgsRange ? COGDL_HIP_ERANGE : COGDL_HIP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cleared = clear_flags_async(flags, s);
    if (cleared != COGDL_HIP_OK || n_samples == 0) return cleared;
    const cogdl_walk::Graph g = {indptr, indices, num_nodes, num_edges};
    const int64_t total = n_samples * window;
    int64_t blocks = (total + kNetsmfBlock - 1) / kNetsmfBlock;
    if (blocks > kNetsmfMaxBlocks) blocks = kNetsmfMaxBlocks;
    hipLaunchKernelGGL(netsmf_sample_kernel, dim3((unsigned)blocks), dim3(kNetsmfBlock), 0, s, g, first_sample, n_samples, total,
                       seed, out_row, out_col, flags);
    return launch_status();
}
