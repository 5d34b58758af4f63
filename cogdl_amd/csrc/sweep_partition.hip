// sweep_partition.hip -- which XCD the rows of a sweep layout run on (cogdl_amd/sweepplan.py: deal_by_xcd).  The law --
// counts, scores, buckets, keys, quotas -- is sweep_partition_law.h's, shared with the host twin (host_sweep_partition.cpp).
// One round is five launches on the caller's stream, nothing is read back:
//   clear      the counts cnt [n_src, P], the buckets' sizes and their fill cursors
//   count      one thread per row: cnt[ind[e], label] += 1 (atomics: a sum)
//   candidate  one thread per row: its candidate word; the size of its bucket += 1 (atomics: a sum)
//   offsets    one workgroup: exclusive scan of the sizes, every bucket's quota
//   fill       one thread per row: a candidate's key goes to a free place of its bucket (atomic cursor: the ORDER inside a
//              bucket differs from launch to launch, the SET does not)
//   accept     one thread per place: rank = keys of its bucket below its own (keys are distinct: the rank does not depend on
//              the places); rank < quota: the row takes its best part.  A thread writes its own row's label and reads no
//              other row's.
// The rank costs a bucket's size squared reads out of L2; buckets are (from, to, edge count) classes, a few hundred candidates
// each on the benchmark's graph, and the law gives a bucket beyond kMaxBucket candidates a quota of zero: at most kMaxBucket
// reads per candidate and round on any graph.
#include "common.h"
#include "sweep_partition_law.h"

namespace cogdl {
namespace sp = cogdl_sweep_part;

struct PartScratch {
    int32_t *cnt;      // [n_src * P]
    int32_t *size;     // [B]      } one range, cleared together with cnt
    int32_t *cursor;   // [B]      }
    int32_t *off;      // [B + 1]
    int32_t *quota;    // [B]
    int32_t *cand;     // [n_rows]
    uint64_t *keys;    // [n_rows]
};

static size_t part_words(int64_t n_rows, int64_t n_src, int P) {
    const int64_t B = sp::n_buckets(P);
    size_t w = (size_t)n_src * P + 4 * (size_t)B + 1 + (size_t)n_rows;
    return (w + 1) & ~(size_t)1;  // (the keys behind them are 8-byte words)
}

__global__ __launch_bounds__(256) void part_count_kernel(const int32_t *__restrict__ ptr, const int32_t *__restrict__ ind,
                                                         const int32_t *__restrict__ labels, int32_t *__restrict__ cnt,
                                                         int64_t n_rows, int64_t n_src, int P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int32_t label = labels[i];
    for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e) {
        const int32_t s = ind[e];
        if (sp::counted(s, label, n_src, P)) atomicAdd(&cnt[(int64_t)s * P + label], 1);
    }
}

__global__ __launch_bounds__(256) void part_candidate_kernel(const int32_t *__restrict__ ptr, const int32_t *__restrict__ ind,
                                                             const int32_t *__restrict__ labels, const int32_t *__restrict__ cnt,
                                                             int32_t *__restrict__ cand, int32_t *__restrict__ size,
                                                             int64_t n_rows, int64_t n_src, int P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int32_t c = sp::candidate(ptr, ind, cnt, labels, i, n_src, P);
    cand[i] = c;
    if (c != sp::kStays) atomicAdd(&size[sp::bucket(labels[i], sp::cand_part(c), ptr[i + 1] - ptr[i], P)], 1);
}

// One workgroup of 1024 threads: thread t owns the `per` consecutive buckets from t * per on.
__global__ __launch_bounds__(1024) void part_offsets_kernel(const int32_t *__restrict__ size, int32_t *__restrict__ off,
                                                            int32_t *__restrict__ quota, int B, int per, int P) {
    __shared__ int32_t partial[1024];
    const int t = threadIdx.x;
    const int lo = min(t * per, B), hi = min(lo + per, B);
    int32_t sum = 0;
    for (int b = lo; b < hi; ++b) {
        sum += size[b];
        quota[b] = sp::quota(size[b], size[sp::mirror(b, P)]);
    }
    partial[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // (Hillis-Steele, inclusive)
        const int32_t v = t >= d ? partial[t - d] : 0;
        __syncthreads();
        partial[t] += v;
        __syncthreads();
    }
    int32_t at = partial[t] - sum;
    for (int b = lo; b < hi; ++b) {
        off[b] = at;
        at += size[b];
    }
    if (t == 1023) off[B] = partial[t];
}

__global__ __launch_bounds__(256) void part_fill_kernel(const int32_t *__restrict__ ptr, const int32_t *__restrict__ labels,
                                                        const int32_t *__restrict__ cand, const int32_t *__restrict__ off,
                                                        int32_t *__restrict__ cursor, uint64_t *__restrict__ keys,
                                                        int64_t n_rows, int P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int32_t c = cand[i];
    if (c == sp::kStays) return;
    const int b = sp::bucket(labels[i], sp::cand_part(c), ptr[i + 1] - ptr[i], P);
    // (size[b] candidates take the places off[b] .. off[b + 1] - 1: at most n_rows places in all)
    keys[off[b] + atomicAdd(&cursor[b], 1)] = sp::key(sp::cand_gain(c), (int)i);
}

__global__ __launch_bounds__(256) void part_accept_kernel(const int32_t *__restrict__ ptr, int32_t *__restrict__ labels,
                                                          const int32_t *__restrict__ cand, const int32_t *__restrict__ off,
                                                          const int32_t *__restrict__ quota, const uint64_t *__restrict__ keys,
                                                          int64_t n_rows, int B, int P) {
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= n_rows || at >= off[B]) return;
    const uint64_t mine = keys[at];
    const int row = sp::key_row(mine);  // (a row the fill kernel wrote: < n_rows, a candidate)
    const int32_t c = cand[row];
    const int b = sp::bucket(labels[row], sp::cand_part(c), ptr[row + 1] - ptr[row], P);
    const int32_t q = quota[b];
    int32_t rank = 0;
    for (int32_t j = off[b]; j < off[b + 1] && rank < q; ++j) rank += keys[j] < mine ? 1 : 0;
    if (rank < q) labels[row] = sp::cand_part(c);
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_sweep_partition_workspace_bytes(int64_t n_rows, int64_t n_src, int n_parts) {
    if (sp::sizes_status(n_rows, 0, n_src, n_parts, 0) != 0) return 0;
    return 4 * part_words(n_rows, n_src, n_parts) + 8 * (size_t)n_rows;
}

extern "C" int cogdl_hip_sweep_partition(const int32_t *ptr, const int32_t *ind, int64_t n_rows, int64_t nnz, int64_t n_src,
                                         int n_parts, int rounds, int32_t *labels, void *workspace, size_t workspace_bytes,
                                         void *stream) {
    const int rc = sp::sizes_status(n_rows, nnz, n_src, n_parts, rounds);
    if (rc != 0) return rc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (n_rows == 0 || rounds == 0) return COGDL_HIP_OK;
    if (!ptr || !labels || (nnz > 0 && !ind) || !workspace) return COGDL_HIP_EINVAL;
    if (workspace_bytes < cogdl_hip_sweep_partition_workspace_bytes(n_rows, n_src, n_parts)) return COGDL_HIP_EINVAL;
    if (!aligned_to(workspace, 8) || !aligned_to(ptr, 4) || !aligned_to(ind, 4) || !aligned_to(labels, 4)) return COGDL_HIP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int P = n_parts;
    const int B = (int)sp::n_buckets(P);
    PartScratch w;
    w.cnt = (int32_t *)workspace;
    w.size = w.cnt + n_src * P;
    w.cursor = w.size + B;
    w.off = w.cursor + B;
    w.quota = w.off + B + 1;
    w.cand = w.quota + B;
    w.keys = (uint64_t *)((int32_t *)workspace + part_words(n_rows, n_src, P));
    const unsigned blocks = (unsigned)((n_rows + 255) / 256);
    for (int round = 0; round < rounds; ++round) {
        const hipError_t e = fill_u32_async(w.cnt, 0u, (size_t)n_src * P + 2 * (size_t)B, s);
        if (e != hipSuccess) {
            g_last_hip_error = (int)e;
            return COGDL_HIP_ELAUNCH;
        }
        hipLaunchKernelGGL(part_count_kernel, dim3(blocks), dim3(256), 0, s, ptr, ind, labels, w.cnt, n_rows, n_src, P);
        hipLaunchKernelGGL(part_candidate_kernel, dim3(blocks), dim3(256), 0, s, ptr, ind, labels, w.cnt, w.cand, w.size, n_rows,
                           n_src, P);
        hipLaunchKernelGGL(part_offsets_kernel, dim3(1), dim3(1024), 0, s, w.size, w.off, w.quota, B, (B + 1023) / 1024, P);
        hipLaunchKernelGGL(part_fill_kernel, dim3(blocks), dim3(256), 0, s, ptr, labels, w.cand, w.off, w.cursor, w.keys, n_rows, P);
        hipLaunchKernelGGL(part_accept_kernel, dim3(blocks), dim3(256), 0, s, ptr, labels, w.cand, w.off, w.quota, w.keys, n_rows,
                           B, P);
        const int st = launch_status();
        if (st != COGDL_HIP_OK) return st;
    }
    return COGDL_HIP_OK;
}
