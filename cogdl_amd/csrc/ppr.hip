// ppr.hip -- top-k personalised PageRank ("forward push") on a GPU-resident CSR graph (int64 indptr / indices) for gfx950:
//   cogdl_hip_ppr_topk   for every source the topk largest entries of its approximate PPR vector
//                        (the contract of cogdl/utils/ppr_utils.py:8-48, made deterministic: include/cogdl_hip.h)
// The arithmetic (fixed point, quantum 2^-62), the push rule and the output order live in ppr_fixed.h, which the host twin
// (host_ppr.cpp) includes too: for equal inputs both return the same arrays.
//
// Shape.  Sources are independent: a persistent grid of workgroups takes sources off one device-wide counter.  Per source a
// workgroup keeps an open-addressed table node -> (r, p) (linear probing, load <= 1/2), the list of occupied slots, and
// two frontier lists.  A round is
//   A  one thread per frontier node: res = exchange(r, 0); p += res; share = mulhi64(res, beta) / deg      | barrier
//   B  the rows of the frontier go out: r[v] += share by a 64-bit integer atomic; the ONE addition that makes v
//      pushable appends v to the next frontier (ppr_fixed.h: crossed)                                        | barrier
// Integer additions commute, so the schedule inside a round cannot show in r or p; slot numbers and list orders do depend
// on it, and nothing that is returned depends on them (the selection orders by (score, node id)).
// Rows of fewer than kHubDeg entries are walked by groups of 16 lanes, one row per group at a time; longer rows by the
// whole workgroup, 256 entries per step.
// The table lives in LDS when it has at most ppr_fixed.h's kLdsCap slots (68 KiB with its lists), otherwise in a slice of
// the caller's workspace; in both cases a source cleans exactly the slots it occupied, so the cost of a source is
// proportional to what it touched, not to the table.
// Every loop is bounded: probes by the table size, rounds by Params::max_rounds, sources by S; an id or a row outside
// its range, a full table or the round cap end the source with a flag and an empty output row.
// Table words are read and written with relaxed agent-scope atomic loads / stores: the 64-bit atomics execute in L2, and
// a plain load could be served a stale line from the CU's vector cache.
#include "common.h"

#include "ppr_fixed.h"

namespace cogdl {

namespace pp = cogdl_ppr;

constexpr int kPprBlock = 256;
constexpr int kPprGroup = 16;     // lanes that walk one ordinary row
constexpr int kHubDeg = 1024;     // rows from this length on are walked by the whole workgroup
constexpr int kHubList = 64;      // hub rows remembered per round; further ones take the ordinary path
constexpr int kPprGridLds = 1024;
constexpr int kPprGridGlobal = 256;
constexpr size_t kPprWsHeader = 256;
constexpr size_t kPprWsLimit = (size_t)2 << 30;

template <typename T> __device__ __forceinline__ T ld(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T> __device__ __forceinline__ void st(T *p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct PprTable {
    unsigned long long *keys;  // node id + 1, 0 = empty
    unsigned long long *r, *p;
    uint32_t *touched, *fr0, *fr1;
    unsigned long long *shares;
};

struct PprState {
    int n_touched, nf, n_hub, err_a, err_b;  // err_a is written in phase A only, err_b elsewhere
    int hub[kHubList];
    unsigned long long next_source;
    unsigned long long red_p[kPprBlock / kWave];
    long long red_k[kPprBlock / kWave];
};

constexpr unsigned long long kEmpty = 0ull;

// Bytes of one table with its lists, and where the pieces start (the same carving in LDS and in the workspace).
__host__ __device__ inline size_t ppr_table_bytes(int64_t cap) {
    return (size_t)cap * 24 + (size_t)(cap / 2) * (3 * 4 + 8);
}
__device__ __forceinline__ PprTable ppr_carve(unsigned char *base, int64_t cap) {
    PprTable t;
    const size_t mt = (size_t)cap / 2;
    t.keys = (unsigned long long *)base;
    t.r = t.keys + cap;
    t.p = t.r + cap;
    t.shares = t.p + cap;
    t.touched = (uint32_t *)(t.shares + mt);
    t.fr0 = t.touched + mt;
    t.fr1 = t.fr0 + mt;
    return t;
}

// Slot of v, inserted if new.  Bounded by the table size; the load limit keeps it short.
__device__ __forceinline__ int64_t ppr_slot_of(const PprTable &t, PprState *st_, const pp::Params &P, int64_t v) {
    const uint64_t mask = (uint64_t)P.cap - 1;
    const unsigned long long key = (unsigned long long)v + 1;
    uint64_t h = pp::hash_id(v) & mask;
    for (int64_t probe = 0; probe < P.cap; ++probe, h = (h + 1) & mask) {
        unsigned long long k = ld(&t.keys[h]);
        if (k == key) return (int64_t)h;
        if (k == kEmpty) {
            k = atomicCAS(&t.keys[h], kEmpty, key);
            if (k == kEmpty) {
                const int idx = atomicAdd(&st_->n_touched, 1);
                if (idx < P.max_touched)
                    st(&t.touched[idx], (uint32_t)h);
                else
                    atomicOr(&st_->err_b, pp::kTableFull);  // (the slot stays valid; the source ends after this round)
                return (int64_t)h;
            }
            if (k == key) return (int64_t)h;
        }
    }
    atomicOr(&st_->err_b, pp::kTableFull);
    return -1;
}

// One entry of a pushed row: the share goes to v, and v joins the next frontier if this addition made it pushable.
__device__ __forceinline__ void ppr_give(const pp::Graph &g, const PprTable &t, PprState *st_, const pp::Params &P, int64_t v,
                                         unsigned long long sh, uint32_t *next) {
    if (!pp::valid_id(g, v)) {
        atomicOr(&st_->err_b, pp::kBadNeighbour);
        return;
    }
    int64_t vlo, vhi;
    if (!pp::row_of(g, v, vlo, vhi)) {
        atomicOr(&st_->err_b, pp::kBadRowPtr);
        return;
    }
    const int64_t h = ppr_slot_of(t, st_, P, v);
    if (h < 0) return;
    const unsigned long long old = atomicAdd(&t.r[h], sh);
    if (pp::crossed(old, old + sh, P.thr, vhi - vlo)) {
        const int k = atomicAdd(&st_->nf, 1);
        if (k < P.max_touched) st(&next[k], (uint32_t)h);
    }
}

template <bool LDS>
__global__ __launch_bounds__(kPprBlock) void ppr_topk_kernel(pp::Graph g, const int64_t *__restrict__ sources, int64_t n_sources,
                                                             pp::Params P, int64_t topk, int64_t *__restrict__ nbr,
                                                             float *__restrict__ val, int32_t *__restrict__ count,
                                                             int32_t *__restrict__ stats, int *__restrict__ flags,
                                                             unsigned char *__restrict__ ws) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ PprState S;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    unsigned long long *counter = (unsigned long long *)ws;
    PprTable t;
    if constexpr (LDS) {
        t = ppr_carve(smem, P.cap);
        for (int64_t i = tid; i < P.cap; i += kPprBlock) {
            t.keys[i] = kEmpty;
            t.r[i] = 0;
            t.p[i] = 0;
        }
    } else {
        t = ppr_carve(ws + kPprWsHeader + (size_t)blockIdx.x * ppr_table_bytes(P.cap), P.cap);  // cleared by the entry point
    }
    int all_err = 0;
    for (int64_t guard = 0; guard < n_sources; ++guard) {  // (a workgroup takes at most every source)
        __syncthreads();
        if (tid == 0) {
            S.next_source = atomicAdd(counter, 1ull);
            S.n_touched = 0;
            S.nf = 0;
            S.n_hub = 0;
            S.err_a = S.err_b = 0;
        }
        __syncthreads();
        const unsigned long long si = S.next_source;
        if (si >= (unsigned long long)n_sources) break;
        const int64_t s = sources[si];
        if (tid == 0) {
            if (!pp::valid_id(g, s)) {
                S.err_b = pp::kBadSource;
            } else {
                const uint64_t h = pp::hash_id(s) & ((uint64_t)P.cap - 1);
                st(&t.keys[h], (unsigned long long)s + 1);
                st(&t.r[h], (unsigned long long)P.r0);
                st(&t.touched[0], (uint32_t)h);
                st(&t.fr0[0], (uint32_t)h);
                S.n_touched = 1;
            }
        }
        __syncthreads();
        int nf = S.err_b ? 0 : 1;
        int64_t rounds = 0;
        while (nf > 0) {
            uint32_t *cur = (rounds & 1) ? t.fr1 : t.fr0, *next = (rounds & 1) ? t.fr0 : t.fr1;
            if (rounds >= P.max_rounds) {
                if (tid == 0) S.err_b |= pp::kRoundCap;
                break;
            }
            // A: residual -> score; the share of the round; hub rows noted
            for (int i = tid; i < nf; i += kPprBlock) {
                const uint32_t h = ld(&cur[i]);
                const int64_t u = (int64_t)ld(&t.keys[h]) - 1;
                int64_t lo, hi;
                if (!pp::row_of(g, u, lo, hi)) atomicOr(&S.err_a, pp::kBadRowPtr);
                const unsigned long long res = atomicExch(&t.r[h], 0ull);
                st(&t.p[h], ld(&t.p[h]) + res);
                unsigned long long sh = pp::share(res, P.beta, hi - lo);
                if (sh != 0 && hi - lo >= kHubDeg) {
                    const int k = atomicAdd(&S.n_hub, 1);
                    if (k < kHubList) {
                        S.hub[k] = i;
                        sh |= 1ull << 63;  // marked: phase B's ordinary pass skips it (a share is below 2^62)
                    }
                }
                st(&t.shares[i], sh);
            }
            if (tid == 0) S.nf = 0;
            __syncthreads();
            if (S.err_a) break;  // (phase B does not write err_a)
            // B: ordinary rows, one per group of 16 lanes
            for (int i = tid / kPprGroup; i < nf; i += kPprBlock / kPprGroup) {
                const unsigned long long sh = ld(&t.shares[i]);
                if (sh == 0 || (sh >> 63)) continue;
                int64_t lo, hi;
                pp::row_of(g, (int64_t)ld(&t.keys[ld(&cur[i])]) - 1, lo, hi);
                for (int64_t j = lo + tid % kPprGroup; j < hi; j += kPprGroup) ppr_give(g, t, &S, P, g.indices[j], sh, next);
            }
            // B: hub rows, the whole workgroup per row
            const int n_hub = S.n_hub < kHubList ? S.n_hub : kHubList;
            for (int k = 0; k < n_hub; ++k) {
                const int i = S.hub[k];
                const unsigned long long sh = ld(&t.shares[i]) & ~(1ull << 63);
                int64_t lo, hi;
                pp::row_of(g, (int64_t)ld(&t.keys[ld(&cur[i])]) - 1, lo, hi);
                for (int64_t j = lo + tid; j < hi; j += kPprBlock) ppr_give(g, t, &S, P, g.indices[j], sh, next);
            }
            __syncthreads();
            nf = S.nf < P.max_touched ? S.nf : (int)P.max_touched;
            const int err_b = S.err_b;
            if (tid == 0) S.n_hub = 0;  // (read before the barrier above, added to after the one below)
            __syncthreads();
            if (err_b) break;
            ++rounds;
        }
        __syncthreads();
        const int err = S.err_a | S.err_b;
        const int n_t = S.n_touched < P.max_touched ? S.n_touched : (int)P.max_touched;
        all_err |= err;
        // selection: the k-th pass finds the first entry in output order that comes after the (k-1)-th
        int64_t n_out = 0;
        if (!err) {
            unsigned long long prev_p = ~0ull;
            long long prev_k = -1;
            const int64_t k_max = topk < n_t ? topk : n_t;
            for (; n_out < k_max; ++n_out) {
                unsigned long long best_p = 0;
                long long best_k = -1;
                for (int i = tid; i < n_t; i += kPprBlock) {
                    const uint32_t h = ld(&t.touched[i]);
                    const unsigned long long p = ld(&t.p[h]);
                    if (p == 0) continue;
                    const long long k = (long long)ld(&t.keys[h]) - 1;
                    if (!pp::before(prev_p, prev_k, p, k)) continue;
                    if (best_p == 0 || pp::before(p, k, best_p, best_k)) {
                        best_p = p;
                        best_k = k;
                    }
                }
#pragma unroll
                for (int o = kWave / 2; o > 0; o >>= 1) {
                    const unsigned long long op = __shfl_xor(best_p, o, kWave);
                    const long long ok = __shfl_xor(best_k, o, kWave);
                    if (op != 0 && (best_p == 0 || pp::before(op, ok, best_p, best_k))) {
                        best_p = op;
                        best_k = ok;
                    }
                }
                if (lane == 0) {
                    S.red_p[wave] = best_p;
                    S.red_k[wave] = best_k;
                }
                __syncthreads();
                best_p = S.red_p[0];
                best_k = S.red_k[0];
#pragma unroll
                for (int w = 1; w < kPprBlock / kWave; ++w) {
                    const unsigned long long op = S.red_p[w];
                    const long long ok = S.red_k[w];
                    if (op != 0 && (best_p == 0 || pp::before(op, ok, best_p, best_k))) {
                        best_p = op;
                        best_k = ok;
                    }
                }
                __syncthreads();
                if (best_p == 0) break;  // (uniform: every thread read the same four pairs)
                if (tid == 0) {
                    nbr[si * topk + n_out] = best_k;
                    val[si * topk + n_out] = pp::to_f32(best_p);
                }
                prev_p = best_p;
                prev_k = best_k;
            }
        }
        for (int64_t j = n_out + tid; j < topk; j += kPprBlock) {
            nbr[si * topk + j] = -1;
            val[si * topk + j] = 0.0f;
        }
        if (tid == 0) {
            count[si] = (int32_t)n_out;
            if (stats) {
                stats[2 * si] = (int32_t)rounds;
                stats[2 * si + 1] = n_t;
            }
        }
        // the source cleans what it occupied (everything, if the touched list is not complete)
        if (err & pp::kTableFull) {
            for (int64_t i = tid; i < P.cap; i += kPprBlock) {
                st(&t.keys[i], kEmpty);
                st(&t.r[i], 0ull);
                st(&t.p[i], 0ull);
            }
        } else {
            for (int i = tid; i < n_t; i += kPprBlock) {
                const uint32_t h = ld(&t.touched[i]);
                st(&t.keys[h], kEmpty);
                st(&t.r[h], 0ull);
                st(&t.p[h], 0ull);
            }
        }
    }
    if (all_err && lane == 0) atomicOr(flags, all_err);
}

static int ppr_grid(const pp::Params &P, int64_t n_sources) {
    const bool lds = P.cap <= pp::kLdsCap;
    int64_t blocks = lds ? kPprGridLds : kPprGridGlobal;
    if (!lds) {
        const int64_t fit = (int64_t)((kPprWsLimit - kPprWsHeader) / ppr_table_bytes(P.cap));
        blocks = std::max<int64_t>(1, std::min(blocks, fit));
    }
    return (int)std::max<int64_t>(1, std::min(blocks, n_sources));
}

}  // namespace cogdl

using namespace cogdl;

extern "C" size_t cogdl_hip_ppr_topk_workspace_bytes(int64_t num_nodes, int64_t num_edges, int64_t max_source_degree,
                                                     double alpha, double eps, int64_t n_sources) {
    pp::Params P;
    if (n_sources < 0 || pp::make_params(alpha, eps, num_nodes, num_edges, max_source_degree, &P) != 0) return 0;
    if (P.cap <= pp::kLdsCap) return kPprWsHeader;
    return kPprWsHeader + (size_t)ppr_grid(P, n_sources) * ppr_table_bytes(P.cap);
}

extern "C" int cogdl_hip_ppr_topk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                                  const int64_t *sources, int64_t n_sources, int64_t max_source_degree, double alpha,
                                  double eps, int64_t topk, int64_t *nbr, float *val, int32_t *count, int32_t *stats,
                                  int *flags, void *ws, size_t ws_bytes, void *stream) {
    if (num_nodes < 0 || num_edges < 0 || n_sources < 0 || topk < 1 || !flags || !ws) return COGDL_HIP_EINVAL;
    if (n_sources > 0 && (!indptr || !sources || !nbr || !val || !count)) return COGDL_HIP_EINVAL;
    if (num_edges > 0 && !indices) return COGDL_HIP_EINVAL;
    pp::Params P;
    const int prc = pp::make_params(alpha, eps, num_nodes, num_edges, max_source_degree, &P);
    if (prc != 0) return prc == 1 ? COGDL_HIP_EINVAL : COGDL_HIP_ERANGE;
    if (!aligned_to(ws, 16)) return COGDL_HIP_EALIGN;
    const bool lds = P.cap <= pp::kLdsCap;
    const int grid = ppr_grid(P, n_sources);
    const size_t table = ppr_table_bytes(P.cap);
    const size_t need = kPprWsHeader + (lds ? 0 : (size_t)grid * table);
    if (ws_bytes < need) return COGDL_HIP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = fill_u32_async(flags, 0u, 1, s);
    if (e == hipSuccess) e = fill_u32_async(ws, 0u, (n_sources == 0 ? kPprWsHeader : need) / 4, s);  // counter; tables empty
    if (n_sources == 0) {
        if (e != hipSuccess) {
            g_last_hip_error = (int)e;
            return COGDL_HIP_ELAUNCH;
        }
        return COGDL_HIP_OK;
    }
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return COGDL_HIP_ELAUNCH;
    }
    const pp::Graph g = {indptr, indices, num_nodes, num_edges};
    if (lds) {
        const size_t lds_bytes = ppr_table_bytes(P.cap);
        e = hipFuncSetAttribute((const void *)ppr_topk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) {
            g_last_hip_error = (int)e;
            return COGDL_HIP_ELAUNCH;
        }
        hipLaunchKernelGGL(ppr_topk_kernel<true>, dim3(grid), dim3(kPprBlock), lds_bytes, s, g, sources, n_sources, P, topk, nbr, val,
                           count, stats, flags, (unsigned char *)ws);
    } else {
        hipLaunchKernelGGL(ppr_topk_kernel<false>, dim3(grid), dim3(kPprBlock), 0, s, g, sources, n_sources, P, topk, nbr, val,
                           count, stats, flags, (unsigned char *)ws);
    }
    return launch_status();
}
