// netsmf_law.h -- the path sampling of NetSMF (Qiu et al., WWW'19, algorithm 2; the reference's interpreted loop is
// cogdl/models/emb/netsmf.py:134-159), shared by the HIP kernel (netsmf.hip) and its host twin (host_netsmf.cpp).  Plain
// C++ on top of walk_draw.h: no HIP runtime, no libc beyond <stdint.h>.  Both sides run the SAME functions on the same
// integers, so a sample is the same pair on the GPU and on the host, bit for bit.
//
// Graph: int64 indptr[N + 1] / indices[E], unit weights.  Sample s >= 0 with path length r in [1, T]:
//     e = s mod E;  u = the row that holds entry e (the last u with indptr[u] <= e: binary search, so empty rows are
//                   skipped);  v = indices[e]
//     k = 1 + draw_below(draw(seed, s, r, 0), r)                     uniform on 1 .. r
//     for i = 1 .. r - 1:  d = draw(seed, s, r, i);  steps i <= k - 1 move u, the others move v;
//                          a move from x goes to indices[beg_x + draw_below(d, deg_x)]; at a node without out-neighbours
//                          the walker stays (as step_first_order does)
//     result (u, v)
// Every draw is a pure function of (seed, s, r, i) through Philox4x32-10: counter = (s_lo, s_hi, r, i), key = seed.  Nothing
// depends on launch shape, thread count, batch, or the order in which samples are processed.
//
// Why one pass over the entries is the right unit: on a simple symmetric graph the reference takes every undirected edge
// with a fair orientation flip, which is a uniformly chosen directed CSR entry, so `num_round` rounds of the reference
// have the law of num_round / 2 passes over s = 0 .. E - 1.
//
// Errors.  A neighbour id outside [0, N) raises kBadNeighbour, a row pointer that does not bracket what it should inside
// [0, E] raises kBadRowPtr; the sample then is (-1, -1) and reads nothing more.  Nothing is read out of bounds: every
// index into indices is checked against [0, E) before the load, every id against [0, N) before it indexes indptr.
#pragma once
#include "walk_draw.h"

namespace cogdl_netsmf {

namespace wk = cogdl_walk;

constexpr int kMaxWindow = 256;

struct Pair {
    int32_t u, v;
};

// k of sample (s, r): how the r - 1 steps are split (k - 1 from u, r - k from v)
COGDL_WALK_FN int64_t path_k(uint64_t seed, int64_t s, int64_t r) {
    return 1 + wk::draw_below(wk::draw(seed, s, r, 0u), (uint64_t)r);
}

// The row that holds entry e in [0, E): the last u in [0, N) with indptr[u] <= e.  false + kBadRowPtr when indptr does not
// put e inside that row.  Reads indptr[0 .. N] only, whatever it holds.
COGDL_WALK_FN bool row_holding(const wk::Graph &g, int64_t e, int64_t &u, int &err) {
    int64_t lo = 0, hi = g.n;  // the number of u in [0, N) with indptr[u] <= e lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (g.indptr[mid] <= e) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) {
        err |= wk::kBadRowPtr;
        return false;
    }
    u = lo - 1;
    int64_t beg, deg;
    if (!wk::row_of(g, u, beg, deg, err)) return false;
    if (e < beg || e >= beg + deg) {
        err |= wk::kBadRowPtr;
        return false;
    }
    return true;
}

// One uniform move from x (a valid id); x stays at a node without out-neighbours.  false after an error.
COGDL_WALK_FN bool move(const wk::Graph &g, const wk::Draw &d, int64_t &x, int &err) {
    int64_t beg, deg;
    if (!wk::row_of(g, x, beg, deg, err)) return false;
    if (deg == 0) return true;
    const int64_t y = g.indices[beg + wk::draw_below(d, (uint64_t)deg)];
    if (!wk::valid_id(g, y)) {
        err |= wk::kBadNeighbour;
        return false;
    }
    x = y;
    return true;
}

// Sample (s, r) with g.e > 0, 0 < g.n < 2^31, s >= 0, r >= 1.
COGDL_WALK_FN Pair sample(const wk::Graph &g, uint64_t seed, int64_t s, int64_t r, int &err) {
    const Pair bad = {-1, -1};
    const int64_t e = s % g.e;
    int64_t u;
    if (!row_holding(g, e, u, err)) return bad;
    int64_t v = g.indices[e];
    if (!wk::valid_id(g, v)) {
        err |= wk::kBadNeighbour;
        return bad;
    }
    const int64_t k = path_k(seed, s, r);
    for (int64_t i = 1; i < r; ++i) {
        const wk::Draw d = wk::draw(seed, s, r, (uint32_t)i);
        if (!move(g, d, i <= k - 1 ? u : v, err)) return bad;
    }
    return {(int32_t)u, (int32_t)v};
}

// Position of sample (s, r) in the output of a call over samples first .. first + n - 1: all pairs of one r are contiguous
COGDL_WALK_FN int64_t slot(int64_t s, int64_t r, int64_t first_sample, int64_t n_samples) {
    return (r - 1) * n_samples + (s - first_sample);
}

enum : int { kArgsOk = 0, kArgsInvalid = 1, kArgsRange = 2 };

// The argument check of both entry points (each maps the result to its own status codes).
inline int args_status(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges, int64_t first_sample,
                       int64_t n_samples, int window, const int32_t *out_row, const int32_t *out_col, const int *flags) {
    if (num_nodes < 0 || num_edges < 0 || first_sample < 0 || n_samples < 0 || !flags) return kArgsInvalid;
    if (window < 1 || window > kMaxWindow) return kArgsInvalid;
    if (num_nodes > 0x7fffffff) return kArgsRange;  // (pairs are int32)
    if (n_samples > ((int64_t)1 << 53) || first_sample > ((int64_t)1 << 62)) return kArgsRange;  // window * n_samples < 2^62
    if (n_samples > 0 && (num_edges == 0 || num_nodes == 0 || !indptr || !indices || !out_row || !out_col)) return kArgsInvalid;
    return kArgsOk;
}

}  // namespace cogdl_netsmf
