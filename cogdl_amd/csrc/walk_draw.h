// walk_draw.h -- the random draws, the step functions and the RULE of every kind of random walk, shared by the HIP kernel
// (walk.hip) and its host twin (host_ops.cpp).  Plain C++: no HIP runtime, no libc beyond <stdint.h>; libcogdl_host.so
// includes it and must stay HIP-free.  A rule (FirstOrderRule, Node2vecRule, MetapathRule, at the end of this file) is
// everything a walk kind decides: what a walker carries, what position 0 holds, how it advances, when it counts and what
// it stores at the end.  Each side owns only a scaffold that runs a rule (the tile loop of walk_kernel, the row loop of
// host_ops.cpp), so both run the SAME code on the same integers: a walk is the same array on the GPU and on the host,
// bit for bit.  The argument check of the entry points is here too (walk_args_status).
//
// Randomness.  Every draw is a pure function of (seed, walker w, step i, trial) through Philox4x32-10 (Salmon et al.,
// SC'11; the round function is restated here because philox.h pulls in the HIP runtime):
//     (x, y, z, w) = philox4x32_10(counter = (w_lo, w_hi, i, trial), key = (seed_lo, seed_hi))
//     restart?         x < T,  T = round(restart_p * 2^32) as a 64-bit number, so restart_p = 0 never restarts and
//                      restart_p = 1 (T = 2^32) always does
//     which neighbour  mulhi64((y << 32) | z, deg): uniform over [0, deg) with a bias below deg / 2^64, and able to
//                      return deg - 1
//     accept?          w < A,  A = round(weight / max weight * 2^32) (node2vec rejection sampling; A = 2^32 accepts always)
// The first-order walk and the metapath walk (the first-order draw on a typed row) use trial 0 only.  node2vec uses trials 0 .. max_trials - 1 for its rejection loop and trial
// `max_trials` for the one draw of the exact fallback: r = mulhi64((y << 32) | z, total weight).
// Nothing depends on launch shape, thread count or the order in which walkers are processed.
//
// Weights of node2vec are 32.32 fixed-point integers (the A above): rejection loop and fallback sample exactly the same
// law, proportional to A_back : A_near : A_far, which differs from 1/p : 1 : 1/q by a relative 2^-32 at most.
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define COGDL_WALK_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define COGDL_WALK_FN inline
#endif
#if defined(__clang__)
#define COGDL_WALK_UNROLL _Pragma("unroll")
#else
#define COGDL_WALK_UNROLL
#endif

namespace cogdl_walk {

enum : int {
    kBadStart = 1,      // a start id outside [0, N)
    kBadNeighbour = 2,  // a neighbour id outside [0, N)
    kBadRowPtr = 4      // a row of indptr that is not inside [0, E] or runs backwards
};

constexpr int kDefaultTrials = 256;  // node2vec: rejection trials per step before the exact pass over the row

struct Draw {
    uint32_t x, y, z, w;
};

COGDL_WALK_FN Draw philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    COGDL_WALK_UNROLL
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return {c0, c1, c2, c3};
}

COGDL_WALK_FN Draw draw(uint64_t seed, int64_t walker, int64_t step, uint32_t trial) {
    return philox4x32_10((uint32_t)(uint64_t)walker, (uint32_t)((uint64_t)walker >> 32), (uint32_t)step, trial,
                         (uint32_t)seed, (uint32_t)(seed >> 32));
}

// High 64 bits of a 64 x 64 -> 128-bit product, from 32-bit halves (the same code on both compilers).
COGDL_WALK_FN uint64_t mulhi64(uint64_t a, uint64_t b) {
    const uint64_t al = a & 0xffffffffu, ah = a >> 32, bl = b & 0xffffffffu, bh = b >> 32;
    const uint64_t p0 = al * bl, p1 = al * bh, p2 = ah * bl, p3 = ah * bh;
    const uint64_t mid = (p0 >> 32) + (p1 & 0xffffffffu) + (p2 & 0xffffffffu);
    return p3 + (p1 >> 32) + (p2 >> 32) + (mid >> 32);
}

COGDL_WALK_FN bool draw_restart(const Draw &d, uint64_t restart_t) { return (uint64_t)d.x < restart_t; }
COGDL_WALK_FN int64_t draw_below(const Draw &d, uint64_t n) { return (int64_t)mulhi64(((uint64_t)d.y << 32) | d.z, n); }
COGDL_WALK_FN bool draw_accept(const Draw &d, uint64_t a) { return (uint64_t)d.w < a; }

// round(v * 2^32) for v in [0, 1], host side (called once per call by both libraries, in double)
inline uint64_t fixed32(double v) {
    if (!(v > 0.0)) return 0;
    if (v >= 1.0) return (uint64_t)1 << 32;
    return (uint64_t)(v * 4294967296.0 + 0.5);
}

struct N2vWeights {
    uint64_t back, near, far;  // x == t, t in row x, neither; the largest is 2^32
};
inline N2vWeights n2v_weights(double p, double q) {
    const double wb = 1.0 / p, wf = 1.0 / q;
    double m = 1.0;
    if (wb > m) m = wb;
    if (wf > m) m = wf;
    N2vWeights w = {fixed32(wb / m), fixed32(1.0 / m), fixed32(wf / m)};
    if (w.back == 0) w.back = 1;  // (a weight below 2^-32 of the largest still has to be reachable in the fallback)
    if (w.near == 0) w.near = 1;
    if (w.far == 0) w.far = 1;
    return w;
}

struct Graph {
    const int64_t *indptr, *indices;
    int64_t n, e;
};

// Row `v` (a valid id) -> [beg, beg + deg); false and kBadRowPtr if indptr does not describe a range inside indices.
COGDL_WALK_FN bool row_of(const Graph &g, int64_t v, int64_t &beg, int64_t &deg, int &err) {
    beg = g.indptr[v];
    const int64_t end = g.indptr[v + 1];
    deg = end - beg;
    if (beg < 0 || end > g.e || deg < 0) {
        err |= kBadRowPtr;
        return false;
    }
    return true;
}

COGDL_WALK_FN bool valid_id(const Graph &g, int64_t v) { return (uint64_t)v < (uint64_t)g.n; }

// One step of the first-order walk with restart.  `cur` is returned unchanged (the walker stays) at a node without
// out-neighbours and after any error: a walker that has raised a flag reads nothing more.
COGDL_WALK_FN int64_t step_first_order(const Graph &g, uint64_t seed, int64_t walker, int64_t step, int64_t start,
                                       int64_t cur, uint64_t restart_t, int &err) {
    if (err) return cur;
    const Draw d = draw(seed, walker, step, 0u);
    const int64_t src = draw_restart(d, restart_t) ? start : cur;
    int64_t beg, deg;
    if (!row_of(g, src, beg, deg, err) || deg == 0) return cur;
    const int64_t x = g.indices[beg + draw_below(d, (uint64_t)deg)];
    if (!valid_id(g, x)) {
        err |= kBadNeighbour;
        return cur;
    }
    return x;
}

// Is `t` in row `x` (sorted by column)?  Binary search, 64-bit offsets.
COGDL_WALK_FN bool has_edge(const Graph &g, int64_t x, int64_t t, int &err) {
    int64_t lo, deg;
    if (!row_of(g, x, lo, deg, err)) return false;
    const int64_t end = lo + deg;
    int64_t hi = end;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (g.indices[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && g.indices[lo] == t;
}

// node2vec weight of moving to x with previous node t (x already validated)
COGDL_WALK_FN uint64_t n2v_weight(const Graph &g, const N2vWeights &wt, int64_t x, int64_t t, int &err) {
    if (x == t) return wt.back;
    if (wt.near == wt.far) return wt.near;  // q = 1: the membership test cannot change the weight
    return has_edge(g, x, t, err) ? wt.near : wt.far;
}

// One step of the node2vec walk: previous node t, current node v.  step 1 (no previous node yet) is uniform.
// `fell_back` is set when the exact pass over the row decided the step.
COGDL_WALK_FN int64_t step_node2vec(const Graph &g, uint64_t seed, int64_t walker, int64_t step, int64_t t, int64_t v,
                                    const N2vWeights &wt, int max_trials, int &err, bool &fell_back) {
    fell_back = false;
    if (err) return v;
    int64_t beg, deg;
    if (!row_of(g, v, beg, deg, err) || deg == 0) return v;
    if (step == 1) {
        const int64_t x = g.indices[beg + draw_below(draw(seed, walker, step, 0u), (uint64_t)deg)];
        if (!valid_id(g, x)) {
            err |= kBadNeighbour;
            return v;
        }
        return x;
    }
    for (int trial = 0; trial < max_trials; ++trial) {
        const Draw d = draw(seed, walker, step, (uint32_t)trial);
        const int64_t x = g.indices[beg + draw_below(d, (uint64_t)deg)];
        if (!valid_id(g, x)) {
            err |= kBadNeighbour;
            return v;
        }
        const uint64_t a = n2v_weight(g, wt, x, t, err);
        if (err) return v;
        if (draw_accept(d, a)) return x;
    }
    // exact: total weight of the row, then the inverse CDF at r in [0, total)
    fell_back = true;
    uint64_t total = 0;
    for (int64_t e = beg; e < beg + deg; ++e) {
        const int64_t x = g.indices[e];
        if (!valid_id(g, x)) {
            err |= kBadNeighbour;
            return v;
        }
        total += n2v_weight(g, wt, x, t, err);
        if (err) return v;
    }
    const uint64_t r = (uint64_t)draw_below(draw(seed, walker, step, (uint32_t)max_trials), total);
    uint64_t acc = 0;
    for (int64_t e = beg; e < beg + deg; ++e) {
        const int64_t x = g.indices[e];
        acc += n2v_weight(g, wt, x, t, err);
        if (r < acc) return x;
    }
    return v;  // unreachable: r < total = the final acc
}

// ---------------------------------------------------------------- metapath-constrained walk
// Typed row layout: seg has n * t + 1 entries, indices[seg[v * t + c] .. seg[v * t + c + 1]) are the neighbours of v whose
// type is c (cogdl_amd/operators/walk.py: typed_rows), so "a uniform neighbour of the wanted type" is the first-order
// step on row v * t + c: two dependent loads.  With t == 1 seg is indptr itself.
enum : int {
    kBadStartType = 8,  // a start node whose type is not the first item of its metapath
    kBadPathType = 16   // a wanted type outside [0, t), a metapath id outside [0, n_paths) or a malformed path_off
};

struct TypedGraph {
    const int64_t *seg, *indices;
    int64_t n, e;
    int32_t t;
};

// Where a walker is in its metapath: pat[0 .. period) is the schema without its repeated last item, k = position % period.
struct PathCursor {
    const int32_t *pat;
    int32_t period, k;
};

// Position 0 of walker `start` on metapath `p`: validates the start id, the metapath id, its slice of `pattern` (inside
// [0, path_off[n_paths]]) and, where node_type is given, the start node's type.  On any failure err is raised and the
// cursor points at nothing.  Otherwise the cursor stands at position 1.
COGDL_WALK_FN PathCursor metapath_begin(const TypedGraph &g, const int32_t *node_type, int64_t start, int32_t p,
                                        const int32_t *pattern, const int32_t *path_off, int32_t n_paths, int &err) {
    PathCursor c = {pattern, 1, 0};
    if ((uint64_t)start >= (uint64_t)g.n) {
        err |= kBadStart;
        return c;
    }
    if ((uint32_t)p >= (uint32_t)n_paths) {
        err |= kBadPathType;
        return c;
    }
    const int32_t lo = path_off[p], hi = path_off[p + 1], total = path_off[n_paths];
    if (lo < 0 || hi <= lo || hi > total) {
        err |= kBadPathType;
        return c;
    }
    c.pat = pattern + lo;
    c.period = hi - lo;
    c.k = c.period == 1 ? 0 : 1;
    if (node_type && node_type[start] != c.pat[0]) err |= kBadStartType;
    return c;
}

// The type wanted at the cursor's position, pattern[path_off[p] + i % period]; the cursor moves on to position i + 1.
// Independent of where the walker stands: a kernel can issue it one step ahead.
COGDL_WALK_FN int32_t metapath_next_type(PathCursor &c) {
    const int32_t t = c.pat[c.k];
    c.k = c.k + 1 == c.period ? 0 : c.k + 1;
    return t;
}

// One step of the metapath walk: from `cur` to a uniformly drawn neighbour of type `t` (the draw of the first-order walk).
// -1: the walk has ended (no neighbour of that type: the reference's `break`), had ended before (cur < 0), or a flag is up --
// such a walker reads nothing.
COGDL_WALK_FN int64_t step_metapath(const TypedGraph &g, int32_t t, uint64_t seed, int64_t walker, int64_t step, int64_t cur,
                                    int &err) {
    if (err || cur < 0) return -1;
    if ((uint32_t)t >= (uint32_t)g.t) {
        err |= kBadPathType;
        return -1;
    }
    const int64_t r = cur * g.t + t;
    const int64_t beg = g.seg[r], end = g.seg[r + 1], len = end - beg;
    if (beg < 0 || end > g.e || len < 0) {
        err |= kBadRowPtr;
        return -1;
    }
    if (len == 0) return -1;
    const int64_t x = g.indices[beg + draw_below(draw(seed, walker, step, 0u), (uint64_t)len)];
    if ((uint64_t)x >= (uint64_t)g.n) {
        err |= kBadNeighbour;
        return -1;
    }
    return x;
}

// ---------------------------------------------------------------- the rules
// A rule holds the constants of one call (passed by value to the kernel) and three functions over its per-walker State:
//   begin(st, w, err)             walker w: validates, raises into err -> what position 0 holds
//   advance(st, seed, w, i, err)  -> what position i >= 1 holds
//   finish(st, w)                 stores the walker's side output where the call asked for one
// A scaffold starts a walker with a zeroed State and err = 0 and calls advance for i = 1, 2, .. in order.  Once err is up
// the step functions read nothing more.
struct FirstOrderRule {
    Graph g;
    const int64_t *start;
    uint64_t restart_t;
    struct State {
        int64_t first, cur;
    };
    COGDL_WALK_FN int64_t begin(State &st, int64_t w, int &err) const {
        st.first = st.cur = start[w];
        if (!valid_id(g, st.cur)) err |= kBadStart;
        return st.cur;
    }
    COGDL_WALK_FN int64_t advance(State &st, uint64_t seed, int64_t w, int64_t i, int &err) const {
        return st.cur = step_first_order(g, seed, w, i, st.first, st.cur, restart_t, err);
    }
    COGDL_WALK_FN void finish(const State &, int64_t) const {}
};

struct Node2vecRule {
    Graph g;
    const int64_t *start;
    N2vWeights wt;
    int max_trials;
    int32_t *fallback_steps;  // [n_walkers] or null: steps that the exact pass decided
    struct State {
        int64_t prev, cur;
        int32_t n_fallback;
    };
    COGDL_WALK_FN int64_t begin(State &st, int64_t w, int &err) const {
        st.prev = st.cur = start[w];
        st.n_fallback = 0;
        if (!valid_id(g, st.cur)) err |= kBadStart;
        return st.cur;
    }
    COGDL_WALK_FN int64_t advance(State &st, uint64_t seed, int64_t w, int64_t i, int &err) const {
        bool fell_back;
        const int64_t nxt = step_node2vec(g, seed, w, i, st.prev, st.cur, wt, max_trials, err, fell_back);
        st.n_fallback += fell_back ? 1 : 0;
        st.prev = st.cur;
        return st.cur = nxt;
    }
    COGDL_WALK_FN void finish(const State &st, int64_t w) const {
        if (fallback_steps) fallback_steps[w] = st.n_fallback;
    }
};

// Position 0 holds the start id even where it is refused; after that a walker whose walk has ended, or that raised a flag,
// holds -1 and reads nothing.  The wanted type does not depend on where the walker stands, so it is fetched one step ahead
// (t_next): in the kernel that load (4 bytes of a table of a few dozen entries: an L1/L2 hit) is in flight together with the
// two dependent loads of the step before it; on the host it is harmless.
struct MetapathRule {
    TypedGraph g;
    const int32_t *node_type;
    const int64_t *start;
    const int32_t *walker_path, *pattern, *path_off;
    int32_t n_paths;
    int32_t *lengths;  // [n_walkers] or null: positions that hold a node
    struct State {
        int64_t cur;
        PathCursor pc;
        int32_t t_next, n_held;
    };
    COGDL_WALK_FN int64_t begin(State &st, int64_t w, int &err) const {
        const int64_t first = start[w];
        st.pc = metapath_begin(g, node_type, first, walker_path[w], pattern, path_off, n_paths, err);
        st.n_held = 1;
        st.cur = -1;
        st.t_next = 0;
        if (err == 0) {
            st.cur = first;
            st.t_next = metapath_next_type(st.pc);  // the type wanted at position 1
        }
        return first;
    }
    COGDL_WALK_FN int64_t advance(State &st, uint64_t seed, int64_t w, int64_t i, int &err) const {
        if (err == 0 && st.cur >= 0) {
            const int32_t t = st.t_next;
            st.t_next = metapath_next_type(st.pc);
            st.cur = step_metapath(g, t, seed, w, i, st.cur, err);
            st.n_held += st.cur >= 0 ? 1 : 0;
        } else {
            st.cur = -1;
        }
        return st.cur;
    }
    COGDL_WALK_FN void finish(const State &st, int64_t w) const {
        if (lengths) lengths[w] = st.n_held;
    }
};

enum : int { kArgsOk = 0, kArgsInvalid = 1, kArgsRange = 2 };

// The argument check of the walk entry points of both libraries (each maps the result to its own status codes; the typed
// graph passes seg / indices_t as indptr / indices).  Where the libraries differ:
//   * length > 2^31 - 1 (the step index is one 32-bit word of the Philox counter) is kArgsRange: libcogdl_hip answers
//     ERANGE, libcogdl_host answers EINVAL, as it always has;
//   * max_walkers: libcogdl_hip bounds n_walkers (ERANGE above (2^31 - 1) * 64, the bound the first walk kernel shipped
//     with; its grid of n_walkers / 256 workgroups would fit gridDim.x for more); libcogdl_host has no such bound and
//     passes INT64_MAX.
inline int walk_args_status(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                            const int64_t *start, int64_t n_walkers, int64_t length, const int64_t *walks, const int *flags,
                            int64_t max_walkers) {
    if (num_nodes < 0 || num_edges < 0 || n_walkers < 0 || length < 1 || !flags) return kArgsInvalid;
    if (n_walkers > 0 && (!indptr || !start || !walks)) return kArgsInvalid;
    if (num_edges > 0 && !indices) return kArgsInvalid;
    if (length > 0x7fffffff || n_walkers > max_walkers) return kArgsRange;
    return kArgsOk;
}

}  // namespace cogdl_walk
