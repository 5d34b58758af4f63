// multiplex_law.h -- the law of the fused multiplex attention embedding (GATNE's model step), read by multiplex.hip.  Plain C++:
// no HIP runtime.  The library is built with -ffp-contract=off: a product and the sum it goes into are two roundings everywhere
// below.  tanhf and expf are the device library's; there is no host twin (two libms do not agree bit for bit).
//
// Forward, for sample b with x = inputs[b], t = types[b]; every sum starts from +0 and adds one term at a time:
//   c[i, u]   = SUM_s type_emb[neigh[x, i, s], i, u]                ascending s
//   h[i, a]   = tanhf(SUM_u c[i, u] * att_w1[t, u, a])              ascending u
//   e[i]      = float(SUM_a double(h[i, a]) * double(att_w2[t, a])) ascending a, in float64 (the products are exact there),
//               rounded once: the softmax turns an absolute error of e into a relative error of att, and |e| may be large
//   mx        = e[0], then fmaxf(mx, e[i]) for i = 1 .. T-1
//   z         = SUM_i expf(e[i] - mx)                               ascending i
//   att[i]    = expf(e[i] - mx) / z
//   m[u]      = SUM_i att[i] * c[i, u]                              ascending i
//   y[d]      = node_emb[x, d] + (SUM_u m[u] * trans_w[t, u, d])    ascending u
//   nrm       = sqrtf(butterfly(p)), p[l] = SUM y[d]^2 over d = l, l + 64, l + 128, .. ascending (64 slots, see below)
//   out[b, d] = y[d] / fmaxf(nrm, kEps)
// The butterfly is p[l] = p[l] + p[l ^ off] for off = 32, 16, 8, 4, 2, 1, all l at once.
//
// Backward, per sample, g the gradient that arrives for out[b]:
//   dot       = butterfly(q), q[l] = SUM g[d] * out[b, d] over d = l, l + 64, ..
//   g_y[d]    = (g[d] - out[b, d] * dot) / nrm      where nrm >= kEps  (a NaN nrm takes this line)
//             = g[d] / kEps                         where nrm <  kEps  (torch's clamp_min passes nothing to the norm there)
//   g_m[u]    = butterfly(r), r[l] = SUM g_y[d] * trans_w[t, u, d] over d = l, l + 64, ..
//   g_att[i]  = SUM_u g_m[u] * c[i, u]                              ascending u
//   ds        = SUM_i att[i] * g_att[i]                             ascending i
//   g_e[i]    = att[i] * (g_att[i] - ds)
//   g_pre[i, a] = (g_e[i] * att_w2[t, a]) * (1 - h[i, a] * h[i, a])
//   g_c[i, u] = att[i] * g_m[u], then + g_pre[i, a] * att_w1[t, u, a] for ascending a
//
// Gradient sums.  A list is summed sequentially from +0 inside chunks of kChunk = 128 entries; the chunk partials are then added
// to +0 in ascending chunk order.  An empty list gives +0, and every element of every gradient is written.
//   grad trans_w[t, u, d]  the samples b with types[b] == t, ascending b:        term m[b, u] * g_y[b, d]
//   grad att_w1[t, u, a]   the same list; per b the T terms c[b, i, u] * g_pre[b, i, a] in ascending i (chunks count samples)
//   grad att_w2[t, a]      the same list; per b the T terms g_e[b, i] * h[b, i, a] in ascending i
//   grad node_emb[n, d]    the samples b with inputs[b] == n, ascending b:       term g_y[b, d]
//   grad type_emb[n, i, u] the slots (b, s) with neigh[inputs[b], i, s] == n, ascending b S + s:   term g_c[b, i, u]
// The lists come from one inverted index (operators/kgscore.py: inverted_index) over the keys
//   n T + i  for slot (b, i, s) at position (b T + i) S + s   |   N T + inputs[b] at B T S + b   |   N T + N + types[b] at B T S + B + b
// so that ascending position inside a list is the order stated above.
//
// Ids.  A sample whose input, type or any of its T S neighbours is out of range gets out = NaN and nrm = -1 (norms are never
// negative); the per-sample backward writes zeros for it and the caller keys it into no list.  Malformed lists give wrong
// numbers, never an access outside the operands: every position is range-checked.
// Nothing depends on the launch geometry: a sample is one wave, a chunk of a gradient element's list is one thread.
#pragma once
#include <stdint.h>

namespace cogdl_multiplex {

constexpr int kSlots = 64;
constexpr int64_t kChunk = 128;  // list entries summed sequentially before a partial is closed (chunks may run side by side)
constexpr float kEps = 1e-12f;   // torch.nn.functional.normalize's eps
// what one wave holds: c and h in LDS, y in 16 registers per lane, the softmax on T lanes, m on U lanes
constexpr int64_t kMaxT = 16, kMaxS = 64, kMaxU = 64, kMaxA = 64, kMaxD = 1024;

// 0 ok, 1 invalid, 2 beyond the limits above or int32 indexing of the lists
inline int sizes_status(int64_t B, int64_t N, int64_t T, int64_t S, int64_t U, int64_t A, int64_t D) {
    if (B < 0 || N < 0 || T < 1 || S < 1 || U < 1 || A < 1 || D < 1) return 1;
    if (T > kMaxT || S > kMaxS || U > kMaxU || A > kMaxA || D > kMaxD) return 2;
    const int64_t lim = 0x7fffffff;
    if (B >= lim || N >= lim) return 2;
    if (B * T * S + 2 * B >= lim || N * T + N + T >= lim) return 2;
    return 0;
}

}  // namespace cogdl_multiplex
