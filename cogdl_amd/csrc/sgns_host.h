// sgns_host.h -- what the host twins of the embedding trainers (host_sgns.cpp, host_pvdbow.cpp, host_line.cpp) share: the
// dot product and the target step of sgns_law.h as sgns_step.h runs them on a wave, the trace of applied targets, and the
// loop that runs rows / documents / samples on one thread or under OpenMP.  No HIP.
#pragma once
#include <omp.h>

#include <cstdint>

#include "sgns_law.h"

namespace cogdl_sgns {

// the dot product in the law's order: lane sums over d % 64, then the butterfly's lower half
inline float dot(const float *a, const float *b, int D, int B) {
    float p[kLanes];
    const int m = D < kLanes ? D : kLanes;
    for (int l = 0; l < m; ++l) p[l] = 0.0f + a[l] * b[l];
    for (int l = m; l < B; ++l) p[l] = 0.0f;
    for (int d = kLanes; d < D; ++d) p[d & (kLanes - 1)] = p[d & (kLanes - 1)] + a[d] * b[d];
    for (int s = B >> 1; s > 0; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
    return p[0];
}

// One target: f = dot(x, y); where Rule applies, acc += g * y (the old row), then y += g * x.  x, y and acc are three
// different rows.  -> whether the target was applied.
template <class Rule>
inline bool apply_target(const float *__restrict__ x, float *__restrict__ y, float *__restrict__ acc, int D, int B, float label, float lr,
                         const float *exp_table) {
    const float f = dot(x, y, D, B);
    if (!Rule::applies(f)) return false;
    const float g = Rule::gradient(f, label, lr, exp_table);
    for (int d = 0; d < D; ++d) {
        acc[d] = acc[d] + g * y[d];
        y[d] = y[d] + g * x[d];
    }
    return true;
}

// the applied targets of a serial run, one record of doubles each; n counts the records that did not fit as well
struct Trace {
    double *rec;
    int64_t cap, n;
    template <class... Field>
    void add(Field... fields) {
        if (!rec) return;  // (not asked for: the throughput mode, which must not write here)
        if (n < cap) {
            double *r = rec + n * (int64_t)sizeof...(Field);
            ((*r++ = (double)fields), ...);
        }
        ++n;
    }
};

// body(i, scratch) for i in [0, n).  workers == 1: in order on the calling thread, no parallel region.  Otherwise under
// OpenMP, schedule(dynamic, grain), on `workers` threads (0: OpenMP's default); every thread has a scratch of its own.
template <class MakeScratch, class Body>
inline void parallel_for(int workers, int64_t n, int grain, MakeScratch make_scratch, Body body) {
    if (workers == 1) {
        auto scratch = make_scratch();
        for (int64_t i = 0; i < n; ++i) body(i, scratch);
        return;
    }
#pragma omp parallel num_threads(workers > 0 ? workers : omp_get_max_threads())
    {
        auto scratch = make_scratch();
#pragma omp for schedule(dynamic, grain)
        for (int64_t i = 0; i < n; ++i) body(i, scratch);
    }
}

}  // namespace cogdl_sgns
