// host_hin2vec.cpp -- the host twin of the pair builder of csrc/hin2vec.hip: live-slot counts and offsets, then HIN2Vec's
// training rows (positives and type-constrained negatives).  Staging, liveness, keys and draws are hin2vec_law.h's, the same
// the kernels follow, so for equal inputs and seed every output element and the flags word are the GPU's.  OpenMP over the
// walks; the result does not depend on the number of threads.  No HIP.  (The score has no host twin: hin2vec_law.h.)
#include <cstdint>
#include <vector>

#include "../../include/cogdl_host.h"
#include "hin2vec_law.h"

namespace hv = cogdl_hin2vec;

namespace {

struct Staged {
    std::vector<int32_t> id, type;
};

int stage_walk(const int64_t *row, int64_t L, const int32_t *node_type, int64_t N, Staged &st) {
    int err = 0;
    st.id.resize((size_t)L);
    st.type.resize((size_t)L);
    for (int64_t p = 0; p < L; ++p) hv::stage(row[p], p + 1 < L ? row[p + 1] : -1, node_type, N, st.id[p], st.type[p], err);
    return err;
}

int status_of(int rc) { return rc == 0 ? COGDL_HOST_OK : (rc == 1 ? COGDL_HOST_EINVAL : COGDL_HOST_ERANGE); }

}  // namespace

extern "C" int cogdl_host_hin_pairs_count(const int64_t *walks, int64_t W, int64_t L, int hop, const int32_t *node_type,
                                          int64_t N, int64_t *offsets, int64_t *scratch, int *flags) {
    (void)scratch;
    const int rc = hv::pairs_status(W, L, hop, 0, N);
    if (rc != 0) return status_of(rc);
    if (!flags || !offsets) return COGDL_HOST_EINVAL;
    *flags = 0;
    if (W > 0 && (!walks || (N > 0 && !node_type))) return COGDL_HOST_EINVAL;
    int err = 0;
#pragma omp parallel reduction(| : err)
    {
        Staged st;
#pragma omp for schedule(static)
        for (int64_t w = 0; w < W; ++w) {
            err |= stage_walk(walks + w * L, L, node_type, N, st);
            const int32_t *ids = st.id.data();
            int64_t live = 0;
            for (int64_t i = 0; i < L - hop; ++i)
                for (int j = 1; j <= hop; ++j) live += hv::slot_live([ids](int64_t p) { return ids[p]; }, i, j, hop) ? 1 : 0;
            offsets[w] = live;
        }
    }
    int64_t run = 0;
    for (int64_t w = 0; w < W; ++w) {
        const int64_t c = offsets[w];
        offsets[w] = run;
        run += c;
    }
    offsets[W] = run;
    *flags = err;
    return COGDL_HOST_OK;
}

extern "C" int cogdl_host_hin_pairs_emit(const int64_t *walks, int64_t W, int64_t L, int hop, int64_t negative,
                                         const int32_t *node_type, const int32_t *type_ptr, const int32_t *type_nodes,
                                         const int32_t *rank, int64_t N, uint64_t seed, const int64_t *offsets, int64_t total,
                                         int64_t *x, int64_t *y, int64_t *key, int64_t *label, int *flags) {
    const int rc = hv::pairs_status(W, L, hop, negative, N);
    if (rc != 0) return status_of(rc);
    if (total < 0 || !flags) return COGDL_HOST_EINVAL;
    if (W == 0 || total == 0) return COGDL_HOST_OK;
    if (!walks || !node_type || !offsets || !x || !y || !key || !label) return COGDL_HOST_EINVAL;
    if (negative > 0 && (!type_ptr || !type_nodes || !rank)) return COGDL_HOST_EINVAL;
    const hv::TypeTables tb = {type_ptr, type_nodes, rank, N};
    const int64_t per = negative + 1;
    int err = 0;
#pragma omp parallel reduction(| : err)
    {
        Staged st;
#pragma omp for schedule(static)
        for (int64_t w = 0; w < W; ++w) {
            (void)stage_walk(walks + w * L, L, node_type, N, st);  // (the count call raised these)
            const int32_t *ids = st.id.data(), *types = st.type.data();
            int64_t slot = offsets[w];
            for (int64_t i = 0; i < L - hop; ++i) {
                for (int j = 1; j <= hop; ++j) {
                    if (!hv::slot_live([ids](int64_t p) { return ids[p]; }, i, j, hop)) continue;
                    if (slot >= 0 && slot < total) {
                        const int32_t xs = ids[i], ys = ids[i + j];
                        const int64_t k = hv::slot_key([types](int64_t p) { return types[p]; }, i, j), at = slot * per;
                        x[at] = xs, y[at] = ys, key[at] = k, label[at] = 1;
                        const uint64_t s = hv::slot_number(w, i, j, L, hop);
                        for (int64_t n = 0; n < negative; ++n) {
                            int64_t nx, ny;
                            hv::negative_row(tb, seed, s, n, xs, ys, types[i], types[i + j], nx, ny, err);
                            x[at + 1 + n] = nx, y[at + 1 + n] = ny, key[at + 1 + n] = k, label[at + 1 + n] = 0;
                        }
                    }
                    ++slot;
                }
            }
        }
    }
    *flags |= err;
    return COGDL_HOST_OK;
}
