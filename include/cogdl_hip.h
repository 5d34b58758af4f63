/*
 * cogdl_hip.h -- C ABI of libcogdl_hip.so: the MI355X (gfx950) sparse message-passing
 * backend that sits underneath CogDL's `cogdl.operators` API.
 *
 * Every entry point replaces one function of the reference's per-op pybind11/CUDA
 * extensions (cited as file:line under /root/reference/).  The reference binds those with
 * torch::Tensor arguments; this ABI is torch-free: raw device pointers, sizes, a dtype
 * enum and the hipStream_t (as void*) to launch on.  Ownership: all buffers are
 * caller-allocated and borrowed for the duration of the enqueued work; nothing is
 * allocated, freed or synchronised inside (so calls are hipGraph-capturable), except the
 * *_workspace_bytes queries which are pure host functions.
 *
 * Error convention: 0 = COGDL_HIP_OK, otherwise a COGDL_HIP_E* code (the reference
 * assert()s / exit()s instead: operators/spmm/computeUtil.h:13-27).  cogdl_hip_strerror
 * maps a code to text.  Launch errors are reported from hipGetLastError() right after the
 * launch; asynchronous faults surface at the caller's next synchronisation as usual.
 *
 * Conventions: CSR index arrays are int32 (what the callers pass: rowptr.int(),
 * colind.int(), cogdl/utils/spmm_utils.py:106); all row*width offset arithmetic inside
 * the kernels is 64-bit.  Dense matrices are row-major contiguous.
 */
#ifndef COGDL_HIP_H
#define COGDL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COGDL_HIP_ABI_VERSION 9

/* Exported with default visibility (the library is built -fvisibility=hidden). */
#if defined(COGDL_HIP_BUILD)
#define COGDL_API __attribute__((visibility("default")))
#else
#define COGDL_API
#endif

enum cogdl_hip_status {
    COGDL_HIP_OK = 0,
    COGDL_HIP_EINVAL = 1,      /* bad argument (null pointer, negative size, ...) */
    COGDL_HIP_EDTYPE = 2,      /* unsupported dtype for this entry point */
    COGDL_HIP_EALIGN = 3,      /* pointer not aligned to the element size */
    COGDL_HIP_ELAUNCH = 4,     /* hipLaunchKernel / runtime error (see cogdl_hip_last_hip_error) */
    COGDL_HIP_EWORKSPACE = 5,  /* workspace too small */
    COGDL_HIP_ERANGE = 6,      /* size exceeds what int32 CSR indices can address */
    COGDL_HIP_EUNSUPPORTED = 7 /* valid call, but a shape this entry point declines (see its comment): the caller
                                * is expected to take its documented alternative -- never returned for a bad call */
};

enum cogdl_hip_dtype {
    COGDL_HIP_F32 = 0,
    COGDL_HIP_F16 = 1,
    COGDL_HIP_BF16 = 2
};

COGDL_API int cogdl_hip_abi_version(void);
COGDL_API const char *cogdl_hip_strerror(int status);
/* hipError_t of the most recent COGDL_HIP_ELAUNCH on this thread (0 if none). */
COGDL_API int cogdl_hip_last_hip_error(void);
/* Run-time tuning knobs for experiments and tests (defaults are the measured optima; the negative results behind the
 * retired keys are tabled in DESIGN.md section 8):
 *    0  XCD stripe of the row-block -> workgroup map (0 = hardware round-robin, default 32)
 *    1  long-row threshold override (0 = automatic)          2  1 = natural row -> lane-group assignment inside a workgroup
 *    3  cap on the number of long-row workgroups (1024)      4  cap on the fused-GAT vector width (0 = widest)
 *    5  fused-GAT forward kernel (0 = automatic, 1 = edge-wise online softmax, 2 = chunk-wise softmax where it applies,
 *       3 = plan kernels without the per-chunk scalars through LDS: attn_col / stats gathered per edge as before)
 *    6  csr_spmm / mhspmm vector width cap (negative: force; -99: power-of-two lane groups only; any value but 0 also keeps the
 *       16-bit plan kernels at 8-byte lanes)
 *    7  edge_softmax lanes (bit 0: 4-byte lanes in the row kernels, bit 1: in the hub-row path, bit 2: row kernels only)
 *    8  polls before the flat edge_softmax kernel's cross-tile wait recomputes the row statistics (0 = 4096; < 0: at once)
 *    9  flat edge_softmax experiments (bit 0: no cross-tile exchange -- WRONG results; bit 2: half-size 16-bit tiles; bit 3: no
 *       kept exp values; bit 4: one 16-bit element per LDS access; bit 6: full-size tiles for under-filled launches; bit 7:
 *       phase stamps, tools/es_phase_probe.py; bit 8: round 5's two-kernel forward, measured slower)
 *   10  csr2csc (0 = by size: one single-workgroup launch up to 16 k slots, the radix sort above; 2 = the radix sort at
 *       every size; 3 = with packed intermediate records at every size)
 *   11  sampler relabelling (1 = the sort-based form)       13  timing: 1 = row blocks exit, 2 = long-row workgroups exit (WRONG results)
 *   15  64-bit CSR: edges per row segment (0 = 2^29)       18  csr_spmm sweep: cap on the rows of one round (0 = the device's)
 *   12, 14, 16  retired in round 6 (wave-scope split of medium rows, row tiles, per-workgroup row queue: all measured <= +-5 %). */
COGDL_API int cogdl_hip_set_tuning(int key, int value);
/* Measurement hook (bench.py `roofline.measured_read_GBs`, SURVEY.md section 8d: the box's own roof beside the spec
 * peak): one read-only pass over `bytes` of device memory in 16-byte vectors; sink: COGDL_HIP_PROBE_BLOCKS * 16 bytes. */
#define COGDL_HIP_PROBE_BLOCKS 4096
COGDL_API int cogdl_hip_probe_read_stream(const void *p, size_t bytes, void *sink, void *stream);
/* ... and one 16-byte-vector copy of `bytes` from src to dst (`roofline.measured_copy_GBs` counts read + written bytes). */
COGDL_API int cogdl_hip_probe_copy_stream(const void *src, void *dst, size_t bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * csr_spmm:  out[i,:] = sum_{e in row i, CSR order} val[e] * x[colind[e],:]
 * Replaces spmm.csr_spmm (operators/spmm/spmm.cpp:22-45 -> spmm_cuda, spmm_kernel.cu:534-594)
 * and, with val == NULL, spmm.csr_spmm_no_edge_value (spmm.cpp:47-65, spmm_kernel.cu:155-190).
 * CPU twin / oracle: csr_spmm_cpu (operators/spmm/spmm_cpu.cpp:6-58).
 * f32: each output element is accumulated sequentially in CSR edge order with a separate
 * fp32 multiply and add -- bit-identical to the reference CPU path as CogDL builds it.
 * f16/bf16: val has the dtype of x; products and sums are fp32, rounded once on store.
 * Weighted 16-bit sums are fp32 fused multiply-adds at vector widths of at least 2 and a rounded multiply followed by a
 * rounded add at width 1 (odd k, or x / out not 4-byte aligned): results can therefore differ in the last place with the
 * parity of k and with pointer alignment.  Unweighted 16-bit rows of at most cogdl_hip_exact_row_edges(nnz) edges equal the
 * fp32 result (the reference loop on the 16-bit inputs) rounded once, whatever the width or alignment.
 * x: [n_src, k], out: [m, k]; rowptr: [m+1]; colind/val: [nnz], nnz == rowptr[m].
 * workspace (optional, device, 256-B aligned, >= cogdl_hip_csr_spmm_workspace_bytes(nnz, k, dtype)):
 * enables the chunk-parallel treatment of rows longer than cogdl_hip_long_row_threshold(nnz)
 * edges (power-law graphs); such rows are summed as fixed-order partial sums (deterministic,
 * re-associated).  With workspace == NULL every row is summed strictly sequentially.
 * The same convention holds for every row-wise operator below: `workspace` is optional scratch
 * for the long-row path (csrc/rowreduce.h), sized by the operator's *_workspace_bytes query
 * (pure host functions; they assume 16-byte aligned operands, as every allocator provides).
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_csr_spmm_workspace_bytes(int64_t nnz, int64_t k, int dtype);
COGDL_API int cogdl_hip_long_row_threshold(int64_t nnz);
/* Rows of at most this many edges are ALWAYS reduced sequentially in CSR order (fp32: bit-identical to the reference's
 * csr_spmm_cpu loop, spmm_cpu.cpp:24-35): cogdl_hip_long_row_threshold(nnz).  Longer rows are cut into contiguous pieces
 * whose partial sums are merged in order by whole workgroups: deterministic, re-associated at the piece borders only
 * (<= 1e-6 relative). */
COGDL_API int cogdl_hip_exact_row_edges(int64_t nnz);
COGDL_API int cogdl_hip_csr_spmm(const int32_t *rowptr, const int32_t *colind, const void *val,
                       const void *x, void *out, int64_t m, int64_t k, int64_t nnz, int dtype,
                       void *workspace, size_t workspace_bytes, void *stream);

/* out += A x: same kernels, the per-element accumulator starts from the existing out[i,:] (then the
 * row's edges are added in CSR order).  Used by the vertex-sharded SpMM, where the remote-column
 * block is applied after the local-column block (no reference counterpart). */
COGDL_API int cogdl_hip_csr_spmm_acc(const int32_t *rowptr, const int32_t *colind, const void *val,
                           const void *x, void *out, int64_t m, int64_t k, int64_t nnz, int dtype,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Tuning hook (benchmarks only): force a kernel variant for csr_spmm; <0 = automatic. */
COGDL_API int cogdl_hip_csr_spmm_variant(const int32_t *rowptr, const int32_t *colind, const void *val,
                               const void *x, void *out, int64_t m, int64_t k, int64_t nnz, int dtype,
                               int variant, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * XCD-partitioned columns (ABI v8; no reference counterpart -- the reference's GE-SpMM kernels have no notion of the chip's
 * eight private L2s).  For gathered tables that fit the eight 4 MiB L2s of the MI355X together but not one of them
 * (BASELINE configs[2]: 233 k rows of 128-256 bytes, rows of hundreds of edges) a PLAN gives every column an owner XCD
 * (hash of its id), cuts every long row into the sub-rows of its edges by owner and lays these virtual rows out so that a
 * workgroup on XCD x only gathers columns XCD x owns.  The plan is built once per structure by the caller
 * (cogdl_amd/xcdplan.py); this struct is its device view, all arrays int32 device memory:
 *   vrowptr [n_slots + 1]  edge offsets of the virtual rows ("slots") in the plan's edge order
 *   vcol    [nnz]          column ids in that order
 *   vdesc   [n_slots][2]   {row, record}: row < 0 = padding slot; record < 0 = the row's only part (finished by the main
 *                          kernel), otherwise the index of this part's state record
 *   eid     [nnz]          what a per-edge operand is indexed by for the edge at a plan position (the CSR position of
 *                          the edge; for a CSC view: the caller's own edge id) -- NULL if the operator has none
 *   mrow [n_multi], mptr [n_multi + 1]   rows with several parts and their records [mptr[i], mptr[i+1]) in merge order
 *   big  [n_big]           the indices i (into mrow) of ALL rows with more than 32 parts: merged by a whole workgroup each
 * n_slots is a multiple of 512 (units of 64 slots, round-robin over the 8 XCDs).  Results are deterministic; a row cut into
 * parts is re-associated (fp32 <= 1e-6 relative) -- which is why csr_spmm takes this path only when asked to. */
typedef struct cogdl_hip_vrows {
    const int32_t *vrowptr, *vcol, *vdesc, *eid, *mrow, *mptr, *big;
    int64_t n_slots, n_multi, n_parts, n_big, nnz;
} cogdl_hip_vrows;
/* out = A x (acc != 0: out += A x) over a plan; val in PLAN order (val_plan[j] = val[eid[j]]) or NULL.
 * workspace >= cogdl_hip_csr_spmm_xcd_workspace_bytes(n_parts, k, dtype). */
COGDL_API size_t cogdl_hip_csr_spmm_xcd_workspace_bytes(int64_t n_parts, int64_t k, int dtype);
COGDL_API int cogdl_hip_csr_spmm_xcd(const cogdl_hip_vrows *plan, const void *val_plan, const void *x, void *out,
                                     int64_t m, int64_t k, int dtype, int acc, void *workspace, size_t workspace_bytes,
                                     void *stream);

/* ---------------------------------------------------------------------------------------
 * Sweep layout (added within ABI v9: new symbols only, nothing existing changes; no reference counterpart): out = A x for a
 * structure whose rows list their columns in ASCENDING order -- the
 * stable transpose that the backward pass of csr_spmm runs over -- with the edges of every group of r consecutive rows merged
 * in ascending column order (stable: equal columns keep their CSR order).  One wave owns a group and keeps its rows' states on chip --
 * registers and LDS -- while it walks the table x top to bottom; with every wave of the chip doing so at about the same pace, the rows an
 * XCD gathers at any moment share a few MB of x (its private L2).  No wave waits for another: the pace only affects speed.
 * Every row still sees its own edges in CSR order, so the result is bit-identical to cogdl_hip_csr_spmm on the same structure.
 *   goff [n_groups + 1]   edge offsets of the groups in layout order, n_groups = ceil(m / r)
 *   src  [nnz]            per edge: column (low 24 bits; x: [n_src, k] with n_src <= 2^23, else COGDL_HIP_EUNSUPPORTED) |
 *                         row - g * r (high 8 bits)
 *   w    [nnz]            fp32 edge weights in layout order, or NULL (unweighted)
 * r <= cogdl_hip_csr_spmm_sweep_group_rows().  Only f32 with k = 128 (512-byte rows); other shapes: COGDL_HIP_EUNSUPPORTED.
 * cogdl_hip_csr_spmm_sweep_round_rows(k, dtype): how many rows the waves resident on the current device hold at once for this
 * width (0: a width the kernel declines); more rows are walked as further groups by the same waves -- correct, less local.
 * Tuning key 18 caps the rows of one round (tests). */
COGDL_API int cogdl_hip_csr_spmm_sweep_group_rows(void);
COGDL_API int64_t cogdl_hip_csr_spmm_sweep_round_rows(int64_t k, int dtype);
COGDL_API int cogdl_hip_csr_spmm_sweep(const int32_t *goff, const int32_t *src, const void *w, const void *x, void *out,
                                       int64_t m, int64_t n_src, int64_t n_groups, int r, int64_t k, int64_t nnz, int dtype,
                                       void *stream);

/* ---------------------------------------------------------------------------------------
 * Guarded launches (added within ABI v9: new symbols only).  The sweep needs no sorted rows, only an order inside each group
 * that keeps every row's own edge order -- so the FORWARD pass may walk a layout of A itself (cogdl_amd/sweepplan.py:
 * build_forward), cached for a structure seen earlier.  Whether the call at hand passes that structure is decided ON THE DEVICE:
 * `parts` are the COGDL_HIP_FINGERPRINT_PARTS partials that cogdl_hip_csr_fingerprint_dev has written to device memory on the
 * same stream (16-byte aligned), `expect` the cached structure's hash.  Every wave sums the partials and compares; with
 * run_if_equal = 1 the launch does its work on a match and nothing otherwise, with run_if_equal = 0 the other way round.  A
 * launch that stands down writes nothing -- not `out`, not the workspace.  Enqueue the sweep guarded 1 and the ordinary launch
 * guarded 0 with the same `out`: exactly one of them computes it, with the bits of cogdl_hip_csr_spmm either way.
 * Both take f32 with k = 128 only (COGDL_HIP_EUNSUPPORTED otherwise); the other arguments are those of cogdl_hip_csr_spmm_sweep /
 * cogdl_hip_csr_spmm. */
COGDL_API int cogdl_hip_csr_spmm_sweep_guarded(const int32_t *goff, const int32_t *src, const void *w, const void *x, void *out,
                                               int64_t m, int64_t n_src, int64_t n_groups, int r, int64_t k, int64_t nnz,
                                               int dtype, const uint64_t *parts, uint64_t expect, int run_if_equal, void *stream);
COGDL_API int cogdl_hip_csr_spmm_guarded(const int32_t *rowptr, const int32_t *colind, const void *val, const void *x,
                                         void *out, int64_t m, int64_t k, int64_t nnz, int dtype, const uint64_t *parts,
                                         uint64_t expect, int run_if_equal, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sweep over groups of ANY rows (added within ABI v9: new symbols only): the two sweep entries above with a row map.
 *   rows [n_map]          n_map = n_groups * r: the output row of local row l of group g at g * r + l; a negative entry is a
 *                         pad slot that is never written.  Every row of out must be named exactly once (a row with no edge is
 *                         stored as zeros by the group that names it); n_groups is the caller's, with n_groups * r >= m.
 * The high 8 bits of a src word are the local row l.  The map is read only where a group's rows are stored, never per edge.
 * Its length is checked here (COGDL_HIP_EINVAL); that every entry is < m is the layout builder's duty
 * (cogdl_amd/sweepplan.py checks it before anything is enqueued).  Bit-identical to cogdl_hip_csr_spmm as above. */
COGDL_API int cogdl_hip_csr_spmm_sweep_rows(const int32_t *goff, const int32_t *src, const void *w, const void *x, void *out,
                                            int64_t m, int64_t n_src, int64_t n_groups, int r, int64_t k, int64_t nnz, int dtype,
                                            const int32_t *rows, int64_t n_map, void *stream);
COGDL_API int cogdl_hip_csr_spmm_sweep_rows_guarded(const int32_t *goff, const int32_t *src, const void *w, const void *x,
                                                    void *out, int64_t m, int64_t n_src, int64_t n_groups, int r, int64_t k,
                                                    int64_t nnz, int dtype, const int32_t *rows, int64_t n_map,
                                                    const uint64_t *parts, uint64_t expect, int run_if_equal, void *stream);

/* ---------------------------------------------------------------------------------------
 * 64-bit CSR ("big CSR", ABI v7): graphs of 2^31 edges and more -- ogbn-papers100M as CogDL feeds it to GCN
 * (symmetrised + coalesced, cogdl/datasets/ogb.py:50-55: 3.2e9 edges).  The reference cannot represent them: the
 * dispatcher casts row pointers to int32 (utils/spmm_utils.py:106), csr_spmm_cpu walks `int` edge offsets and
 * `int ik = i * k` (operators/spmm/spmm_cpu.cpp:24-33), the CUDA kernels take `int nnz` (spmm_kernel.cu:534-594).
 * Row pointers are int64, column ids stay int32.  The rows are cut into SEGMENTS of about 2^29 edges; each segment is
 * one launch of the 32-bit kernels on a rebased int32 copy of its row pointers (csrc/bigcsr.hip), so results are
 * those of cogdl_hip_csr_spmm row for row (same summation order, same long-row rule with the SEGMENT's edge count).
 *   1. cogdl_hip_csr_segments(rowptr64, m, nnz, 0, &seg, scratch, stream)      -- plan time; SYNCHRONISES `stream`
 *   2. cogdl_hip_csr_rebase_rowptr(rowptr64, &seg, rowptr32, stream)           -- rowptr32: [m + seg.n] int32
 *   3. cogdl_hip_csr_spmm_i64 / cogdl_hip_csr_sddmm_i64 / cogdl_hip_csr2csc_i64 with (rowptr32, &seg)
 * Segment s covers rows [row[s], row[s+1]) = edges [edge[s], edge[s+1]); its rebased row pointers are
 * rowptr32[row[s] + s .. row[s+1] + s] (rows + 1 entries, starting at 0).
 * ------------------------------------------------------------------------------------- */
#define COGDL_HIP_MAX_SEGMENTS 64
#define COGDL_HIP_SEGMENT_MAX_EDGES 0x7ff00000ll /* what one 32-bit launch takes (2^31 - 2^20) */
typedef struct cogdl_hip_segments {
    int32_t n;
    int64_t row[COGDL_HIP_MAX_SEGMENTS + 1];
    int64_t edge[COGDL_HIP_MAX_SEGMENTS + 1];
} cogdl_hip_segments;
/* max_edges: target edges per segment (0 = default: tuning key 15, else 2^29; capped at 2^30).  scratch: device,
 * >= 2 * (COGDL_HIP_MAX_SEGMENTS + 1) * 8 bytes.  rowptr[m] must equal nnz (COGDL_HIP_EINVAL otherwise); a single row
 * of more than COGDL_HIP_SEGMENT_MAX_EDGES edges is COGDL_HIP_ERANGE. */
COGDL_API int cogdl_hip_csr_segments(const int64_t *rowptr, int64_t m, int64_t nnz, int64_t max_edges,
                                     cogdl_hip_segments *out, void *scratch, void *stream);
COGDL_API int cogdl_hip_csr_rebase_rowptr(const int64_t *rowptr, const cogdl_hip_segments *seg, int32_t *rowptr32,
                                          void *stream);
/* csr_spmm over all segments (x: [n_src, k], out: [row[n], k], colind / val: [edge[n]]).  Workspace as cogdl_hip_csr_spmm,
 * sized for the largest segment by the query below; NULL = every row sequential. */
COGDL_API size_t cogdl_hip_csr_spmm_i64_workspace_bytes(const cogdl_hip_segments *seg, int64_t k, int dtype);
COGDL_API int cogdl_hip_csr_spmm_i64(const int32_t *rowptr32, const cogdl_hip_segments *seg, const int32_t *colind,
                                     const void *val, const void *x, void *out, int64_t k, int dtype, void *workspace,
                                     size_t workspace_bytes, void *stream);
/* The same with a plan-time ROW SCHEDULE (round 6; no reference counterpart: spmm_kernel.cu walks rows in id order).
 * row_order: [m] int32, a permutation of 0 .. m-1 (for the segmented form: per segment a permutation of the segment's LOCAL
 * row ids 0 .. rows-1, stored at row_order[row[s] ..]); row block b of the launch walks rows row_order[b * G ..] instead of
 * b * G .. -- e.g. rows by decreasing degree inside windows, so that the lane groups of a wave carry rows of one length.
 * Every row is still reduced by one lane group in CSR order and written to its own place: results are those of the
 * unordered call bit for bit.  NULL = id order.  The entries are not validated (a plan-time artefact of the caller, like
 * colind: an id outside [0, m) reads out of bounds). */
COGDL_API int cogdl_hip_csr_spmm_ordered(const int32_t *rowptr, const int32_t *colind, const void *val, const void *x,
                                         void *out, int64_t m, int64_t k, int64_t nnz, int dtype, int acc /* != 0: out += A x */,
                                         const int32_t *row_order, void *workspace, size_t workspace_bytes, void *stream);
COGDL_API int cogdl_hip_csr_spmm_i64_ordered(const int32_t *rowptr32, const cogdl_hip_segments *seg, const int32_t *colind,
                                             const void *val, const void *x, void *out, int64_t k, int dtype,
                                             const int32_t *row_order, void *workspace, size_t workspace_bytes, void *stream);
/* csr_sddmm over all segments (d1: [row[n], k], d2: [n_src, k], out: [edge[n]] fp32). */
COGDL_API int cogdl_hip_csr_sddmm_i64(const int32_t *rowptr32, const cogdl_hip_segments *seg, const int32_t *colind,
                                      const float *d1, const float *d2, float *out, int64_t k, void *stream);
/* Stable transpose -> colptr [n_cols + 1] int64, rowind [nnz] int32, and either or both of
 *   perm [nnz] int64 (CSR position of CSC entry j; may be NULL: 8 bytes per edge are 26 GB at 3.2e9 edges) and
 *   val_t [nnz] = val[perm] (val_bytes in {2, 4}; val and val_t both NULL or both given),
 * ordered inside a column by ascending CSR position like cogdl_hip_csr2csc.  Every segment is transposed by
 * cogdl_hip_csr2csc (twice: column counts, then entries) and merged. */
COGDL_API size_t cogdl_hip_csr2csc_i64_workspace_bytes(const cogdl_hip_segments *seg, int64_t n_cols);
COGDL_API int cogdl_hip_csr2csc_i64(const int32_t *rowptr32, const cogdl_hip_segments *seg, const int32_t *colind,
                                    int64_t n_cols, int64_t *colptr, int32_t *rowind, int64_t *perm, const void *val,
                                    void *val_t, int val_bytes, void *workspace, size_t workspace_bytes, void *stream);
/* out[i, 0:h] = src[perm[i], 0:h] with 64-bit positions (elem_bytes in {2,4}). */
COGDL_API int cogdl_hip_gather_rows_i64(const int64_t *perm, const void *src, void *out, int64_t n, int64_t h,
                                        int elem_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * csr_spmm with a fused normalisation / bias / activation epilogue (fp32):
 *   out[i,:] = act( dst_scale[i] * sum_e val[e] * (src_scale[colind[e]] * x[colind[e],:]) + bias[:] )
 * i.e. the GPU branch of cogdl.utils.spmm_utils.spmm for a graph that carries its normalisation as out_norm / in_norm
 * vectors (utils/spmm_utils.py:98-109: `x = out_norm * x`, kernel, `x = in_norm * x` -- CSR-only graphs such as sampled
 * blocks after row_norm(), cogdl/data/data.py:240-258) plus the bias / ReLU a layer applies behind it
 * (layers/gcn_layer.py:51-64), in ONE pass: no scaled copy of x, no second and third sweep over the output.
 * src_scale [n_src], dst_scale [m], bias [k] are fp32 device vectors, each may be NULL; act: 0 none, 1 ReLU; val may be
 * NULL (unweighted).  Every product is a separately rounded fp32 multiply in the reference's order: bit-identical to
 * the unfused composition for rows up to the long-row threshold.  Workspace: as cogdl_hip_csr_spmm (same query).
 * Returns COGDL_HIP_EUNSUPPORTED for dtype != COGDL_HIP_F32 (callers compose the unfused operators).
 * ------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_csr_spmm_epilogue(const int32_t *rowptr, const int32_t *colind, const void *val, const void *x,
                                void *out, int64_t m, int64_t k, int64_t nnz, int dtype, const float *src_scale,
                                const float *dst_scale, const float *bias, int act, void *workspace,
                                size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * csr2csc: stable transpose of the CSR structure.
 * Replaces spmm.csr2csc (operators/spmm/spmm.cpp:72-90 -> cusparseCsr2cscEx2 ALG1,
 * spmm_kernel.cu:514-532,596-614) and mhtranspose.csr2csc (mhTranspose.cu:51-111).
 * Outputs colptr [n_cols+1], rowind [nnz] and perm [nnz] (perm[j] = CSR position of CSC
 * entry j; within a column entries keep ascending CSR position, i.e. ascending row).
 * Values are moved with cogdl_hip_gather_rows(perm, val, ...) -- one gather serves both
 * the scalar weights of csr2csc and the [E,H] attention of mhtranspose.
 * workspace: device scratch of at least cogdl_hip_csr2csc_workspace_bytes(...) bytes.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_csr2csc_workspace_bytes(int64_t m, int64_t n_cols, int64_t nnz);
COGDL_API int cogdl_hip_csr2csc(const int32_t *rowptr, const int32_t *colind, int64_t m, int64_t n_cols,
                      int64_t nnz, int32_t *colptr, int32_t *rowind, int32_t *perm,
                      void *workspace, size_t workspace_bytes, void *stream);
/* The same for a fixed-capacity block (cogdl_hip_sample_adj_padded): colind holds `nnz` slots, the first rowptr[m]
 * (read on the device) are edges, the rest is ignored -- colptr[n_cols] = rowptr[m]; rowind / perm hold that many
 * meaningful entries (the tail is unspecified but in range).  Launch shapes depend on the capacity only. */
COGDL_API size_t cogdl_hip_csr2csc_padded_workspace_bytes(int64_t m, int64_t n_cols, int64_t nnz);
COGDL_API int cogdl_hip_csr2csc_padded(const int32_t *rowptr, const int32_t *colind, int64_t m, int64_t n_cols,
                             int64_t nnz, int32_t *colptr, int32_t *rowind, int32_t *perm, void *workspace,
                             size_t workspace_bytes, void *stream);

/* out[i, 0:h] = src[perm[i], 0:h]  (elem_bytes in {2,4}).
 * Replaces mhtranspose.mhtranspose (operators/spmm/mhTranspose.cu:6-49) and the value leg
 * of csr2csc. */
COGDL_API int cogdl_hip_gather_rows(const int32_t *perm, const void *src, void *out, int64_t n, int64_t h,
                          int elem_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * csr_sddmm: out[e] = < d1[row(e),:], d2[colind[e],:] >      (gradient of edge weights)
 * Replaces sddmm.csr_sddmm (operators/spmm/sddmm.cpp:47-70, sddmm_kernel.cu:249-417,451-476).
 * ------------------------------------------------------------------------------------- */
/* Per-edge outputs: hub rows are split over whole workgroups without any scratch. */
COGDL_API int cogdl_hip_csr_sddmm(const int32_t *rowptr, const int32_t *colind, const float *d1,
                        const float *d2, float *out, int64_t m, int64_t k, int64_t nnz, void *stream);

/* ---------------------------------------------------------------------------------------
 * edge_softmax: per (destination row, head) softmax over the row's edges; values [E,H].
 * Replaces edge_softmax.edge_softmax / edge_softmax_backward
 * (operators/edge_softmax/edge_softmax.cc:16-49, edge_softmax.cu:7-60,63-98).
 * Any H >= 1 (the reference's block (32,H) caps H at 32).  values / softmax / grad / out share the element type
 * `dtype` (f32, f16, bf16; fp32 arithmetic, rounded once on store).
 * With a workspace of cogdl_hip_edge_softmax_workspace_bytes(nnz, h) bytes (device, 256-B aligned), H a power of
 * two <= 64 and 16-byte aligned operands the call is ONE streaming pass (every value read from HBM once, written
 * once; rows that cross tile borders are combined inside the launch, csrc/edge_softmax_flat.hip): two launches (a
 * small init kernel + the main kernel), no host synchronisation, hipGraph-capturable.  Other shapes use
 * row-parallel kernels (every dtype since ABI v5: 2-byte values with H not a power of two / H > 64 are read and written
 * natively by the generic row kernel; without a workspace hub rows are reduced sequentially).
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_edge_softmax_workspace_bytes(int64_t nnz, int64_t h);
COGDL_API int cogdl_hip_edge_softmax_fwd(const int32_t *rowptr, const void *values, void *out, int64_t m,
                               int64_t nnz, int64_t h, int dtype, void *workspace, size_t workspace_bytes,
                               void *stream);
COGDL_API int cogdl_hip_edge_softmax_bwd(const int32_t *rowptr, const void *softmax, const void *grad,
                               void *grad_in, int64_t m, int64_t nnz, int64_t h, int dtype, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * mhspmm:  out[v,h,:] = sum_e att[e,h] * feat[colind[e],h,:]     feat [n_src,H,F]
 * Replaces mhspmm.mhspmm (operators/spmm/multiheadSpmm.cpp, multiheadSpmm.cu:6-77).
 * att is always f32; feat/out have `dtype` (f32: sequential fp32 mul+add per element).
 * f16/bf16 feat: fp32 arithmetic, rounded once on store.  Weighted 16-bit sums are fp32 fused multiply-adds at vector widths
 * of at least 2 and multiply-then-add at width 1 (odd F, or feat / out not 4-byte aligned): results can therefore differ in
 * the last place with the parity of F and with pointer alignment.  (Unweighted 16-bit rows up to the exact-row bound equal
 * the fp32 result rounded once: csr_spmm with val == NULL; mhspmm always has weights.)
 * workspace: cogdl_hip_mhspmm_workspace_bytes(nnz, H, F, dtype) (mhsddmm needs none).
 * mhsddmm: out[e,h] = < grad[row(e),h,:], feat[colind[e],h,:] >
 * Replaces mhsddmm.mhsddmm (operators/spmm/multiheadSddmm.cu:6-113).
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_mhspmm_workspace_bytes(int64_t nnz, int64_t h, int64_t f, int dtype);
COGDL_API int cogdl_hip_mhspmm(const int32_t *rowptr, const int32_t *colind, const float *att,
                     const void *feat, void *out, int64_t v, int64_t h, int64_t f, int64_t nnz, int dtype,
                     void *workspace, size_t workspace_bytes, void *stream);
/* mhspmm over a permuted view: the attention row of CSR position e is att[eid[e],:] (eid NULL = identity).  With
 * (rowptr, colind, eid) = (colptr, rowind, perm) of cogdl_hip_csr2csc this is the backward product A^T with the
 * attention left in its forward (CSR) order -- no transposed copy of the [E, H] tensor (the reference permutes it
 * with mhtranspose first, operators/mhspmm.py:57-60). */
COGDL_API int cogdl_hip_mhspmm_eid(const int32_t *rowptr, const int32_t *colind, const float *att, const int32_t *eid,
                         const void *feat, void *out, int64_t v, int64_t h, int64_t f, int64_t nnz, int dtype,
                         void *workspace, size_t workspace_bytes, void *stream);
COGDL_API int cogdl_hip_mhsddmm(const int32_t *rowptr, const int32_t *colind, const float *grad,
                      const float *feat, float *out, int64_t v, int64_t h, int64_t f, int64_t nnz,
                      void *stream);

/* ---------------------------------------------------------------------------------------
 * scatter_max: out[r,c] = max_{e in row r} feat[colind[e],c]; max_id[r,c] = the colind of
 * the FIRST maximum in CSR order (-1 and 0.0 for an empty row).
 * Replaces scatter_max.scatter_max_fp / scatter_max_bp
 * (operators/scatter_max/scatter_max.cc:19-38, scatter_max.cu:5-75) -- without its
 * FLT_MIN initial value, uninitialised argmax and uninitialised gradient buffer.
 * Backward: grad_src[max_id[r,c], c] += grad[r,c]; grad_src [n_src,k] is zeroed inside.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_scatter_max_workspace_bytes(int64_t nnz, int64_t k);
COGDL_API int cogdl_hip_scatter_max_fwd(const int32_t *rowptr, const int32_t *colind, const float *feat,
                              float *out, int32_t *max_id, int64_t m, int64_t k, int64_t nnz,
                              void *workspace, size_t workspace_bytes, void *stream);
COGDL_API int cogdl_hip_scatter_max_bwd(const float *grad, const int32_t *max_id, float *grad_src, int64_t m,
                              int64_t k, int64_t n_src, void *stream);
/* The same backward as a gather over the transposed structure (colptr[n_src+1], rowind[nnz] of cogdl_hip_csr2csc):
 * grad_src[u,c] = sum over the out-edges (u -> v) with max_id[v,c] == u of grad[v,c], in ascending v.  No atomics and no
 * zero-fill: deterministic, and bit-identical to the sequential reference loop for rows up to the long-row threshold.
 * A multi-edge counts once.  workspace: cogdl_hip_scatter_max_bwd_workspace_bytes (optional, hub rows). */
COGDL_API size_t cogdl_hip_scatter_max_bwd_workspace_bytes(int64_t nnz, int64_t k);
COGDL_API int cogdl_hip_scatter_max_bwd_csc(const int32_t *colptr, const int32_t *rowind, const float *grad,
                                  const int32_t *max_id, float *grad_src, int64_t n_src, int64_t k, int64_t nnz,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * gspmm ("source OP edge feature, then aggregate"): the s_{add,sub,mul}_e_{sum,mean} operators and scatter_add of
 * cogdl/operators/ops.py:4-11 (scatter_add), :19-26 (op_src_edge), :28-40 (op_aggr), :43-52 (src_op_e_aggr_coo),
 * :55-103, which the reference composes from torch ops over the COO edge list (an [E, F] message tensor, then
 * scatter_add_).  Over the destination-sorted (CSR) view of the same edges:
 *   out[v,:] = scale_v * sum_{j in row v} weight[id_j] * ( x[colind[j],:] OP efeat[id_j,:] ),  id_j = eid ? eid[j] : j
 *   eid     CSR position -> edge id of efeat/weight (perm of cogdl_hip_coo2csr_index, as int32), NULL = identity;
 *   x       [n_src, k] or NULL (message = the edge feature alone: scatter_add(efeat, dst));
 *   efeat   [E, k], or [E] with efeat_is_scalar != 0 (ops.py:45-46 views a 1-D e_feat as [E, 1]), or NULL (message =
 *           the source row alone);   weight [E] or NULL (ops.py:49-50);   op: COGDL_HIP_GSPMM_*;
 *   mean    != 0: scale_v = 1 / deg(v) (0 for an empty row), else 1.
 * fp32; per output element the edges are added in row order with every step rounded like the torch expression, so
 * rows up to the long-row threshold equal a sequential CPU scatter_add_ bit for bit.  No atomics (deterministic).
 * ------------------------------------------------------------------------------------- */
/* WMUL: (x * weight) * efeat -- the rounding order of autograd's chain for the MUL operator's source gradient (x := the
 * upstream gradient rows over the SOURCE-sorted view of the edges), so that the fused backward equals the torch one bit
 * for bit; needs x and efeat. */
enum { COGDL_HIP_GSPMM_ADD = 0, COGDL_HIP_GSPMM_SUB = 1, COGDL_HIP_GSPMM_MUL = 2, COGDL_HIP_GSPMM_WMUL = 3 };
COGDL_API size_t cogdl_hip_gspmm_workspace_bytes(int64_t nnz, int64_t k);
COGDL_API int cogdl_hip_gspmm(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const float *x,
                    const float *efeat, int efeat_is_scalar, const float *weight, int op, int mean, float *out,
                    int64_t m, int64_t k, int64_t nnz, void *workspace, size_t workspace_bytes, void *stream);

/* gspmm over an XCD-partitioned plan of the destination-sorted view (round 6, ABI v9; cogdl_hip_vrows as built by
 * cogdl_amd/xcdplan.py: build(rowptr, colind_sorted, eid_base = the view's perm, split = cogdl_hip_exact_row_edges(nnz))): the
 * same sums -- rows up to the exact-row bound in the caller's edge order, longer rows in pieces like the ordinary launch's
 * long-row path -- with rows of one length per wave.  rowptr: the view's row pointer (used by `mean`).  The Python front
 * takes it for memoised edge lists of skewed graphs from their second use on (operators/ops.py: EdgePlan.xcd). */
COGDL_API size_t cogdl_hip_gspmm_xcd_workspace_bytes(int64_t n_parts, int64_t k);
COGDL_API int cogdl_hip_gspmm_xcd(const cogdl_hip_vrows *plan, const int32_t *rowptr, const float *x, const float *efeat,
                        int efeat_is_scalar, const float *weight, int op, int mean, float *out, int64_t m, int64_t k,
                        void *workspace, size_t workspace_bytes, void *stream);


/* Per-edge gradients of the family (autograd of src_op_e_aggr_coo, ops.py:43-52) without [E, k] temporaries, over the
 * caller's COO list (row = destination, col = source, int64 as CogDL keeps them), from the upstream gradient grad [m, k]:
 *   g = grad[row[e], :] * scale[row[e]]            (scale [m]: 1 / deg for "mean", NULL for "sum")
 *   grad_weight[e]   = sum_k (x[col[e], k] OP efeat[e, k]) * g[k]                     ([E]; NULL = not wanted)
 *   grad_efeat[e, :] = MUL: (g * weight[e]) * x[col[e], :];  ADD: g * weight[e];  SUB: -(g * weight[e])
 *                      ([E, k], or [E] summed over k when efeat_is_scalar; NULL = not wanted; weight NULL = 1)
 * with autograd's roundings in autograd's order (bit-identical to the torch composition for [E, k] outputs).
 * op: COGDL_HIP_GSPMM_ADD | SUB | MUL.  fp32. */
COGDL_API int cogdl_hip_gspmm_edge_grad(const int64_t *row, const int64_t *col, const float *grad, const float *scale,
                              const float *weight, const float *x, const float *efeat, int efeat_is_scalar, int op,
                              float *grad_efeat, float *grad_weight, int64_t n_edges, int64_t k, void *stream);

/* ---------------------------------------------------------------------------------------
 * Relational gspmm (csrc/relspmm.hip): gspmm on a graph whose edges carry a TYPE, the edge operand being a row of a small
 * relation table looked up through the type -- the message passing of CompGCN (cogdl/models/nn/compgcn.py:124-140: gather
 * x[col], gather rel_embed[edge_type], combine, multiply by the layer weight, scale, scatter_add_) without any [E, k] tensor
 * and without atomics.  Over the destination-sorted (CSR) view of the edges:
 *   out[v,:] = sum_{j in row v} weight[id_j] * ( x[colind[j],:] OP rel[etype[id_j],:] ),   id_j = eid ? eid[j] : j
 *   eid     CSR position -> edge id of etype/weight (perm of cogdl_hip_coo2csr_index, as int32), NULL = identity;
 *   etype   [E] int32 in the caller's edge order, every id in [0, n_rel) (the kernel clamps: a bad id gives a wrong
 *           number, not a read outside rel; the Python front refuses it before the launch);
 *   x       [n_src, k];   rel [n_rel, k] or NULL (message = the source row alone, etype unused);   weight [E] or NULL;
 *   op      COGDL_HIP_GSPMM_ADD | SUB | MUL | WMUL (WMUL: (x * weight) * rel, autograd's rounding order for the source
 *           gradient of MUL: x := the upstream gradient rows over the SOURCE-sorted view; SUB / ADD take rel = NULL there).
 * fp32; per output element the edges are added in row order with every step rounded like the torch expression, so rows
 * of up to cogdl_hip_exact_row_edges(nnz) edges equal a sequential CPU scatter_add_ bit for bit; longer rows are summed
 * in pieces merged in a fixed order.  No atomics (deterministic).  Vector width 4 -> 2 -> 1 by pointer alignment and k.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_rel_gspmm_workspace_bytes(int64_t nnz, int64_t k);
COGDL_API int cogdl_hip_rel_gspmm(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const int32_t *etype,
                        const float *x, const float *rel, const float *weight, int op, float *out, int64_t m, int64_t k,
                        int64_t nnz, int64_t n_rel, void *workspace, size_t workspace_bytes, void *stream);

/* Gradient of the relation table, over the TYPE-sorted view of the same edges (typeptr [n_rel + 1]; stable sort, so the
 * edges of a type keep the caller's order), from the upstream gradient grad [m, k]:
 *   grad_rel[t,:] = sum_{j in row t}  SUB: -(grad[dst_j,:] * weight[id_j])   ADD: grad[dst_j,:] * weight[id_j]
 *                                     MUL: (grad[dst_j,:] * weight[id_j]) * x[src_j,:]
 *   dst_sorted / src_sorted  [E] destination / source of every edge in sorted order (src_sorted and x: MUL only);
 *   eid     sorted position -> edge id of weight, NULL = identity;   op: COGDL_HIP_GSPMM_ADD | SUB | MUL.
 * Same engine, same summation rules; a type without edges gives a zero row.  The rows are long by construction (E / n_rel
 * edges), so the chunk path with its fixed merge order is the usual one: deterministic, re-associated. */
COGDL_API size_t cogdl_hip_rel_gspmm_grad_rel_workspace_bytes(int64_t nnz, int64_t k);
COGDL_API int cogdl_hip_rel_gspmm_grad_rel(const int32_t *typeptr, const int32_t *dst_sorted, const int32_t *src_sorted,
                                 const int32_t *eid, const float *grad, const float *x, const float *weight, int op,
                                 float *grad_rel, int64_t n_rel, int64_t k, int64_t nnz, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * GENConv aggregation (csrc/genaggr.hip): the message passing of DeeperGCN's layer (cogdl/layers/deepergcn_layer.py:67-93:
 * gather x[col], add the encoded edge features, relu + eps, times beta, edge softmax with one channel per column, multiply,
 * scatter_add_) without any [E, k] tensor and without atomics.  Over the destination-sorted (CSR) view of the edges:
 *   msg[j,:]  = relu(x[colind[j],:] + eterm[id_j,:]) + eps,                          id_j = eid ? eid[j] : j
 *   SOFTMAX:    out[v,:] = sum_{j in row v} softmax_{j in row v}(beta * msg[j,:]) * msg[j,:]     (per column)
 *   SUM / MEAN: out[v,:] = sum_{j in row v} w_v * msg[j,:],   w_v = 1 | 1 / deg(v) (0 for an empty row); the product is
 *               rounded before the add, so rows of up to cogdl_hip_exact_row_edges(nnz) edges equal a sequential CPU
 *               scatter_add_ of msg * deg_rev[row] bit for bit.
 *   eterm     [E, k] in the caller's edge order, or NULL;   eid as for cogdl_hip_rel_gspmm;
 *   beta_dev  one float in device memory (read by the kernel: nothing is baked into a captured graph), or NULL: `beta`;
 *   lse       [m, k] or NULL: max + log(denom) of every (row, column), what the backward needs (0 for an empty row);
 *   q         [m, k] or NULL (needs lse): sum_j softmax_j * msg_j^2, from which the caller takes the gradient of beta,
 *             sum(grad * (q - out^2)).  lse and q are SOFTMAX only (COGDL_HIP_EINVAL otherwise).
 * The softmax is an online softmax in CSR edge order (one expf per edge and column); rows longer than the long-row
 * threshold are reduced in pieces whose states merge with the usual rescaling in a fixed order.  A row of one edge returns
 * msg bit for bit, an empty row 0.  fp32, deterministic.  Vector width 4 -> 2 -> 1 by pointer alignment and k.
 * ------------------------------------------------------------------------------------- */
enum { COGDL_HIP_GEN_SOFTMAX = 0, COGDL_HIP_GEN_SUM = 1, COGDL_HIP_GEN_MEAN = 2 };
COGDL_API size_t cogdl_hip_gen_aggr_fwd_workspace_bytes(int64_t nnz, int64_t k);
COGDL_API int cogdl_hip_gen_aggr_fwd(const int32_t *rowptr, const int32_t *colind, const int32_t *eid, const float *x,
                           const float *eterm, int mode, const float *beta_dev, float beta, float eps, float *out,
                           float *lse, float *q, int64_t m, int64_t k, int64_t nnz, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Backward over the SOURCE-sorted view of the same edges (srcptr [n_src + 1]; dst_sorted [E] the destination of every edge
 * in that order; eid sorted position -> edge id of eterm / grad_eterm, NULL = identity):
 *   pre = x[u,:] + eterm[id,:],  msg = relu(pre) + eps,  s = exp(beta * msg - lse[v,:])
 *   SOFTMAX:    d = grad[v,:] * s * (1 + beta * (msg - out[v,:])) * [pre > 0]
 *   SUM / MEAN: d = grad[v,:] * [pre > 0]            (MEAN: the caller passes grad already multiplied by 1 / deg(v))
 *   grad_x[u,:] = sum of d over the out-edges of u in the caller's edge order (pieces in a fixed order for long rows);
 *   grad_eterm[id,:] = d when grad_eterm != NULL ([E, k]: every row is written exactly once).
 * out / lse: the forward's results (SOFTMAX only).  No atomics. */
COGDL_API size_t cogdl_hip_gen_aggr_bwd_workspace_bytes(int64_t nnz, int64_t k);
COGDL_API int cogdl_hip_gen_aggr_bwd(const int32_t *srcptr, const int32_t *dst_sorted, const int32_t *eid, const float *x,
                           const float *eterm, const float *grad, const float *out, const float *lse, int mode,
                           const float *beta_dev, float beta, float eps, float *grad_x, float *grad_eterm, int64_t n_src,
                           int64_t k, int64_t nnz, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Neighbourhood routing (csrc/disen.hip): one step of DisenGCN's routing loop (cogdl/layers/disengcn_layer.py:56-69) without
 * any [E, K d] or [E, K] tensor and without atomics.  c, z, out: [n, n_channels * d], channel k = columns k d .. (k + 1) d - 1.
 * Over the destination-sorted (CSR) view of the edges (rowptr [n + 1], colind [nnz] = the source of every edge):
 *   s[e,k]   = <c[i,k], z[j,k]> / tau                                           (i the row, j = colind[e])
 *   a[i,k]   = z[i,k] + sum_{e in row i} softmax_{e in row i}(s[e,k]) * z[j,k]      (a row without edges: z[i,k])
 *   out[i,k] = a[i,k] / nrm[i,k],   nrm[i,k] = ||a[i,k]||_2                     (no epsilon: a zero a[i,k] gives nan)
 *   nrm, lse [n, n_channels]: the norm, and max + log(denom) of the softmax (0 for a row without edges; lse may be NULL).
 * d in {2, 4, 8, 16, 32, 64} (anything else: COGDL_HIP_EUNSUPPORTED), any n_channels >= 1, tau > 0.  The softmax is an online
 * softmax in CSR edge order (one expf per edge and channel); rows longer than the long-row threshold are reduced in pieces
 * whose states merge with the usual rescaling in a fixed order.  fp32, deterministic.  Vector width 4 -> 2 -> 1 by pointer
 * alignment, row length and d; the workspace covers every width.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_disen_route_fwd_workspace_bytes(int64_t nnz, int64_t n_channels, int64_t d);
COGDL_API int cogdl_hip_disen_route_fwd(const int32_t *rowptr, const int32_t *colind, const float *c, const float *z, float tau,
                              float *out, float *nrm, float *lse, int64_t n, int64_t n_channels, int64_t d, int64_t nnz,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Backward.  The caller supplies ga = d loss / d a = (g - out <out, g>) / nrm  [n, n_channels * d]  and
 * dl[i,k] = <ga[i,k], nrm[i,k] out[i,k] - z[i,k]>  [n, n_channels].  Per edge both passes recompute
 *   p = exp(s - lse[i,k]),  t = <ga[i,k], z[j,k]>,  r = p * (t - dl[i,k]) / tau            (no per-edge scratch)
 * bwd_c, over the destination-sorted view of the forward:  grad_c[i,k] = sum_{e in row i} r * z[j,k];
 * bwd_z, over the SOURCE-sorted view (srcptr [n + 1]; dst_sorted [nnz] the destination of every edge in that order):
 *   grad_z[j,k] = ga[j,k] + sum_{e: source j} (p * ga[i,k] + r * c[i,k]).
 * Sums in the view's edge order (pieces in a fixed order for long rows).  No atomics. */
COGDL_API size_t cogdl_hip_disen_route_bwd_c_workspace_bytes(int64_t nnz, int64_t n_channels, int64_t d);
COGDL_API int cogdl_hip_disen_route_bwd_c(const int32_t *rowptr, const int32_t *colind, const float *c, const float *z,
                                const float *ga, const float *lse, const float *dl, float tau, float *grad_c, int64_t n,
                                int64_t n_channels, int64_t d, int64_t nnz, void *workspace, size_t workspace_bytes,
                                void *stream);
COGDL_API size_t cogdl_hip_disen_route_bwd_z_workspace_bytes(int64_t nnz, int64_t n_channels, int64_t d);
COGDL_API int cogdl_hip_disen_route_bwd_z(const int32_t *srcptr, const int32_t *dst_sorted, const float *c, const float *z,
                                const float *ga, const float *lse, const float *dl, float tau, float *grad_z, int64_t n,
                                int64_t n_channels, int64_t d, int64_t nnz, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused GAT attention + aggregation (no [E,H] tensor is materialised in forward):
 *   s[e,h] = LeakyReLU(attn_row[row(e),h] + attn_col[colind[e],h]);  a = softmax_row(s)
 *   out[v,h,:] = sum_e a[e,h] * feat[colind[e],h,:]
 * Replaces fused_gatconv.gat_forward / gat_backward as bound by
 * operators/fused_gat.py:14-41 (dgNN; source absent from the reference tree -- semantics
 * are those of the unfused path, layers/gat_layer.py:73-77).
 * Forward also emits edge_max/edge_sum [v,H] (row max of s and sum exp(s-max)), which the
 * backward consumes like the reference's ctx.save_for_backward does (fused_gat.py:20).
 * Forward workspace (optional): cogdl_hip_gat_fwd_workspace_bytes -- hub rows are then split over whole
 * workgroups and their (max, sum, acc) states merged like flash-attention blocks.  The launch picks its lane width from the
 * alignment of feat / out (backward: grad_out / grad_feat too), and narrower lanes need larger piece records: the four
 * workspace queries of this operator answer for the least aligned operands an element type allows, so an operand that
 * starts mid-allocation never meets COGDL_HIP_EWORKSPACE with a workspace of the queried size.
 * Backward needs the CSC view (colptr,rowind from cogdl_hip_csr2csc), the forward
 * output and a workspace of cogdl_hip_gat_bwd_workspace_bytes(v, n_src, h, f, nnz, dtype) bytes (D[v,h], the per-tile
 * partials of the tiled shapes, plus the long-row scratch of its two passes; a workspace without the latter disables
 * the long-row path).
 * feat / out / grad_out / grad_feat have element type `dtype` (f32, f16 or bf16: read natively, fp32
 * arithmetic, grad_feat rounded once on store); attention vectors, statistics and their gradients are fp32.
 * Any H and F: rows of up to 64 lanes x one 16-byte vector whose heads are a power-of-two number of lanes take one lane
 * group per row; everything else (8 heads x 64 features, 6 x 12, ...) runs in column tiles with the per-(row, head)
 * scalars finished by a second small kernel (csrc/gat_tiled.hip) -- the reference's backward has no shape limit
 * (operators/fused_gat.py:28-40).
 *
 * Attention dropout (ABI v5).  CogDL's gat model runs with attn_drop = 0.5 by default (models/nn/gat.py:30), which
 * sends GATLayer.forward through leaky_relu(h_l[row] + h_r[col]) -> edge_softmax -> nn.Dropout -> mhspmm
 * (layers/gat_layer.py:72-77).  cogdl_hip_gat_dropout_fwd / _bwd are that composition as ONE forward kernel and two
 * backward passes:  out[v,h,:] = sum_e d[e,h] * a[e,h] * feat[colind[e],h,:],  d[e,h] = keep(e,h) ? scale : 0.
 * The mask is a pure function of (seed, e, h) -- Philox4x32-10, csrc/philox.h: counter (e, 0, h / 8, 0), key = seed, the
 * (h % 8)-th 16-bit piece compared with thresh = round(p * 65536); scale = 65536 / (65536 - thresh) (p = 0.5: 2, as
 * torch) -- with e the edge's position in (rowptr, colind), so nothing of size [E,H] is stored between forward and
 * backward: the backward regenerates it (its column pass reads e from `perm`, the CSC-slot -> CSR-position array of
 * cogdl_hip_csr2csc).  cogdl_hip_edge_dropout_mask writes d[e,h] as a dense [nnz,h] fp32 tensor (tests; callers that
 * want the same mask on the unfused operators).  h <= 64.  p = 0 is the plain operator.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_gat_fwd_workspace_bytes(int64_t nnz, int64_t h, int64_t f, int dtype);
COGDL_API int cogdl_hip_gat_fwd(const int32_t *rowptr, const int32_t *colind, const float *attn_row,
                      const float *attn_col, const void *feat, float negative_slope, void *out,
                      float *edge_max, float *edge_sum, int64_t v, int64_t h, int64_t f, int64_t nnz,
                      int dtype, void *workspace, size_t workspace_bytes, void *stream);
COGDL_API size_t cogdl_hip_gat_bwd_workspace_bytes(int64_t v, int64_t n_src, int64_t h, int64_t f, int64_t nnz,
                      int dtype);
COGDL_API int cogdl_hip_gat_bwd(const int32_t *rowptr, const int32_t *colind, const int32_t *colptr,
                      const int32_t *rowind, const float *attn_row, const float *attn_col,
                      const void *feat, float negative_slope, const float *edge_max,
                      const float *edge_sum, const void *out, const void *grad_out,
                      void *grad_feat, float *grad_attn_row, float *grad_attn_col,
                      void *workspace, size_t workspace_bytes, int64_t v, int64_t n_src, int64_t h,
                      int64_t f, int64_t nnz, int dtype, void *stream);
COGDL_API int cogdl_hip_gat_dropout_fwd(const int32_t *rowptr, const int32_t *colind, const float *attn_row,
                      const float *attn_col, const void *feat, float negative_slope, float p, uint64_t seed,
                      void *out, float *edge_max, float *edge_sum, int64_t v, int64_t h, int64_t f, int64_t nnz,
                      int dtype, void *workspace, size_t workspace_bytes, void *stream);
COGDL_API int cogdl_hip_gat_dropout_bwd(const int32_t *rowptr, const int32_t *colind, const int32_t *colptr,
                      const int32_t *rowind, const int32_t *perm, const float *attn_row, const float *attn_col,
                      const void *feat, float negative_slope, float p, uint64_t seed, const float *edge_max,
                      const float *edge_sum, const void *out, const void *grad_out,
                      void *grad_feat, float *grad_attn_row, float *grad_attn_col,
                      void *workspace, size_t workspace_bytes, int64_t v, int64_t n_src, int64_t h,
                      int64_t f, int64_t nnz, int dtype, void *stream);
/* The fused GAT operator over XCD-partitioned plans (cogdl_hip_vrows above; p == 0: no dropout, p > 0: the mask of
 * cogdl_hip_gat_dropout_fwd -- a function of (seed, CSR position, head), so plan->eid must be the CSR position of every plan
 * position; for the CSC plan of the backward: the CSR position of the transposed entry, i.e. perm composed with the plan).
 * Shapes the ordinary entries run through the chunk-wise forward / the column-tiled backward return COGDL_HIP_EUNSUPPORTED:
 * the caller keeps the ordinary entry for them.  Same results as the ordinary entries up to re-association. */
COGDL_API size_t cogdl_hip_gat_fwd_xcd_workspace_bytes(int64_t n_parts, int64_t h, int64_t f, int dtype);
COGDL_API int cogdl_hip_gat_fwd_xcd(const cogdl_hip_vrows *plan, const float *attn_row, const float *attn_col,
                      const void *feat, float negative_slope, float p, uint64_t seed, void *out, float *edge_max,
                      float *edge_sum, int64_t v, int64_t h, int64_t f, int dtype, void *workspace,
                      size_t workspace_bytes, void *stream);
COGDL_API size_t cogdl_hip_gat_bwd_xcd_workspace_bytes(int64_t v, int64_t h, int64_t f, int64_t n_parts_row,
                      int64_t n_parts_col, int dtype);
COGDL_API int cogdl_hip_gat_bwd_xcd(const cogdl_hip_vrows *plan_csr, const cogdl_hip_vrows *plan_csc,
                      const float *attn_row, const float *attn_col, const void *feat, float negative_slope, float p,
                      uint64_t seed, const float *edge_max, const float *edge_sum, const void *out,
                      const void *grad_out, void *grad_feat, float *grad_attn_row, float *grad_attn_col,
                      void *workspace, size_t workspace_bytes, int64_t v, int64_t n_src, int64_t h, int64_t f,
                      int dtype, void *stream);
COGDL_API int cogdl_hip_edge_dropout_mask(int64_t nnz, int64_t h, float p, uint64_t seed, float *mask, void *stream);
/* the same mask into HOST memory, computed on the host by the same code (no GPU needed: CPU tests pin the generator) */
COGDL_API int cogdl_hip_edge_dropout_mask_host(int64_t nnz, int64_t h, float p, uint64_t seed, float *mask);

/* ---------------------------------------------------------------------------------------
 * Helpers used by the graph-plan cache and the vertex-sharded (multi-GPU) SpMM.
 * fingerprint: 64-bit content hash of (rowptr[0..m], colind[0..nnz)) = the sum modulo 2^64 of the
 * COGDL_HIP_FINGERPRINT_PARTS partials written to out_parts (device memory, or host-mapped pinned memory so that
 * no device-to-host copy is needed; plain stores, no memset, no atomics).  Not part of the reference.
 * ------------------------------------------------------------------------------------- */
#define COGDL_HIP_FINGERPRINT_PARTS 256
COGDL_API int cogdl_hip_csr_fingerprint(const int32_t *rowptr, const int32_t *colind, int64_t m, int64_t nnz,
                              uint64_t *out_parts, void *stream);
/* the same, with every partial ALSO stored to dev_parts (device memory, COGDL_HIP_FINGERPRINT_PARTS entries): for the guarded
 * launches above, which read the hash on the device */
COGDL_API int cogdl_hip_csr_fingerprint_dev(const int32_t *rowptr, const int32_t *colind, int64_t m, int64_t nnz,
                                            uint64_t *out_parts, uint64_t *dev_parts, void *stream);

/* ---------------------------------------------------------------------------------------
 * coo2csr_index on the GPU: stable sort of the edges by row -> (row_ptr[num_nodes+1], perm[nnz]), perm[j] = COO
 * position of CSR entry j (edges of a row keep their COO order).  int64 in and out, like the reference's
 * sampler.coo2csr_cpu_index (cogdl/operators/sample/sample.cpp:234-270), which cogdl/utils/graph_utils.py:133-142
 * reaches through a GPU -> CPU -> GPU round trip and a single-threaded counting sort.  *bad_flag (device int) is set
 * to 1 if a row id lies outside [0, num_nodes).  workspace: cogdl_hip_coo2csr_index_workspace_bytes.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_coo2csr_index_workspace_bytes(int64_t nnz, int64_t num_nodes);
COGDL_API int cogdl_hip_coo2csr_index(const int64_t *row, int64_t nnz, int64_t num_nodes, int64_t *row_ptr,
                            int64_t *perm, int *bad_flag, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * sample_adj on the GPU: neighbour sampling + relabelling of a GPU-resident CSR graph, the contract of
 * sampler.sample_adj (cogdl/operators/sample/sample.cpp:6-144; the reference runs it single-threaded on the CPU
 * with libc rand()) and of cogdl_host_sample_adj (include/cogdl_host.h), int64 in and out, device pointers:
 *   -> out_indptr[batch+1], out_indices[E'] (LOCAL ids), out_nodes[N'] (global id of every local id: the seeds
 *      first, then new nodes in discovery order), out_edges[E'] (CSR positions of the picked edges);
 *   num_neighbors < 0: all neighbours (identical to the reference); replace != 0: num_neighbors uniform draws per
 *   seed with a neighbour; else min(deg, num_neighbors) distinct neighbours (Floyd), emitted in ascending CSR
 *   position; num_neighbors <= 1024 without replacement (else COGDL_HIP_ERANGE).  Seeds must be distinct.
 *   Randomness: a counter-based generator keyed by (seed, seed row, draw) -- reproducible, scheduling-independent.
 *   cap_edges >= sum of the per-seed counts (batch * num_neighbors always suffices for num_neighbors >= 0);
 *   out_nodes holds batch + cap_edges entries.  out_counts (DEVICE int64[3]) = {N', E', flags}; flags != 0 marks
 *   an invalid result: bit 0 seed id out of range, bit 1 neighbour id out of range, bit 2 capacity exceeded.
 *   Nothing synchronises; the caller reads out_counts when it needs the sizes.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_sample_adj_workspace_bytes(int64_t batch, int64_t cap_edges, int64_t num_nodes);
COGDL_API int cogdl_hip_sample_adj(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                         const int64_t *node_idx, int64_t batch, int64_t num_neighbors, int replace,
                         uint64_t seed, int64_t *out_indptr, int64_t *out_indices, int64_t *out_nodes,
                         int64_t *out_edges, int64_t cap_edges, int64_t *out_counts, void *workspace,
                         size_t workspace_bytes, void *stream);

/* sample_adj into buffers of a FIXED capacity, for mini-batch steps captured in a hipGraph (every launch shape is a
 * function of the capacities, never of what was sampled):
 *   batch        = the number of seed SLOTS; *batch_count (device, NULL = all) of them are in use -- hop 2 passes hop 1's
 *                  out_nodes with out_counts[0] as its count;
 *   seed_dev     = device pointer to the RNG seed, NULL = none: the draws use seed + *seed_dev, so the caller bumps the
 *                  device word between replays and tells the hops of one batch apart by the immediate `seed`;
 *   out_indptr   holds batch + cap_edges + 1 entries: rows beyond the seeds in use are empty (= E'), so the block is a
 *                  well-formed CSR over all batch + cap_edges possible nodes (the padding of cogdl/data/data.py:828-830
 *                  at full capacity);
 *   out_indices / out_edges beyond E' are 0, out_nodes beyond N' are 0 (valid ids: a feature gather over the whole
 *                  capacity reads row 0 for them).
 * Everything else as cogdl_hip_sample_adj (same workspace query). */
COGDL_API int cogdl_hip_sample_adj_padded(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                                const int64_t *node_idx, int64_t batch, const int64_t *batch_count,
                                int64_t num_neighbors, int replace, uint64_t seed, const uint64_t *seed_dev,
                                int64_t *out_indptr, int64_t *out_indices, int64_t *out_nodes, int64_t *out_edges,
                                int64_t cap_edges, int64_t *out_counts, void *workspace, size_t workspace_bytes,
                                void *stream);
/* cogdl_hip_sample_adj_padded that ALSO leaves the block as the SpMM takes it -- rowptr32 [batch + 1] (the seed rows
 * only: the rows a layer keeps, graphsage.py:99), col32 [cap_edges] (local ids, 0 behind E') and, unless NULL,
 * inv_deg [batch] = 1 / sampled in-degree (0 for an empty row: Graph.row_norm, cogdl/data/data.py:240-258) -- written by
 * the sampler's own kernels: what cogdl_hip_block_prepare would produce from out_indptr / out_indices, without its
 * launch (a captured mini-batch step pays per dependent kernel node, not per byte). */
COGDL_API int cogdl_hip_sample_adj_block(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                               const int64_t *node_idx, int64_t batch, const int64_t *batch_count,
                               int64_t num_neighbors, int replace, uint64_t seed, const uint64_t *seed_dev,
                               int64_t *out_indptr, int64_t *out_indices, int64_t *out_nodes, int64_t *out_edges,
                               int64_t cap_edges, int64_t *out_counts, int32_t *rowptr32, int32_t *col32,
                               float *inv_deg, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Graph preprocessing on the GPU (what cogdl.data.Graph does once per graph before its first SpMM), int64 COO in and out:
 * add_remaining_self_loops (cogdl/utils/graph_utils.py:40-70 via Adjacency.add_remaining_self_loops,
 *   cogdl/data/data.py:175-191): existing self loops are dropped, one loop per node is appended behind the kept edges
 *   (which keep their order); a node that had loops keeps the weight of its LAST one, the others get fill_value;
 *   val == NULL means unit weights.  Outputs hold nnz + num_nodes entries; *out_count (device) = the number written.
 * coo_norm_weights (graph_utils.py:72-89, degrees as in :10-17 = edges per row): mode 0 (sym)
 *   out[e] = d^-1/2[col[e]] * val[e] * d^-1/2[row[e]], mode 1 (row) out[e] = val[e] / d[row[e]]; 1/0 -> 0.
 * *bad_flag (device int, zeroed by the caller) gets bit 0 if an index lies outside [0, num_nodes).
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_add_remaining_self_loops_workspace_bytes(int64_t nnz, int64_t num_nodes);
COGDL_API int cogdl_hip_add_remaining_self_loops(const int64_t *row, const int64_t *col, const float *val, int64_t nnz,
                                       int64_t num_nodes, float fill_value, int64_t *out_row, int64_t *out_col,
                                       float *out_val, int64_t *out_count, int *bad_flag, void *workspace,
                                       size_t workspace_bytes, void *stream);
COGDL_API size_t cogdl_hip_coo_norm_weights_workspace_bytes(int64_t num_nodes);
COGDL_API int cogdl_hip_coo_norm_weights(const int64_t *row, const int64_t *col, const float *val, int64_t nnz,
                               int64_t num_nodes, int mode, float *out, int *bad_flag, void *workspace,
                               size_t workspace_bytes, void *stream);

/* block_prepare: a sampled block (int64, as sample_adj returns it) as the SpMM takes it, in one launch:
 *   rowptr32[0..n_rows] = row_ptr[0..n_rows], col32[0..n_slots) = col[0..n_slots) narrowed to int32, and (inv_deg != NULL)
 *   inv_deg[r] = 1 / (row_ptr[r+1] - row_ptr[r]), 0 for a row without edges -- the in_norm of Graph.row_norm()
 *   (cogdl/data/data.py:240-258), i.e. the mean aggregator's weights.  n_rows may be smaller than the block's row count
 *   (only the target rows are aggregated), n_slots is the capacity of col (>= row_ptr[n_rows]). */
COGDL_API int cogdl_hip_block_prepare(const int64_t *row_ptr, const int64_t *col, int64_t n_rows, int64_t n_slots,
                            int32_t *rowptr32, int32_t *col32, float *inv_deg, void *stream);

/* ---------------------------------------------------------------------------------------
 * subgraph on the GPU: the node-induced subgraph of a GPU-resident CSR graph, the contract of sampler.subgraph
 * (cogdl/operators/sample/sample.cpp:146-188, reached from Graph.csr_subgraph, cogdl/data/data.py:850-872) and of
 * cogdl_host_subgraph, int64 in and out, device pointers:
 *   row i of the result = row node_idx[i] restricted to the sources that are in node_idx, relabelled to their
 *   position in node_idx (a duplicated id keeps its last position), edges in CSR order;
 *   out_indptr[batch+1], out_indices[E'] (local ids), out_edges[E'] (CSR positions of the kept edges);
 *   cap_edges >= E' (the summed degree of the selected rows always suffices);
 *   out_counts (DEVICE int64[2]) = {E', flags}; flags: bit 0 node id out of range, bit 1 neighbour id out of range,
 *   bit 2 capacity exceeded.  Nothing synchronises.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_subgraph_workspace_bytes(int64_t batch, int64_t num_nodes);
COGDL_API int cogdl_hip_subgraph(const int64_t *indptr, const int64_t *indices, int64_t num_nodes,
                       const int64_t *node_idx, int64_t batch, int64_t *out_indptr, int64_t *out_indices,
                       int64_t *out_edges, int64_t cap_edges, int64_t *out_counts, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Row gathers by node id.
 * gather_feature_rows: out[i,:] = src[ids[i],:], rows of row_bytes bytes (a multiple of 4) -- the mini-batch feature
 *   gather x[n_id] of the sampling pipeline (cogdl/data/sampler.py:82-116, cogdl/models/nn/graphsage.py:86-99).
 *   `src` is a device pointer OR a pointer into PINNED host memory (device-mapped): the selected rows are then read
 *   straight over the host link, overlapping other streams ("zero copy"); `out` is device memory.  ids int64 (what
 *   the sampler returns) or int32 (_i32).  *bad_flag (device int, may be NULL; the caller zeroes it) gets bit 0 if
 *   an id lies outside [0, n_src): such rows are skipped.
 * add_rows_at_f32: out[ids[i],:] += src[i,:] for DISTINCT ids (no atomics): accumulation of returned halo gradients
 *   in the vertex-sharded SpMM backward (cogdl_amd/dist.py).
 * ------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_gather_feature_rows(const int64_t *ids, const void *src, void *out, int64_t n,
                                  int64_t row_bytes, int64_t n_src, int *bad_flag, void *stream);
COGDL_API int cogdl_hip_gather_feature_rows_i32(const int32_t *ids, const void *src, void *out, int64_t n,
                                      int64_t row_bytes, int64_t n_src, int *bad_flag, void *stream);
COGDL_API int cogdl_hip_add_rows_at_f32(const int64_t *ids, const float *src, float *out, int64_t n, int64_t k,
                              int64_t n_dst, int *bad_flag, void *stream);

/* ---------------------------------------------------------------------------------------
 * linear_wgrad: grad_w[out, in] = grad_out[k_rows, out]^T . x[k_rows, in], grad_b[out] = column sums of grad_out
 * (grad_b may be NULL) -- the weight/bias gradient of the `self.linear(x)` inside every CogDL layer
 * (cogdl/layers/gcn_layer.py:52, gat_layer.py:60, sage_layer.py:72; torch.nn.Linear's backward, which torch hands to
 * hipBLASLt).  fp32, row-major, k_rows = number of nodes: a split-K v_mfma_f32_32x32x2_f32 kernel that streams both
 * operands once (csrc/linear_wgrad.hip).  SURVEY.md section 8f rank 3: the one dense product of the path worth a
 * hand-written MFMA kernel.  workspace: cogdl_hip_linear_wgrad_workspace_bytes; x, grad_out 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_linear_wgrad_workspace_bytes(int64_t k_rows, int64_t in_features, int64_t out_features);
COGDL_API int cogdl_hip_linear_wgrad_f32(const float *x, const float *grad_out, float *grad_w, float *grad_b,
                               int64_t k_rows, int64_t in_features, int64_t out_features, void *workspace,
                               size_t workspace_bytes, void *stream);

/* linear_fwd: out[rows, n] = x[rows, k] . B (+ bias[n]) for tall-skinny x (rows = number of nodes), fp32.
 * w_is_n_by_k != 0: B = w^T, w stored [n, k] -- torch.nn.Linear's forward x . W^T + b;
 * w_is_n_by_k == 0: B = w stored [k, n]      -- its grad_input = grad_out . W.
 * Every wave stages 32-row tiles of x through LDS into v_mfma_f32_32x32x2_f32; B stays resident in LDS
 * (csrc/linear_fwd.hip).  Returns COGDL_HIP_EUNSUPPORTED for shapes it does not cover (n > 64 or B larger than 96 KB):
 * the caller then keeps its BLAS call.  x 16-byte aligned. */
COGDL_API int cogdl_hip_linear_fwd_f32(const float *x, const float *w, const float *bias, float *out, int64_t rows,
                             int64_t k_dim, int64_t n_dim, int w_is_n_by_k, void *stream);

/* linear_fwd_bf16 (ABI v9): out[rows, n] (bf16) = bf16(x[rows, k]) . bf16(B) (+ bias[n], fp32 added before the final
 * rounding) -- the same product under bf16 autocast, as torch computes `torch.matmul(x, self.W)` / nn.Linear there
 * (cogdl/layers/gat_layer.py:59 on BASELINE configs[2]: 232,965 x 602 -> 64).  x_dtype / w_dtype: COGDL_HIP_F32 (rounded
 * to bf16 in registers, to nearest even: no bf16 copy of x is made) or COGDL_HIP_BF16; fp32 accumulation in
 * v_mfma_f32_32x32x16_bf16, whose operands are eight CONSECUTIVE k per lane: rows of x are read straight from global
 * memory, B sits in LDS in operand order (csrc/linear_fwd16.hip).  w_is_n_by_k as above.  COGDL_HIP_EUNSUPPORTED: n > 64,
 * more than 128 KB of bf16 B operands, bf16 rows of odd length.  x 16-byte aligned. */
COGDL_API int cogdl_hip_linear_fwd_bf16(const void *x, int x_dtype, const void *w, int w_dtype, const float *bias, void *out,
                              int64_t rows, int64_t k_dim, int64_t n_dim, int w_is_n_by_k, void *stream);
/* head_projection_fwd (ABI v9): h_l[v, h] = sum_f a_l[h, f] * feat[v, h, f] and h_r likewise with a_r -- both attention
 * projections of GATLayer.forward (cogdl/layers/gat_layer.py:65-66) in one pass over feat [n_rows, heads, f_dim] (f32 / f16 /
 * bf16); a_l, a_r [heads, f_dim] fp32; h_l, h_r [n_rows, heads] fp32.  fp32 products summed left to right
 * (csrc/head_proj.hip). */
COGDL_API int cogdl_hip_head_projection_fwd(const void *feat, int dtype, const float *a_l, const float *a_r, float *h_l, float *h_r,
                                  int64_t n_rows, int64_t heads, int64_t f_dim, void *stream);

/* linear_fwd_f16: the same kernel on v_mfma_f32_32x32x16_f16 -- the autocast dtype of the reference's own Trainer(fp16=True)
 * (cogdl/trainer/trainer.py: torch.cuda.amp.autocast); x_dtype / w_dtype: COGDL_HIP_F32 or COGDL_HIP_F16, out f16. */
COGDL_API int cogdl_hip_linear_fwd_f16(const void *x, int x_dtype, const void *w, int w_dtype, const float *bias, void *out,
                             int64_t rows, int64_t k_dim, int64_t n_dim, int w_is_n_by_k, void *stream);

/* ---------------------------------------------------------------------------------------
 * Vertex-sharded graphs (BASELINE.json configs[4]; no reference counterpart -- CogDL only partitions on the host, with
 * METIS, for ClusterGCN: cogdl/data/sampler.py:188-243).  csrc/shard.hip.
 * shard_count / shard_fill: one rank's shard of a 1-D row-partitioned CSR matrix.  The rank owns the rows [lo, hi) =
 *   n_local rows, `rowptr` [n_local + 1] (int64; it may start at any offset: rowptr[0] is subtracted), `col` [nnz]
 *   GLOBAL column ids in [0, n_global), `weight` [nnz] fp32 or NULL.
 *   count: counts[4] (DEVICE int64) = {edges with a column inside [lo, hi), edges outside, distinct outside columns
 *          (= halo rows), flags (bit 0: a column id outside [0, n_global))}.  The caller reads them (the one
 *          synchronisation of building a shard) and allocates the outputs of
 *   fill : rowptr_loc / rowptr_rem [n_local + 1] int32, colind_loc [counts[0]] = col - lo, colind_rem [counts[1]] =
 *          index into the halo table, w_loc / w_rem (NULL iff weight is NULL), halo_ids [counts[2]] = the distinct
 *          outside columns ascending (int64), cut [n_bounds] (int64) = halo ids below bounds[q] -- with
 *          bounds = the partition's row ranges that is where every owner's part of the halo table starts.
 *   A row's edges keep their CSR order inside both blocks.  The same workspace (cogdl_hip_shard_workspace_bytes) must
 *   be passed to both calls, untouched in between.  n_global < 2^31 - 1, nnz < 2^31.
 * bfs_step: one level of a breadth-first search over a CSR graph (int64 rowptr / col, n vertices): every vertex with
 *   level[v] == cur gives its unvisited (level < 0) neighbours the level cur + 1; *changed (device int, zeroed by the
 *   caller) is set when it did.  The caller loops over the levels (cogdl_amd/dist.py: bfs_order, the locality
 *   reordering in front of a contiguous partition).
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_shard_workspace_bytes(int64_t n_local, int64_t n_global);
COGDL_API int cogdl_hip_shard_count(const int64_t *rowptr, const int64_t *col, int64_t n_local, int64_t nnz, int64_t lo,
                          int64_t hi, int64_t n_global, int64_t *counts, void *workspace, size_t workspace_bytes,
                          void *stream);
COGDL_API int cogdl_hip_shard_fill(const int64_t *rowptr, const int64_t *col, const float *weight, int64_t n_local,
                         int64_t nnz, int64_t lo, int64_t hi, int64_t n_global, const int64_t *bounds, int64_t n_bounds,
                         int32_t *rowptr_loc, int32_t *colind_loc, float *w_loc, int32_t *rowptr_rem,
                         int32_t *colind_rem, float *w_rem, int64_t *halo_ids, int64_t *cut, void *workspace,
                         size_t workspace_bytes, void *stream);
COGDL_API int cogdl_hip_bfs_step(const int64_t *rowptr, const int64_t *col, int64_t n, int32_t *level, int32_t cur,
                       int *changed, void *stream);

/* ---------------------------------------------------------------------------------------
 * spgemm: C = A . B, A [m, k] and B [k, n] int32 CSR with fp32 values, C canonical CSR (columns ascending and unique
 * inside a row).  The contract of torch_sparse.spspmm (reached by the reference's srgcn / graph_unet / gtn models)
 * and of torch.sparse.mm: the pattern is STRUCTURAL -- every (i, j) with a product A[i,k] B[k,j] is in C, an entry
 * whose products sum to 0.0 included.  A and B need not be canonical (duplicate columns are summed like any other
 * products).  Every value of C is the sum of its products in expansion order (A_i's entries in CSR order, then B_k's),
 * added by one thread: bit-identical results on every call, no float atomics.  m, k, n < 2^31, nnz(C) < 2^31.
 * The output size depends on the data, so a product is a short host-driven sequence (not hipGraph-capturable):
 *   1. count   plan: caller-owned, cogdl_hip_spgemm_plan_bytes(m) bytes (8-byte aligned), kept until fill.
 *              Writes rowptrC [m+1] and the plan's DEVICE header, int64 hdr[8] at the plan's start:
 *              hdr[3] = n_hub (rows whose products exceed the 4096 an LDS table holds), hdr[4] = their number of
 *              products, hdr[5] = nnz(C) (hub rows counted as 0 while n_hub > 0).  The caller reads the header: the
 *              one synchronisation of a product without hub rows; rowptrC is valid only when hdr[5] < 2^31.
 *   2. hub rows only (hdr[3] > 0): expand writes their products, row by row in expansion order, as a CSR
 *              hub_rowptr [n_hub+1], hub_col / hub_val [hdr[4]] (hdr[4] <= COGDL_HIP_SEGMENT_MAX_EDGES, else
 *              COGDL_HIP_ERANGE); the caller makes it canonical (cogdl_hip_csr2csc twice, then cogdl_hip_coo_dupsum with
 *              the composed permutation: sums in expansion order) and passes the canonical CSR to rowptr, which
 *              rewrites rowptrC and hdr[5] (a second synchronisation), and to fill.
 *   3. fill    colC / valC [nnzC] (nnzC = hdr[5] as read by the caller).
 * count / rowptr workspace: cogdl_hip_spgemm_count_workspace_bytes(m); expand: cogdl_hip_spgemm_expand_workspace_bytes.
 * Backward (values only; every output has one owner, no atomics):
 *   grad_a: gradA[(i,k)] = sum_j gradC[i,j] B[k,j]  (B_k's entries looked up in row i of C; needs C canonical)
 *   grad_b: gradB[(k,j)] = sum_i A[i,k] gradC[i,j]  over column k of A: colptrAT [k+1] / rowindAT / permAT of
 *           cogdl_hip_csr2csc(rowptrA, colA, m, k), A's values read as valA[permAT[q]].
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_spgemm_plan_bytes(int64_t m);
COGDL_API size_t cogdl_hip_spgemm_count_workspace_bytes(int64_t m);
COGDL_API int cogdl_hip_spgemm_count(const int32_t *rowptrA, const int32_t *colA, const int32_t *rowptrB, const int32_t *colB,
                           int64_t m, int64_t k, int64_t n, void *plan, int32_t *rowptrC, void *workspace,
                           size_t workspace_bytes, void *stream);
COGDL_API size_t cogdl_hip_spgemm_expand_workspace_bytes(int64_t n_hub);
COGDL_API int cogdl_hip_spgemm_expand(const int32_t *rowptrA, const int32_t *colA, const float *valA, const int32_t *rowptrB,
                            const int32_t *colB, const float *valB, int64_t m, const void *plan, int64_t n_hub,
                            int64_t hub_products, int32_t *hub_rowptr, int32_t *hub_col, float *hub_val, void *workspace,
                            size_t workspace_bytes, void *stream);
COGDL_API size_t cogdl_hip_spgemm_rowptr_workspace_bytes(int64_t m);
COGDL_API int cogdl_hip_spgemm_rowptr(void *plan, int64_t m, int64_t n_hub, const int32_t *hub_rowptr, int32_t *rowptrC,
                            void *workspace, size_t workspace_bytes, void *stream);
COGDL_API int cogdl_hip_spgemm_fill(const int32_t *rowptrA, const int32_t *colA, const float *valA, const int32_t *rowptrB,
                          const int32_t *colB, const float *valB, int64_t m, int64_t k, int64_t n, const void *plan,
                          const int32_t *rowptrC, int64_t nnzC, int32_t *colC, float *valC, int64_t n_hub,
                          const int32_t *hub_rowptr, const int32_t *hub_col, const float *hub_val, void *stream);
COGDL_API int cogdl_hip_spgemm_grad_a(const int32_t *rowptrA, const int32_t *colA, const int32_t *rowptrB, const int32_t *colB,
                            const float *valB, const int32_t *rowptrC, const int32_t *colC, const float *gradC,
                            float *gradA, int64_t m, int64_t nnzA, void *stream);
COGDL_API int cogdl_hip_spgemm_grad_b(const int32_t *colptrAT, const int32_t *rowindAT, const int32_t *permAT, const float *valA,
                            const int32_t *rowptrB, const int32_t *colB, const int32_t *rowptrC, const int32_t *colC,
                            const float *gradC, float *gradB, int64_t k, int64_t nnzB, void *stream);

/* ---------------------------------------------------------------------------------------
 * coo_dupsum: the segmented duplicate sum of COO canonicalisation.  In: a CSR whose rows are sorted by column
 * (duplicates adjacent) -- rowptr [rows+1], col [nnz] -- and `order` [nnz] (NULL = identity): sorted position t holds
 * input entry order[t].  Out: rowptr_u [rows+1] and col_u of the distinct (row, col) pairs, val_u[u] = the sum of
 * val[order[t]] over the run, added in sorted order by one thread (val / val_u may both be NULL: structure only),
 * map[order[t]] = u (NULL: not written).  col_u / val_u need room for rowptr_u[rows] <= nnz entries.
 * workspace: cogdl_hip_coo_dupsum_workspace_bytes(nnz), 256-byte aligned.  nnz <= COGDL_HIP_SEGMENT_MAX_EDGES.
 * ------------------------------------------------------------------------------------- */
COGDL_API size_t cogdl_hip_coo_dupsum_workspace_bytes(int64_t nnz);
COGDL_API int cogdl_hip_coo_dupsum(const int32_t *rowptr, const int32_t *col, const int32_t *order, const float *val,
                         int64_t rows, int64_t nnz, int32_t *rowptr_u, int32_t *col_u, float *val_u, int32_t *map,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Random walks on a GPU-resident CSR graph (csrc/walk.hip): int64 indptr[num_nodes + 1] / indices[num_edges] (what
 * cogdl.data.Graph holds and cogdl_hip_sample_adj takes), int64 start[W], result int64 walks[W, length] row-major.
 * Stream-ordered, one launch (plus one word fill), no host round trip, no atomics, no workspace; hipGraph-capturable.
 * Replaces the numba / interpreted loops of cogdl/utils/sampling.py:14-67 (RandomWalker.walk) and the transition rule
 * of cogdl/models/emb/node2vec.py:143-156.  Host twin with identical results: cogdl_host_random_walk /
 * cogdl_host_node2vec_walk (include/cogdl_host.h).
 *   random_walk    walks[w, 0] = start[w].  Step i >= 1: with probability 1 - restart_p the walker moves to a uniformly
 *                  drawn out-neighbour of its current node, with probability restart_p to a uniformly drawn
 *                  out-neighbour of its START node (as in the reference, a restart lands on a neighbour of the start, not
 *                  on the start).  restart_p in [0, 1]: 0 never restarts, 1 always does.
 *   node2vec_walk  unweighted graph, return parameter p > 0, in-out parameter q > 0.  Step 1 is uniform; afterwards, with
 *                  previous node t and current node v, a neighbour x of v has weight 1/p if x == t, 1 if t is in row x
 *                  of the CSR, else 1/q.  ROWS MUST BE SORTED BY COLUMN (the membership test is a binary search).
 *                  Rejection sampling against max(1, 1/p, 1/q) for at most max_trials trials per step (0 = the default,
 *                  256), then one exact pass over the row (weights summed, inverse CDF): the law is exact and every step
 *                  terminates.  Weights are 32.32 fixed point relative to the largest.  Rows of fewer than 2^32 edges.
 *                  fallback_steps: NULL, or device int32[W] receiving per walker the number of steps the exact pass decided.
 *   Dead ends      A node without out-neighbours: the reference is undefined there (random.randint on an empty range).
 *                  Here the walker stays and the node is repeated, so every entry of walks is a valid node id.
 *   Randomness     a pure function of (seed, walker w, step i, trial) through Philox4x32-10 (csrc/walk_draw.h), independent
 *                  of launch shape and scheduling; length < 2^31.
 *   flags          DEVICE int, zeroed by the call: bit 0 a start id outside [0, num_nodes), bit 1 a neighbour id outside,
 *                  bit 2 a row of indptr that is not a range inside [0, num_edges].  A walker that meets one parks (repeats
 *                  its node, reads nothing more); nothing is read out of bounds.  Non-zero marks an invalid result; when
 *                  several conditions occur in one call a bit may be missing, the word is never zero then.
 *   W = 0 and length = 1 are valid; offsets are 64-bit throughout (num_edges >= 2^31 is fine).
 * ------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_random_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                          const int64_t *start, int64_t n_walkers, int64_t length, double restart_p, uint64_t seed,
                          int64_t *walks, int *flags, void *stream);
COGDL_API int cogdl_hip_node2vec_walk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                            const int64_t *start, int64_t n_walkers, int64_t length, double p, double q, int max_trials,
                            uint64_t seed, int64_t *walks, int32_t *fallback_steps, int *flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * Metapath-constrained random walk (csrc/walk.hip: metapath_walk_kernel), replacing the interpreted loop of
 * cogdl/models/emb/metapath2vec.py:87-125 (_walk / _simulate_walks; gatne.py:277-336 and hin2vec.py:60-82 use the same step).
 * Stream-ordered, one launch (plus one word fill), no atomics, no workspace.  Host twin with identical results:
 * cogdl_host_metapath_walk (include/cogdl_host.h).
 *   Typed layout   T = num_types node types.  seg: int64[num_nodes * T + 1]; indices_t[seg[v * T + t] .. seg[v * T + t + 1])
 *                  are the neighbours of v whose type is t, so seg[v * T] is the row pointer of v and seg[num_nodes * T] =
 *                  num_edges (cogdl_amd/operators/walk.py: typed_rows builds it with cogdl_hip_coo2csr_index).  With T = 1
 *                  (seg, indices_t) is the plain CSR.
 *   Metapaths      pattern / path_off: int32; metapath p is pattern[path_off[p] .. path_off[p + 1]), the node types of one
 *                  PERIOD: the schema "1-0-2-0-1" is (1, 0, 2, 0), its repeated last item left out.  path_off[n_paths + 1]
 *                  entries, increasing from >= 0.  walker_path[w] in [0, n_paths) is the metapath of walker w.
 *   Walk           walks[w, 0] = start[w].  At position i >= 1 the wanted type is t = pattern[path_off[p] + i mod P], P the
 *                  period (the reference's schema_items[len(walk) % (len(schema_items) - 1)]), and the walker moves to a
 *                  uniformly drawn entry of the segment (v, t), multiplicity counting.  An empty segment ENDS the walk: this
 *                  position and every later one hold -1 (the reference's `break`), and the walker reads nothing more.
 *                  lengths: NULL, or int32[W] receiving the number of positions that hold a node (1 for a walker that raised
 *                  a flag at position 0).
 *   Randomness     the draw of cogdl_hip_random_walk: Philox4x32-10 of (seed, w, i, trial 0).  With T = 1, the one metapath
 *                  (0) and a graph without dead ends the result equals cogdl_hip_random_walk(restart_p = 0) bit for bit.
 *   node_type      NULL, or int32[num_nodes]: then the type of start[w] must be pattern[path_off[p]] (flag bit 3): one load
 *                  per walker.
 *   flags          DEVICE int, zeroed by the call: bits 0 .. 2 as in cogdl_hip_random_walk (bit 2 for a segment that is not
 *                  a range inside [0, num_edges]), bit 3 (8) a start node of the wrong type, bit 4 (16) a wanted type outside
 *                  [0, T), a walker_path entry outside [0, n_paths) or a malformed path_off.  A walker that raises one writes
 *                  -1 from then on and reads nothing; nothing is read out of bounds.  Non-zero marks an invalid result; when
 *                  several conditions occur in one call a bit may be missing, the word is never zero then.
 *   num_types outside [1, 64], n_paths < 1, a null walker_path / pattern / path_off with W > 0: COGDL_HIP_EINVAL.
 * ------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_metapath_walk(const int64_t *seg, const int64_t *indices_t, int64_t num_nodes, int32_t num_types,
                            int64_t num_edges, const int32_t *node_type, const int64_t *start, const int32_t *walker_path,
                            int64_t n_walkers, int64_t length, const int32_t *pattern, const int32_t *path_off,
                            int32_t n_paths, uint64_t seed, int64_t *walks, int32_t *lengths, int *flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * NetSMF path sampling on a GPU-resident CSR graph (csrc/netsmf.hip): int64 indptr[num_nodes + 1] / indices[num_edges], unit
 * weights; result int32 out_row / out_col of window * n_samples entries each.
 * Stream-ordered, one launch (plus one word fill), no host round trip, no atomics, no workspace; hipGraph-capturable.
 * Replaces the interpreted loop of cogdl/models/emb/netsmf.py:134-159 (_path_sampling / _random_walk_matrix).  Host twin
 * with identical results: cogdl_host_netsmf_sample (include/cogdl_host.h).  The law is csrc/netsmf_law.h's:
 *   sample (s, r)  s in [first_sample, first_sample + n_samples), r in [1, window].  e = s mod num_edges; u = the row that
 *                  holds entry e (empty rows are skipped), v = indices[e]; k uniform on 1 .. r; u takes k - 1 uniform
 *                  steps, v takes r - k.  The pair is written at j = (r - 1) * n_samples + (s - first_sample).
 *   One pass       s = 0 .. num_edges - 1 visits every entry once: on a simple symmetric graph `num_round` rounds of the
 *                  reference (each undirected edge once, with a fair flip of its orientation) have the law of
 *                  num_round / 2 passes.
 *   Dead ends      at a node without out-neighbours the walker stays, as in cogdl_hip_random_walk.
 *   Randomness     a pure function of (seed, s, r, step i) through Philox4x32-10 (csrc/walk_draw.h): independent of launch
 *                  shape, of scheduling, and of how a range of samples is cut into calls.
 *   flags          DEVICE int, zeroed by the call: bit 1 a neighbour id outside [0, num_nodes), bit 2 a row of indptr that
 *                  is not a range inside [0, num_edges] or does not hold the entry it should.  Such a sample writes
 *                  (-1, -1); nothing is read out of bounds.  Non-zero marks an invalid result; when both conditions occur
 *                  in one call a bit may be missing, the word is never zero then.
 *   n_samples = 0 is valid (the flags word is still zeroed).  window outside [1, 256], num_edges = 0 or num_nodes = 0 with
 *   n_samples > 0, a negative size: COGDL_HIP_EINVAL.  num_nodes >= 2^31 (pairs are int32) or n_samples > 2^53:
 *   COGDL_HIP_ERANGE.  Offsets are 64-bit throughout (num_edges and window * n_samples >= 2^31 are fine).
 * ------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_netsmf_sample(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                            int64_t first_sample, int64_t n_samples, int window, uint64_t seed, int32_t *out_row,
                            int32_t *out_col, int *flags, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Top-k personalised PageRank by forward push (csrc/ppr.hip), replacing the numba / interpreted loop of
 * cogdl/utils/ppr_utils.py:8-48.  int64 indptr[num_nodes + 1] / indices[num_edges] on the device, deg[u] =
 * indptr[u + 1] - indptr[u], int64 sources[S].  Host twin with identical results: cogdl_host_ppr_topk.
 *   Process     per source s: r[s] = alpha; pushing u does res = r[u]; p[u] += res; r[u] = 0; r[v] += (1 - alpha) * res /
 *               deg[u] for every entry v of u's row.  Round 0 pushes s; round t pushes exactly the nodes with r > 0 and
 *               r >= alpha * eps * deg at its start; the process ends when there are none.  (The reference pushes in LIFO
 *               order, so its values differ within the bound below.)
 *   Arithmetic  r and p are unsigned 64-bit multiples of 2^-62 and the share is floored (csrc/ppr_fixed.h), so additions
 *               commute: the result is a function of the inputs alone, equal from run to run and equal to the host twin's.
 *   Guarantees  on return r[v] < alpha * eps * deg[v] for every v; p never exceeds the exact PPR row pi_s, and on a
 *               symmetric structure pi_s[t] - p[t] < eps * deg[t] + 2^-24 (2^-24 bounds the flooring loss).
 *   Accepted    alpha in (0, 1), eps > 0, alpha * eps >= 2^-20, and 4 (E + budget + 2) / alpha * 2^-62 < 2^-24 with
 *               budget = floor(2^62 / floor(alpha * eps * 2^62)) + 1; otherwise COGDL_HIP_EINVAL / COGDL_HIP_ERANGE and the
 *               workspace query returns 0.
 *   Output      of the touched nodes with p > 0 the topk largest by p, ties by smaller node id, in that order:
 *               nbr int64[S, topk] (unused slots -1), val float32[S, topk] (p rounded to nearest; unused 0),
 *               count int32[S].  stats: NULL, or int32[S, 2] receiving rounds and touched nodes per source.
 *   Tables      a source touches at most 1 + deg[s] + budget nodes; max_source_degree must bound deg[s] over the sources
 *               (the tables are sized from it; a value that is too small raises bit 3, nothing overflows).
 *   *flags      device int, zeroed by the call: bit 0 a source id outside [0, num_nodes), bit 1 a neighbour id outside,
 *               bit 2 a row of indptr that is not a range inside [0, num_edges], bit 3 table full, bit 4 round bound
 *               reached.  A source that meets one ends with count 0 and an empty row; nothing is read out of bounds and
 *               every device loop is bounded.  Non-zero marks an invalid result.
 *   The call enqueues on `stream`, allocates nothing and does not synchronise; ws must hold
 *   cogdl_hip_ppr_topk_workspace_bytes(...) bytes (16-byte aligned) and is bounded whatever S is (a persistent grid). */
COGDL_API size_t cogdl_hip_ppr_topk_workspace_bytes(int64_t num_nodes, int64_t num_edges, int64_t max_source_degree,
                                          double alpha, double eps, int64_t n_sources);
COGDL_API int cogdl_hip_ppr_topk(const int64_t *indptr, const int64_t *indices, int64_t num_nodes, int64_t num_edges,
                       const int64_t *sources, int64_t n_sources, int64_t max_source_degree, double alpha, double eps,
                       int64_t topk, int64_t *nbr, float *val, int32_t *count, int32_t *stats, int *flags, void *ws,
                       size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Skip-gram training with negative sampling (csrc/sgns.hip): the trainer behind gensim's Word2Vec(sg=1, negative=K) as
 * cogdl/models/emb/deepwalk.py:54-80 and node2vec.py:72-103 call it, on walks that are already on the device.  The law --
 * draws, order of updates, every rounding -- is csrc/sgns_law.h.  Host twin: cogdl_host_sgns_init / cogdl_host_sgns_train.
 *   walks        int64 [W, L] row-major, ids in [0, V); a negative id is padding and is skipped.  L <= 1024.
 *   D, window, negative   1..512, 1..32, 1..16.  epochs >= 1.  The learning rate falls linearly from alpha (first row of
 *                the first epoch) towards min_alpha over epochs * W rows.
 *   keep         uint32 [V]: a token is kept iff its draw <= keep[id] (2^32 - 1 keeps always).
 *   cum          uint32 [V]: cumulative noise table, non-decreasing, last entry >= 1 (callers build 2^31 - 1).
 *   exp_table    float [1000]: word2vec.c's sigmoid table, exp_table[i] = s / (s + 1), s = exp((2 i / 1000 - 1) * 6).
 *   syn0, syn1   float [V, D] row-major, read and updated in place (cogdl_hip_sgns_init fills syn0 from the seed and
 *                zeroes syn1; a caller may pass tables of its own to continue training).
 *   workers      1: one launch of one wave, rows in order; the result equals the host twin's bit for bit.  Slow by
 *                construction.  Anything else: launches of at most rows_in_flight rows (0 = the library's default) in row
 *                order; the rows of one launch run concurrently and update the tables without locks, so results differ
 *                from run to run.
 *   *flags       device int, zeroed by the call, then set by a validation pass that runs before any update: bit 0 an id
 *                >= V, bit 1 a cum that runs backwards or ends in 0.  Non-zero: the tables were not touched.  Nothing is
 *                read out of bounds.
 *   Stream-ordered, allocates nothing, does not synchronise.  Tuning key 17 selects the row update: 0 memory-side
 *   atomicAdd(float) (default), 1 write-through read-modify-write stores.
 * ------------------------------------------------------------------------------------------------------------------ */
COGDL_API int cogdl_hip_sgns_init(float *syn0, float *syn1, int64_t V, int D, uint64_t seed, void *stream);
COGDL_API int cogdl_hip_sgns_train(const int64_t *walks, int64_t W, int64_t L, int64_t V, int D, int window, int negative,
                         int64_t epochs, double alpha, double min_alpha, const uint32_t *keep, const uint32_t *cum,
                         const float *exp_table, uint64_t seed, int workers, int64_t rows_in_flight, float *syn0,
                         float *syn1, int *flags, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Batched graph readout (csrc/readout.hip): x[N, F] node rows and the sorted `batch` vector of a mini-batch of graphs ->
 * one row (segment pooling) or k rows (sort-pool) per graph.  Replaces the zeros + scatter_add_ of batch_sum_pooling /
 * batch_mean_pooling (cogdl/utils/utils.py:192-203) and of GIN's forward (models/nn/gin.py:111-112), the CSR detour of
 * batch_max_pooling (utils.py:206-221) and the dense pad + sort + gather of SortPool (models/nn/sortpool.py:111-127).
 * float32, row-major, on `stream`; no atomics, no allocation, no synchronisation, nothing read back.  The order of every
 * addition and the sort order are csrc/readout_law.h's; the host twins (cogdl_host_*, same names) return the same bytes.
 *   ptr          int32 [B + 1]: graph g owns the rows [ptr[g], ptr[g + 1]).  A caller's ptr is trusted, but every row index
 *                is clamped into [0, N]: a malformed ptr gives wrong numbers, never an access outside the arrays.
 *   segment_ptr  int64 batch[N] with values in [0, B) -> ptr; ids that do not occur get empty segments.  *flag (device
 *                int, zeroed by the call) becomes non-zero if batch is not non-decreasing or holds a value outside [0, B);
 *                ptr is then not to be relied on.
 *   mode         0 sum, 1 mean, 2 max.
 *     sum        per column, float32 additions in increasing row order starting from +0.0f -- bit for bit what torch's CPU
 *                scatter_add_ gives -- for segments of up to cogdl_hip_segment_exact_nodes() rows (4096).  A longer segment
 *                is cut into chunks of 1024 rows dealt round-robin to four accumulators that are added in a fixed order:
 *                equal from run to run and equal to the host twin, no longer the sequential association.
 *     mean       that sum, then one division by (float)rows.
 *     max        the maximum and, in argmax int32 [B, F], its row; ties go to the smallest row.
 *     An empty segment gives 0 (argmax -1).
 *     NaN        sum / mean: IEEE propagation.  max: a row is taken only if x > best, starting from -inf, so a NaN is never
 *                the maximum; a column with nothing above -inf in its segment gives -inf and the segment's first row.
 *   pool_bwd     grad_x[i, :] from grad[B, F] as a gather, every element of grad_x written once (no zero-fill pass):
 *                sum grad[g], mean grad[g] / (float)rows, max grad[g, f] where argmax[g, f] == i, else 0.  The graph of
 *                row i is batch[i] where batch is passed (int64 [N], may be NULL), else found in ptr by binary search.
 *   sort_pool    per graph the min(k, n_g) rows with the largest x[i, key_col] in descending key order, equal keys in
 *                increasing row order (-0 equals +0; a NaN key counts as the largest): out [B, k, F], rows past n_g zero;
 *                idx int32 [B, k] the source rows, -1 there.  One workgroup per graph; graphs of up to
 *                cogdl_hip_sort_pool_lds_nodes() rows are sorted in LDS, larger ones by counting ranks through the
 *                workspace (O(n_g^2) comparisons: slow, same result).  workspace: cogdl_hip_sort_pool_workspace_bytes(N)
 *                bytes, 8-byte aligned (0 for N within the LDS bound: no graph can exceed it).
 *   sort_pool_bwd  grad_x [N, F] = zeros, then row idx[g, j] = grad[g, j, :] (each node occurs at most once).
 * N == 0 or B == 0: success, nothing launched.  N, B, F, k, B * k or B * ceil(F / 64) beyond 2^31 - 1: COGDL_HIP_ERANGE.
 * ------------------------------------------------------------------------------------------------------------------ */
COGDL_API int cogdl_hip_segment_exact_nodes(void);
COGDL_API int cogdl_hip_sort_pool_lds_nodes(void);
COGDL_API int cogdl_hip_segment_ptr(const int64_t *batch, int64_t N, int64_t B, int32_t *ptr, int *flag, void *stream);
COGDL_API int cogdl_hip_segment_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int mode,
                               float *out, int32_t *argmax, void *stream);
COGDL_API int cogdl_hip_segment_pool_bwd(const float *grad, const int32_t *ptr, const int64_t *batch, const int32_t *argmax,
                               int64_t N, int64_t B, int64_t F, int mode, float *grad_x, void *stream);
COGDL_API size_t cogdl_hip_sort_pool_workspace_bytes(int64_t N);
COGDL_API int cogdl_hip_sort_pool_fwd(const float *x, const int32_t *ptr, int64_t N, int64_t B, int64_t F, int64_t k,
                            int64_t key_col, float *out, int32_t *idx, void *workspace, size_t workspace_bytes,
                            void *stream);
COGDL_API int cogdl_hip_sort_pool_bwd(const float *grad, const int32_t *idx, int64_t N, int64_t B, int64_t F, int64_t k,
                            float *grad_x, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * One step of a polynomial graph filter (added within ABI v9: a new symbol only; csrc/polyfilter.hip).  What the spectral
 * propagation of ProNE and the heat-kernel / PPR / Gaussian filters iterate (cogdl/utils/prone_utils.py:26-176: a
 * three-term recurrence on an [n, k] matrix, there one scipy product plus 2-5 elementwise passes per term), as ONE launch.
 * For a square CSR structure (int32 rowptr [n + 1], colind [nnz], val fp32 [nnz] or NULL: unweighted), fp32 row-major
 * [n, k] tensors and host scalars:
 *     t[i,:]   = sum over the row's edges of val[e] * x[colind[e],:]
 *     s        = dst_scale[i] * t[i,:]                 (only when dst_scale is given)
 *     y        = a * s
 *     y        = y + b  * x[i,:]                       (only when b != 0)
 *     y        = y + c1 * z1[i,:]                      (only when z1 is given)
 *     y        = y + c2 * z2[i,:]                      (only when z2 is given)
 *     out[i,:] = y
 *     acc[i,:] = acc[i,:] + d * y                      (only when acc is given)
 * Arithmetic: t is cogdl_hip_csr_spmm's sum for the same operands, bit for bit, on every row of at most
 * cogdl_hip_exact_row_edges(nnz) edges (one sequential sum, whatever the lanes).  The launch is the same functor with the
 * geometry csr_spmm takes at this k for the LEAST aligned of x, out, z1, z2 and acc, so an operand that starts mid-allocation
 * narrows the lanes instead of failing the call.  A longer row is summed in pieces whose cut follows the number of lane groups,
 * hence the lane width: it equals csr_spmm's sum for these x / out bit for bit while z1, z2 and acc are at least as aligned as
 * x and out (the geometries are then the same), and up to re-association of the pieces otherwise.  Every product and every
 * sum of the epilogue is a separately rounded fp32 operation, left to right as written (no fused multiply-add).  An absent
 * operand is never read and its term is skipped, not multiplied by zero.  A row without edges has t = 0 and still gets its
 * epilogue.
 * Aliasing: out may be z1 or z2, acc may be z1 or z2 (each lane reads its columns before it writes them).  out overlapping
 * x or acc, acc overlapping x, or a z that overlaps out / acc without being it: COGDL_HIP_EINVAL.
 * dtype != COGDL_HIP_F32: COGDL_HIP_EUNSUPPORTED.  n == 0 or k == 0: success, nothing launched.  k or nnz beyond what one
 * launch addresses: COGDL_HIP_ERANGE.  A pointer not aligned to 4 bytes: COGDL_HIP_EALIGN.
 * workspace: cogdl_hip_csr_spmm_workspace_bytes(nnz, k, COGDL_HIP_F32) bytes (NULL: rows of any length are summed
 * sequentially).  Launches on `stream`; no XCD plan, no sweep layout, no 16-bit operands.
 * ------------------------------------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_csr_filter_step(const int32_t *rowptr, const int32_t *colind, const void *val, const void *x, void *out,
                              int64_t n, int64_t k, int64_t nnz, int dtype, float a, float b, const void *z1, float c1,
                              const void *z2, float c2, const float *dst_scale, void *acc, float d, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * All-entity ranking for knowledge-graph link prediction (added within ABI v9: new symbols only; csrc/kgrank.hip).  For each
 * of M prepared query rows q[i] (fp32 [M, D]) and its target[i] (int32 [M], in [0, N)): how many rows e of table (fp32
 * [N, D]) score above the target's row, and how many score equal, without a [M, N] score matrix or a sort:
 *     counts[i] = (greater, equal_before, equal_after)     int32 [M, 3]
 *                 over the candidates e != target[i] that filter list i does not name:
 *                 s(i, e) > s(i, t);   s(i, e) == s(i, t) and e < t;   s(i, e) == s(i, t) and e > t
 * kind  COGDL_HIP_KG_DOT  s = SUM_k q[k] * table[e, k]                              (fp32 MFMA; gamma is not read)
 *       COGDL_HIP_KG_L1   s = gamma - SUM_k |q[k] - table[e, k]|                    (VALU)
 *       COGDL_HIP_KG_CL2  s = gamma - SUM_{k < D/2} |(q[k] - table[e, k]) + i (q[k + D/2] - table[e, k + D/2])|   (VALU; D even)
 * The order of every float32 operation is csrc/kgrank_law.h's: one pass over k in ascending order per pair of rows, no split
 * over k, the target's score from the same operations as a candidate's -- so `==` is exact, the counts are integers, and
 * both are equal from run to run and equal to the host twin's (cogdl_host_kg_rank).  A NaN score is counted nowhere.
 * filt_ptr int32 [M + 1] (non-decreasing, filt_ptr[0] = 0, filt_ptr[M] = filt_len), filt_idx int32 [filt_len]: per query the
 * ids to leave out, IN NON-DECREASING ORDER within a query (the pass recognises a duplicate as an entry equal to its
 * predecessor and counts it once); the target is never left out even if listed.  filt_len == 0: no filter, both may be NULL.
 * The filter is a correction pass after the count over all N: one score per list entry under the same law.
 * Ids outside [0, N) (a target: its counts are 0; a list entry: passed over) and a malformed filt_ptr give wrong numbers,
 * never an access outside the operands.
 * workspace: cogdl_hip_kg_rank_workspace_bytes(M, N, D, kind) bytes, 4-byte aligned (the targets' scores).  Launches on
 * `stream`; no allocation, no synchronisation, no host read.  M == 0: success, nothing launched.  Pointers aligned to 4 bytes
 * (COGDL_HIP_EALIGN otherwise); an unknown kind, odd D with CL2 or a negative size: COGDL_HIP_EINVAL; sizes of 2^31 - 1 and
 * more: COGDL_HIP_ERANGE.
 * cogdl_hip_kg_rank_slice_entities: the number of consecutive table rows one workgroup of the counting launch walks for
 * these sizes (slice s covers rows [s * len, (s + 1) * len)); for tests that place targets on slice boundaries.
 * ------------------------------------------------------------------------------------------------------------------- */
#define COGDL_HIP_KG_DOT 0
#define COGDL_HIP_KG_L1 1
#define COGDL_HIP_KG_CL2 2
COGDL_API size_t cogdl_hip_kg_rank_workspace_bytes(int64_t M, int64_t N, int64_t D, int kind);
COGDL_API int64_t cogdl_hip_kg_rank_slice_entities(int64_t M, int64_t N, int64_t D, int kind);
COGDL_API int cogdl_hip_kg_rank(const float *q, const float *table, const int32_t *target, int64_t M, int64_t N, int64_t D,
                      int kind, float gamma, const int32_t *filt_ptr, const int32_t *filt_idx, int64_t filt_len,
                      int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Sampled triple scoring for knowledge-graph embedding training (added within ABI v9: new symbols only; csrc/kgscore.hip).
 * For each of B prepared query rows q[b] (fp32 [B, D]) and the K table rows idx[b, :] names (int32 [B, K]; table fp32 [N, D]):
 *     scores[b, j] = s(q[b], table[idx[b, j]])                                  fp32 [B, K]      cogdl_hip_kg_score
 *     grad_q[b, k] = SUM_j g[b, j] * ds/dq_k                                    fp32 [B, D]      cogdl_hip_kg_score_grad_q
 *     grad_table[e, k] = SUM_{(b, j): idx[b, j] == e} g[b, j] * ds/dt_k         fp32 [N, D]      cogdl_hip_kg_score_grad_table
 * with kind and gamma as for cogdl_hip_kg_rank (COGDL_HIP_KG_DOT / _L1 / _CL2).  Nothing of size [B, K, D] exists.  The order
 * of every float32 operation is csrc/kgscore_law.h's (a score is a pure function of its two rows: 64 slot partials and a
 * fixed butterfly -- not kg_rank's sequential order, the two never compare scores); there are no float atomics, so all three
 * results are equal from run to run and equal, bit for bit, to the host twins' (cogdl_host_kg_score*).
 * g fp32 [B, K] is the gradient that arrives for scores.  occ_ptr int32 [N + 1], occ_pos int32 [B K]: the inverted index of
 * idx -- occ_pos[occ_ptr[e] .. occ_ptr[e + 1]) are the flat positions b K + j at which e occurs, ascending; ids outside
 * [0, N) are in no list (occ_ptr[0] need not be 0).  grad_table writes EVERY row, zeros included: no memset precedes it.
 * An idx entry outside [0, N) scores NaN and contributes to no gradient; malformed idx / occ_ptr / occ_pos give wrong numbers,
 * never an access outside the operands.
 * Launches on `stream`; no workspace, no allocation, no synchronisation, no host read.  Checked in this order by all three:
 * an unknown kind, odd D with CL2 or a negative size: COGDL_HIP_EINVAL, sizes (B K included) of 2^31 - 1 and more:
 * COGDL_HIP_ERANGE; an empty output (score: B or K of 0; grad_q: B or D of 0; grad_table: N or D of 0): success, nothing
 * launched; a NULL pointer to a non-empty operand: COGDL_HIP_EINVAL; pointers aligned to 4 bytes (COGDL_HIP_EALIGN otherwise;
 * 16-byte loads are used where base addresses and D allow, the bits are the same either way); D above 16384:
 * COGDL_HIP_ERANGE.  Not for use under stream capture.
 * ------------------------------------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_kg_score(const float *q, const float *table, const int32_t *idx, int64_t B, int64_t K, int64_t N,
                       int64_t D, int kind, float gamma, float *scores, void *stream);
COGDL_API int cogdl_hip_kg_score_grad_q(const float *q, const float *table, const int32_t *idx, const float *g, int64_t B,
                       int64_t K, int64_t N, int64_t D, int kind, float *grad_q, void *stream);
COGDL_API int cogdl_hip_kg_score_grad_table(const float *q, const float *table, const float *g, const int32_t *occ_ptr,
                       const int32_t *occ_pos, int64_t B, int64_t K, int64_t N, int64_t D, int kind, float *grad_table,
                       void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Weisfeiler-Lehman subtree relabelling on a batch of graphs (added within ABI v9: new symbols only; csrc/wl.hip): the
 * refinement of Graph2Vec.wl_iterations (cogdl/models/emb/graph2vec.py:63-78) as integers.  The law is csrc/wl_law.h; the
 * host twin is cogdl_host_wl_labels and returns the same bytes.
 *   indptr, indices   int32 CSR [N + 1] / [E] of the disjoint union of the graphs, taken as given (multiplicity counts, a
 *                self-loop is a neighbour).  N <= 2^30, E < 2^31.
 *   label0       int64 [N], arbitrary values.
 *   labels       int32 [rounds + 1, N]: labels[r][v] = the number of classes of round r whose first node precedes the first
 *                node of v's class.  classes int64 [rounds + 1]: the number of classes per round.
 *   hash_bits    1..128: the per-node hash is cut to that many bits before it is used (128: the whole hash).  A test hook:
 *                the result is exact either way, because every node is verified against its representative.  salt: any.
 *   *flags       device int, zeroed by the call: 1 a malformed indptr, 2 an index outside [0, N), 4 a row of more than
 *                cogdl_hip_wl_max_degree() = 32768 neighbours (these three: nothing is computed), 8 two different signatures
 *                with one hash, 16 the probe bound of the table.  Non-zero marks an invalid result; nothing is read out of
 *                bounds and every device loop is bounded.
 *   Enqueues on `stream`, allocates nothing, does not synchronise; ws: cogdl_hip_wl_workspace_bytes(N, E) bytes, 16-byte
 *   aligned.  Not for use under stream capture.
 * ------------------------------------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_wl_max_degree(void);
COGDL_API size_t cogdl_hip_wl_workspace_bytes(int64_t N, int64_t E);
COGDL_API int cogdl_hip_wl_labels(const int32_t *indptr, const int32_t *indices, const int64_t *label0, int64_t N, int64_t E,
                       int64_t rounds, int hash_bits, uint64_t salt, int32_t *labels, int64_t *classes, int *flags, void *ws,
                       size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * PV-DBOW training over ragged documents (added within ABI v9: new symbols only; csrc/pvdbow.hip): the trainer behind gensim's
 * Doc2Vec(dm=0, negative=K) as cogdl/models/emb/graph2vec.py:99-109 calls it.  The law is csrc/pvdbow_law.h on top of
 * csrc/sgns_law.h.  Host twins: cogdl_host_pvdbow_init / cogdl_host_pvdbow_train.
 *   doc_ptr      int64 [G + 1], non-decreasing, within [0, T]: document g owns words[doc_ptr[g] .. doc_ptr[g + 1]).
 *   words        int64 [T], ids in [0, V); a negative id is padding.  No cap on a document's length below 2^32.
 *   D, negative  1..512, 1..16.  epochs >= 1.  keep, cum, exp_table, alpha, min_alpha as for cogdl_hip_sgns_train; the
 *                learning rate falls over epochs * G documents.
 *   dv           float [G, D], syn1 float [V, D], read and updated in place (cogdl_hip_pvdbow_init fills dv from the seed
 *                and zeroes syn1).
 *   workers      1: one launch of one wave, documents in order; equals the host twin bit for bit.  Anything else: launches
 *                of at most docs_in_flight documents (0 = the library's default, 8192) in document order, one wave per
 *                document; syn1 is updated without locks, a dv row has one writer.
 *   *flags       device int, zeroed by the call, then set by a validation pass that runs before any update: 1 an id >= V,
 *                2 a cum that runs backwards or ends in 0, 4 a doc_ptr below 0, running backwards or past T.  Non-zero: the
 *                tables were not touched.  Nothing is read out of bounds.
 *   Stream-ordered, allocates nothing, does not synchronise.  Tuning key 17 selects the row update as for sgns.
 * ------------------------------------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_pvdbow_init(float *dv, int64_t G, float *syn1, int64_t V, int D, uint64_t seed, void *stream);
COGDL_API int cogdl_hip_pvdbow_train(const int64_t *doc_ptr, int64_t G, const int64_t *words, int64_t T, int64_t V, int D,
                       int negative, int64_t epochs, double alpha, double min_alpha, const uint32_t *keep,
                       const uint32_t *cum, const float *exp_table, uint64_t seed, int workers, int64_t docs_in_flight,
                       float *dv, float *syn1, int *flags, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * One training batch of a knowledge-graph embedding model (added within ABI v9: new symbols only; csrc/kgsample.hip): for
 * each of the B positives `order` names, the triple, its subsampling weight and K negatives drawn uniformly, with
 * repetition, from the entities that are not in the positive's true list -- the batch TrainDataset.__getitem__ and collate_fn
 * make on the host (cogdl/datasets/kg_data.py:98-135).  The law is csrc/kgsample_law.h: negative j of the positive with
 * ordinal sid = first_sid + b (modulo 2^64) is a pure function of (seed, tag, sid, j) and the list; no rejection loop.  The
 * host twin is cogdl_host_kg_train_batch and returns the same bytes.
 *   triples      int32 [T, 3] (head, relation, tail); weight_tab float [T]; group int32 [T]: the list of each triple.
 *   list_ptr     int32 [G + 1], list_idx int32 [list_len]: list g is list_idx[list_ptr[g] .. list_ptr[g + 1]), ids in [0, N)
 *                ascending and distinct (the true heads of a (relation, tail) for a head-batch, the true tails of a
 *                (head, relation) for a tail-batch).
 *   order        int32 [B]: the triple ids of this batch.  tag: COGDL_HIP_KG_TAG_HEAD or _TAIL (any word is accepted: it
 *                only separates streams).
 *   positive     int64 [B, 3]; negative [B, K], int64 where index64 is non-zero and int32 otherwise; weight float [B].
 *   *status      device int, zeroed by the call: 1 an order id outside [0, T), 2 a list that leaves no entity free, 4 a group
 *                id or list bounds outside the tables.  The row concerned is written as -1 (weight 0) and nothing is indexed
 *                with the offending value; every other row is unaffected.  A list that is not ascending and distinct gives
 *                wrong numbers, never an access outside the operands.
 * Launches on `stream`; no workspace, no allocation, no synchronisation, no host read.  A negative size: COGDL_HIP_EINVAL;
 * sizes of 2^31 - 1 and more: COGDL_HIP_ERANGE; B == 0: the status is zeroed, nothing else is launched; a NULL pointer to a
 * non-empty operand: COGDL_HIP_EINVAL; pointers aligned to their element size (COGDL_HIP_EALIGN otherwise).
 * ------------------------------------------------------------------------------------------------------------------- */
#define COGDL_HIP_KG_TAG_HEAD 0x4B474E48u
#define COGDL_HIP_KG_TAG_TAIL 0x4B474E54u
COGDL_API int cogdl_hip_kg_train_batch(const int32_t *triples, const float *weight_tab, const int32_t *group,
                       const int32_t *list_ptr, const int32_t *list_idx, int64_t T, int64_t G, int64_t list_len,
                       const int32_t *order, int64_t B, int64_t K, int64_t N, uint64_t seed, uint32_t tag, uint64_t first_sid,
                       int index64, int64_t *positive, void *negative, float *weight, int *status, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Edge-sampled skip-gram training with negative sampling (added within ABI v9: a new symbol only; csrc/line.hip): the
 * trainer of the LINE model, orders 1 and 2 (cogdl/models/emb/line.py), on an edge table that is already on the device.  The
 * law -- draws, order of updates, every rounding -- is csrc/line_law.h on top of csrc/sgns_law.h.  Host twin:
 * cogdl_host_line_train.  cogdl_hip_sgns_init serves initialisation (emb from the seed, ctx = 0).
 *   eu, ev       int64 [M], M >= 1: the endpoints of the undirected edges, ids in [0, V).  A sample draws an edge in
 *                proportion to its weight and orients it by a fair coin.
 *   ecum         NULL (unit weights), or int64 [M]: cumulative weights, non-decreasing, first entry >= 0, last entry in
 *                [1, 2^52] (callers build 2^52).  An edge of weight 0 is never drawn.
 *   ncum         uint32 [V]: cumulative node noise table, non-decreasing, last entry >= 1 (callers build 2^31 - 1).
 *   exp_table    float [1000], as for cogdl_hip_sgns_train.
 *   D, negative  1..512, 1..16.  order 1: targets are rows of emb, ctx is not used (may be NULL).  order 2: rows of ctx.
 *   S            >= 0 samples; sample s runs at the learning rate alpha * max(1 - s / S, 1e-4).  alpha > 0.
 *   emb, ctx     float [V, D] row-major, read and updated in place.
 *   workers      1: one launch of one wave, samples in order; the result equals the host twin's bit for bit.  Slow by
 *                construction.  Anything else: launches of at most samples_in_flight consecutive samples (0 = the library's
 *                default) in sample order; the samples of one launch run concurrently and update the tables without locks
 *                (no-return float atomics: no add is lost), so results differ from run to run.
 *   *flags       device int, zeroed by the call, then set by a validation pass that runs before any update: 1 an endpoint
 *                outside [0, V), 2 a malformed ncum, 4 a malformed ecum.  Non-zero: the tables were not touched.  Nothing is
 *                read out of bounds.
 *   Stream-ordered, allocates nothing, does not synchronise.
 * ------------------------------------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_line_train(const int64_t *eu, const int64_t *ev, const int64_t *ecum, int64_t M, int64_t V,
                       const uint32_t *ncum, const float *exp_table, int D, int negative, int order, int64_t S, double alpha,
                       uint64_t seed, int workers, int64_t samples_in_flight, float *emb, float *ctx, int *flags,
                       void *stream);

/* -------------------------------------------------------------------------------------------------------------------
 * Fused multiplex (typed-edge) attention embedding: GATNE's model step (csrc/multiplex.hip).  For sample b with
 * x = inputs[b], t = types[b]:
 *     c[i, :] = SUM_s type_emb[neigh[x, i, s], i, :]        h = tanh(c att_w1[t])        e = h att_w2[t]
 *     att = softmax_i(e)        m = att c        y = node_emb[x] + m trans_w[t]        out[b] = y / max(||y||, 1e-12)
 * node_emb fp32 [N, D], type_emb fp32 [N, T, U], trans_w fp32 [T, U, D], att_w1 fp32 [T, U, A], att_w2 fp32 [T, A],
 * neigh int32 [N, T, S], inputs / types int32 [B].  Nothing of size [B, T, S, U] is written.  The order of every float32
 * operation is csrc/multiplex_law.h's; there are no float atomics: results are equal from run to run and do not depend on the
 * launch geometry.  tanh and exp are the device library's (no host twin).
 *   cogdl_hip_multiplex_fwd         one launch, one wave per sample.  Writes out [B, D] and what the backward reads: c [B, T, U],
 *                                   h [B, T, A], att [B, T], m [B, U], nrm [B].  A sample whose input, type or any of its T S
 *                                   neighbour ids is out of range gets out = NaN and nrm = -1; no id is followed unchecked.
 *   cogdl_hip_multiplex_bwd_sample  g fp32 [B, D] -> g_y [B, D], g_c [B, T, U], g_pre [B, T, A], g_e [B, T]; zeros for a sample
 *                                   with nrm < 0.
 *   cogdl_hip_multiplex_bwd_weights grad trans_w, grad att_w1, grad att_w2 (each may be NULL: not computed) from the lists of
 *                                   the samples of each type.
 *   cogdl_hip_multiplex_bwd_node    grad node_emb [N, D] from the lists of the samples of each input node.
 *   cogdl_hip_multiplex_bwd_type    grad type_emb [N, T, U] from the lists of the neighbour slots of each key n T + i.
 * Lists: occ_ptr int32 points at the first bound of the family (T + 1, N + 1, N T + 1 bounds are read), occ_pos int32 [P] is
 * the whole position array of the inverted index; a list entry is pos_base + b (weights, node) or pos_base + (b T + i) S + s
 * (type), ascending.  Entries outside their range are passed over, bounds are clamped to [0, P]; every element of every
 * gradient is written, +0 for an empty list: no memset precedes the launches.
 * Limits: 1 <= T <= 16, 1 <= S, U, A <= 64, 1 <= D <= 1024, B T S + 2 B and N T + N + T below 2^31 - 1 (COGDL_HIP_ERANGE
 * beyond); a negative or zero T, S, U, A, D: COGDL_HIP_EINVAL; B == 0 (N == 0 for the two table gradients): success, nothing
 * launched; a NULL pointer to a non-empty operand: COGDL_HIP_EINVAL; pointers aligned to 4 bytes (COGDL_HIP_EALIGN otherwise).
 * ------------------------------------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_multiplex_fwd(const float *node_emb, const float *type_emb, const float *trans_w, const float *att_w1,
                       const float *att_w2, const int32_t *neigh, const int32_t *inputs, const int32_t *types, int64_t B,
                       int64_t N, int64_t T, int64_t S, int64_t U, int64_t A, int64_t D, float *c, float *h, float *att, float *m,
                       float *nrm, float *out, void *stream);
COGDL_API int cogdl_hip_multiplex_bwd_sample(const float *trans_w, const float *att_w1, const float *att_w2, const int32_t *types,
                       const float *g, const float *out, const float *nrm, const float *c, const float *h, const float *att,
                       int64_t B, int64_t T, int64_t U, int64_t A, int64_t D, float *g_y, float *g_c, float *g_pre, float *g_e,
                       void *stream);
COGDL_API int cogdl_hip_multiplex_bwd_weights(const float *m, const float *g_y, const float *c, const float *g_pre,
                       const float *g_e, const float *h, const int32_t *occ_ptr, const int32_t *occ_pos, int64_t pos_base,
                       int64_t P, int64_t B, int64_t T, int64_t U, int64_t A, int64_t D, float *g_trans, float *g_w1, float *g_w2,
                       void *stream);
COGDL_API int cogdl_hip_multiplex_bwd_node(const float *g_y, const int32_t *occ_ptr, const int32_t *occ_pos, int64_t pos_base,
                       int64_t P, int64_t B, int64_t N, int64_t D, float *g_node, void *stream);
COGDL_API int cogdl_hip_multiplex_bwd_type(const float *g_c, const int32_t *occ_ptr, const int32_t *occ_pos, int64_t pos_base,
                       int64_t P, int64_t B, int64_t N, int64_t T, int64_t S, int64_t U, float *g_type, void *stream);

/* -------------------------------------------------------------------------------------------------------------------
 * Activation compression (added within ABI v9: new symbols only; csrc/actq.hip): what a layer saves for its backward pass,
 * held in 1 / 2 / 4 / 8 bits per element, one bit per element, or not at all.  The law -- groups of the flattened tensor,
 * bounds, Philox draws, stochastic rounding, packing, what a NaN / an infinity / an overflowing range does, the error bound
 * -- is csrc/actq_law.h; the host twins (cogdl_host_<same name>, include/cogdl_host.h) return the same bytes.
 *   cogdl_hip_actq_quantize    x fp32 [n] -> codes uint32 [ceil(n bits / 32)], meta fp32 [2 ceil(n / group)] ((mn, step) per
 *                              group).  bits in {1, 2, 4, 8}, group in {64, 128, 256}; (seed, call) select the draws.
 *   cogdl_hip_actq_dequantize  out[i] = mn + code * step, fp32 [n].
 *   cogdl_hip_relu_mask        y = relu(x) (NaN kept), mask uint64 [ceil(n / 64)]: bit i % 64 of word i / 64 is x[i] > 0.
 *   cogdl_hip_mask_apply       out[i] = bit i ? g[i] : 0.
 *   cogdl_hip_drop_apply       y[i] = keep(seed, call, i) ? x[i] * scale : 0 with thresh in [0, 65536] (drop_params of
 *                              csrc/philox.h); forward and backward are this one function.
 * n == 0: success, nothing launched; n < 0, n >= 2^59, other bits / group / thresh, a NULL operand: COGDL_HIP_EINVAL.  fp32
 * operands at any 4-byte boundary (16-byte aligned ones take 16-byte lanes, same results), meta and mask 8-byte aligned
 * (COGDL_HIP_EALIGN otherwise).  Input and output must not overlap.  Stream-ordered, allocate nothing, do not synchronise; no
 * atomics: results are equal from run to run and do not depend on the launch geometry.
 * ------------------------------------------------------------------------------------------------------------------- */
COGDL_API int cogdl_hip_actq_quantize(const float *x, int64_t n, int bits, int group, uint64_t seed, uint64_t call,
                       uint32_t *codes, float *meta, void *stream);
COGDL_API int cogdl_hip_actq_dequantize(const uint32_t *codes, const float *meta, int64_t n, int bits, int group, float *out,
                       void *stream);
COGDL_API int cogdl_hip_relu_mask(const float *x, int64_t n, float *y, uint64_t *mask, void *stream);
COGDL_API int cogdl_hip_mask_apply(const float *g, const uint64_t *mask, int64_t n, float *out, void *stream);
COGDL_API int cogdl_hip_drop_apply(const float *x, int64_t n, uint64_t seed, uint64_t call, uint32_t thresh, float scale,
                       float *y, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* COGDL_HIP_H */
