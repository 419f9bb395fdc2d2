/* arrow_spmm — C ABI of the MI355X-native arrow-SpMM compute library.
 *
 * This is the drop-in boundary of the rebuilt hot path of spcl/arrow-matrix:
 * the reference does its per-block compute through cupy's cuSPARSE CSRMM
 * binding (`A @ X` on cp.sparse.csr_matrix, arrow_slim_mpi.py:190,211,231)
 * and its permutation routing through host fancy-indexing
 * (arrow_dec_mpi.py:421,437,526,544). Each exported entry point below
 * replaces one of those interfaces:
 *
 *   arrow_csr_create / arrow_csr_destroy
 *       replaces arrow/common/sp2cp.py:6-16 (_sp2cp host->device CSR
 *       conversion, re-done every call in the reference,
 *       arrow_slim_mpi.py:184,210,226) — here the block is uploaded ONCE
 *       and stays resident in HBM.
 *   arrow_spmm
 *       replaces the cupy `A @ X` CSRMM (arrow_slim_mpi.py:190,211,231):
 *       C (+)= A @ X for one resident CSR block, X/C row-major fp32 device
 *       buffers, X (cols,k), C (rows,k).
 *   arrow_gather_rows_f32
 *       replaces the host gathers sendbuf = T[perm]
 *       (arrow_dec_mpi.py:421,526) — payload stays in HBM.
 *   arrow_scatter_rows_f32 / arrow_scatter_add_rows_f32
 *       replace C_i[perm] = recvbuf (arrow_dec_mpi.py:544) and
 *       C_i[perm] += recvbuf (arrow_dec_mpi.py:437).
 *
 * Conventions: device pointers are HIP device memory owned by the caller
 * (e.g. torch tensors' data_ptr); host pointers are read during the call
 * only. `stream` is a hipStream_t (or NULL for the default stream). All
 * functions return 0 on success, negative on error (arrow_last_error()
 * gives the message). One process per GPU; not thread-safe.
 */
#ifndef ARROW_SPMM_H
#define ARROW_SPMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library/device introspection */
int arrow_device_count(void);
int arrow_set_device(int device);
const char *arrow_last_error(void);
int arrow_synchronize(void);
/* ABI version (major*1000 + minor) */
int arrow_abi_version(void);

/* Upload a CSR block (host arrays) once; returns a handle >= 0, < 0 on
 * error. indptr has rows+1 int64 entries; indices int32; data fp32.
 * Builds the row-segment work list for the SpMM kernel at upload time.
 *
 * Limits of one structure, for every arrow_csr_create* entry point: nnz,
 * rows, cols (hence every column index, of either sign) and every output row
 * id of row_ids fit int32, and a row id is not negative; anything else is
 * refused with -1 before anything is allocated, and the message names the
 * limit and the offending value (e.g. "arrow_csr_create: row id 2147483648
 * at row 7 exceeds int32"). Element and byte offsets into X, C, R and D
 * (row * k + column) are 64-bit everywhere, so rows * k and cols * k may
 * pass 2^31 elements and 4 GiB. */
int64_t arrow_csr_create(int64_t rows, int64_t cols, int64_t nnz,
                         const int64_t *indptr, const int32_t *indices,
                         const float *data);
/* As arrow_csr_create_rows plus option flags. flags bit 0: order work
 * items by first column instead of row — for hub-heavy structures whose
 * long rows split into column-contiguous items, a queue segment then
 * covers a COLUMN window of X (locality for the per-XCD scheduler).
 * row_ids may be NULL. */
int64_t arrow_csr_create_opts(int64_t rows, int64_t cols, int64_t nnz,
                              const int64_t *indptr, const int32_t *indices,
                              const float *data, const int64_t *row_ids,
                              int flags);
/* As arrow_csr_create, but structure row r writes output row row_ids[r]
 * (reordered layouts, e.g. hub-sorted first-block-column entries). */
int64_t arrow_csr_create_rows(int64_t rows, int64_t cols, int64_t nnz,
                              const int64_t *indptr, const int32_t *indices,
                              const float *data, const int64_t *row_ids);
int arrow_csr_destroy(int64_t handle);
/* nnz of a resident block (for flop accounting) */
int64_t arrow_csr_nnz(int64_t handle);
/* Enable the XCD-contiguous work remap for this structure (a performance
 * hint for uniform banded rows; off by default). */
int arrow_csr_set_xcd_remap(int64_t handle, int enable);
/* Per-XCD queue scheduler for this structure: workgroups drain contiguous
 * nnz-balanced row segments via per-XCD atomic chunk counters (keeps the
 * consumers of each X row in ONE XCD's L2). mode: 1 on, 0 off,
 * -1 follow the ARROW_QUEUE env default. */
int arrow_csr_set_queue(int64_t handle, int mode);
/* Per-structure launch-grid override for the queue scheduler (workgroup
 * count; 0 = the ARROW_Q_BLOCKS env default). Used to co-schedule two
 * concurrent structure launches on separate HIP streams so neither grid
 * fills the whole chip. */
int arrow_csr_set_qblocks(int64_t handle, int blocks);

/* C (+)= A @ X.  X: (cols, k) fp32 row-major device;  C: (rows, k).
 * beta = 0: C = A@X (rows not touched by A are zeroed);  beta = 1: C += A@X. */
int arrow_spmm(int64_t handle, const float *X_dev, float *C_dev, int64_t k,
               int beta, void *stream);

/* Dual-operand SpMM for the FUSED diagonal + first-block-column layout
 * (replaces the reference's back-to-back C_i = A_ii@X_i; C_i += A_i0@X_0,
 * arrow_slim_mpi.py:121-144, writing C once instead of read-modify-write):
 * a column index c >= 0 reads X0[c]; c < 0 reads X1[-c-1]. The negative
 * encoding is fixed at arrow_csr_create time by the caller's indices. */
int arrow_spmm_dual(int64_t handle, const float *X0_dev, const float *X1_dev,
                    float *C_dev, int64_t k, int beta, void *stream);

/* Launch-plan query: the decision arrow_spmm / arrow_spmm_dual take for a
 * structure with `nnz` nonzeros at feature width k. Needs no handle and no
 * device; the launcher itself consumes the same plan. queue_mode is the
 * structure's arrow_csr_set_queue mode (1 on, 0 off, -1 follow ARROW_QUEUE).
 * Writes min(n_out, ARROW_PLAN_FIELDS) int32 fields to out, in the order of
 * the ARROW_PLAN_* indices below, and returns ARROW_PLAN_FIELDS (negative
 * on error).
 *
 * The kernel-tuning environment variables (ARROW_SPMM_G64, ARROW_K16_G8,
 * ARROW_SPMM_NT, ARROW_QUEUE, ARROW_QWAVE, ARROW_Q_MIN_NNZ, ARROW_Q_CHUNK,
 * ARROW_Q_BLOCKS, ARROW_QW_CHUNK) are read ONCE per process, on the first
 * arrow_spmm, arrow_spmm_dual or arrow_spmm_plan call. Setting one later in
 * the same process changes nothing: choose a variant before first use, in
 * a fresh process. */
#define ARROW_PLAN_VEC 0         /* floats per lane: 1, 2 or 4 */
#define ARROW_PLAN_GROUP 1       /* lanes per work item: 1..64 */
#define ARROW_PLAN_SCHEDULER 2   /* 0 grid-stride, 1 block-grab queue,
                                    2 wave-grab queue */
#define ARROW_PLAN_NT_MODE 3     /* 1 non-temporal A loads / C stores */
#define ARROW_PLAN_CHUNK_ITEMS 4 /* items per queue grab as launched
                                    (0 for grid-stride) */
#define ARROW_PLAN_GRID_CAP 5    /* workgroup cap of the chosen scheduler:
                                    the queue grid (ARROW_Q_BLOCKS, before
                                    any arrow_csr_set_qblocks override) or
                                    the grid-stride cap */
#define ARROW_PLAN_LAUNCHES 6    /* column-offset launches, ceil(k/(group*vec)) */
#define ARROW_PLAN_FIELDS 7
int arrow_spmm_plan(int64_t k, int64_t nnz, int queue_mode, int32_t *out,
                    int n_out);

/* dst[i, :] = src[idx[i], :]   (n rows of width k, fp32, device) */
int arrow_gather_rows_f32(const float *src_dev, float *dst_dev,
                          const int64_t *idx_dev, int64_t n, int64_t k,
                          void *stream);
/* dst[idx[i], :] = src[i, :] */
int arrow_scatter_rows_f32(float *dst_dev, const float *src_dev,
                           const int64_t *idx_dev, int64_t n, int64_t k,
                           void *stream);
/* dst[idx[i], :] += src[i, :] */
int arrow_scatter_add_rows_f32(float *dst_dev, const float *src_dev,
                               const int64_t *idx_dev, int64_t n, int64_t k,
                               void *stream);

/* Fused gather+scatter for the rank-local share of the permutation routing
 * (arrow_dec_mpi.py:526+544 / 421+437 collapsed into one pass):
 * dst[dst_idx[i], :] (+)= src[src_idx[i], :] */
int arrow_permute_rows_f32(float *dst_dev, const float *src_dev,
                           const int64_t *dst_idx_dev, const int64_t *src_idx_dev,
                           int64_t n, int64_t k, void *stream);
int arrow_permute_add_rows_f32(float *dst_dev, const float *src_dev,
                               const int64_t *dst_idx_dev, const int64_t *src_idx_dev,
                               int64_t n, int64_t k, void *stream);

/* ---------------------------------------------------------------------
 * float64 (ABI 1003). The reference's precision knob — `datatype=` on
 * bench_spmm / load_decomposition_new (arrow_bench.py:21,
 * arrow_dec_mpi.py:629), `dtype=` on zero_rhs (arrow_slim_mpi.py:354),
 * `-t float64` on the PETSc and 1.5D CLIs — runs on the GPU there through
 * cupy's float64 CSRMM; these exports replace that.
 *
 * A structure's precision is fixed when it is created. Raw device pointers
 * carry no type, so the handle's tag is the only guard: a handle passed to
 * the other precision's SpMM entry point returns a negative code, sets an
 * arrow_last_error() message naming both precisions, and launches nothing.
 * ------------------------------------------------------------------- */

/* Upload a CSR block with float64 values (replaces sp2cp.py:6-16 for a
 * float64 csr_matrix). Same arguments as arrow_csr_create_opts; row_ids may
 * be NULL. Resident layout: split int32 cols[] + double vals[], 12 B/nnz. */
int64_t arrow_csr_create_f64(int64_t rows, int64_t cols, int64_t nnz,
                             const int64_t *indptr, const int32_t *indices,
                             const double *data, const int64_t *row_ids,
                             int flags);
/* Precision of a resident block: 32 or 64 (negative on a bad handle). */
int arrow_csr_dtype(int64_t handle);

/* C (+)= A @ X in float64 (replaces the cupy `A @ X` CSRMM,
 * arrow_slim_mpi.py:190,211,231, at dtype float64). X: (cols, k) float64
 * row-major device; C: (rows, k). X and C rows must be 16-byte aligned when
 * k is even (any torch allocation is). Accumulates in double with fma;
 * split hub rows add with the hardware float64 global atomic. */
int arrow_spmm_f64(int64_t handle, const double *X_dev, double *C_dev,
                   int64_t k, int beta, void *stream);
/* Dual-operand form, as arrow_spmm_dual (arrow_slim_mpi.py:121-144). */
int arrow_spmm_dual_f64(int64_t handle, const double *X0_dev,
                        const double *X1_dev, double *C_dev, int64_t k,
                        int beta, void *stream);

/* Launch-plan query for the float64 entry points: the same seven fields as
 * arrow_spmm_plan, from the same policy and the same once-per-process
 * environment. ARROW_PLAN_VEC counts doubles per lane: 2 when k is even
 * (16 bytes, as the fp32 float4), else 1; GROUP = the power of two >=
 * ceil(k / vec), capped at 64. The queue policy (GROUP >= 4 and nnz >=
 * ARROW_Q_MIN_NNZ), wave grabs at GROUP < 8 and the chunk and grid
 * variables apply unchanged: a lane is 16 bytes in both precisions, so the
 * GROUP-based thresholds carry over by row bytes — but they were MEASURED
 * FOR FP32 ONLY. ARROW_SPMM_G64 and ARROW_K16_G8 are fp32 layout
 * experiments and are ignored by the float64 plan. */
int arrow_spmm_plan_f64(int64_t k, int64_t nnz, int queue_mode, int32_t *out,
                        int n_out);

/* float64 routing (replace the host fancy-indexing of arrow_dec_mpi.py at
 * dtype float64): gather :421,526; scatter :544; scatter-add :437; the
 * fused rank-local permute :526+544 and permute-add :421+437. */
int arrow_gather_rows_f64(const double *src_dev, double *dst_dev,
                          const int64_t *idx_dev, int64_t n, int64_t k,
                          void *stream);
int arrow_scatter_rows_f64(double *dst_dev, const double *src_dev,
                           const int64_t *idx_dev, int64_t n, int64_t k,
                           void *stream);
int arrow_scatter_add_rows_f64(double *dst_dev, const double *src_dev,
                               const int64_t *idx_dev, int64_t n, int64_t k,
                               void *stream);
int arrow_permute_rows_f64(double *dst_dev, const double *src_dev,
                           const int64_t *dst_idx_dev,
                           const int64_t *src_idx_dev, int64_t n, int64_t k,
                           void *stream);
int arrow_permute_add_rows_f64(double *dst_dev, const double *src_dev,
                               const int64_t *dst_idx_dev,
                               const int64_t *src_idx_dev, int64_t n,
                               int64_t k, void *stream);

/* ---------------------------------------------------------------------
 * bfloat16 features (ABI 1004). Only the STORAGE of the feature matrices X
 * and C changes: they cross the ABI as uint16_t raw bf16 bits, half the
 * bytes of the fp32 rows that dominate the traffic. A stays the resident
 * fp32 (col, val) pairs, every product and every partial sum is fp32
 * (fmaf), and a C element is rounded to bf16 ONCE per call, by a plain
 * cast: round-to-nearest-even, NaN stays NaN. The reference has no bf16
 * mode; these exports stand in for the same cupy `A @ X` CSRMM and host
 * fancy-indexing as the fp32 ones, for a caller that keeps features in
 * bf16 and would otherwise upcast.
 *
 * There is no create call: the bf16 entry points take a float32 structure
 * handle (arrow_csr_create, _rows, _opts), so one resident copy of A serves
 * fp32 and bf16 features alike and arrow_csr_dtype keeps reporting 32. A
 * float64 handle is refused like any precision mismatch: negative code, a
 * message naming both, nothing launched.
 *
 * k must be a multiple of 8 (a lane moves 8 bf16 = 16 bytes; X and C rows
 * are then 16-byte aligned, given 16-byte aligned base pointers). Any other
 * k returns a negative code with a message naming the rule, and launches
 * nothing. k > 512 is column-tiled over launches.
 *
 * Split hub rows (more than 2048 nonzeros) are NOT summed in bf16: their
 * items add fp32 partials into a per-structure fp32 scratch of
 * n_split_rows x k floats, and a small finalise kernel writes
 * C[row] = bf16((beta ? float(C[row]) : 0) + sum) and re-zeroes the
 * scratch. The scratch is allocated on the first bf16 call that needs it
 * and grows when a wider k comes (hipMalloc): that first call must not be
 * under stream capture. RUN ONE WARM-UP CALL AT THE WIDEST k BEFORE ANY
 * CAPTURE. Two bf16 calls on one structure must not overlap in time.
 * ------------------------------------------------------------------- */

/* C (+)= A @ X with bf16 X and C (replaces the cupy `A @ X` CSRMM,
 * arrow_slim_mpi.py:190,211,231). beta = 1 computes
 * bf16(float(C_old) + A@X). */
int arrow_spmm_bf16(int64_t handle, const uint16_t *X_dev, uint16_t *C_dev,
                    int64_t k, int beta, void *stream);
/* Dual-operand form, as arrow_spmm_dual (arrow_slim_mpi.py:121-144). */
int arrow_spmm_dual_bf16(int64_t handle, const uint16_t *X0_dev,
                         const uint16_t *X1_dev, uint16_t *C_dev, int64_t k,
                         int beta, void *stream);

/* Launch-plan query for the bf16 entry points: the same seven fields as
 * arrow_spmm_plan, from the same policy and the same once-per-process
 * environment; needs no device. ARROW_PLAN_VEC reads 8 (bf16 per lane);
 * GROUP = the power of two >= k / 8, capped at 64. k % 8 != 0 returns a
 * negative code. The queue policy, wave grabs at GROUP < 8 and the chunk
 * and grid variables apply unchanged: a lane is still 16 bytes, so the
 * GROUP-based thresholds carry over by row bytes — but they were MEASURED
 * FOR FP32 ONLY. ARROW_SPMM_G64 and ARROW_K16_G8 are ignored. */
int arrow_spmm_plan_bf16(int64_t k, int64_t nnz, int queue_mode, int32_t *out,
                         int n_out);

/* bf16 routing (replace the host fancy-indexing of arrow_dec_mpi.py for
 * bf16 rows, k % 8 == 0): gather :421,526; scatter :544; the fused
 * rank-local permute :526+544 — pure copies, bit-exact. scatter-add :437
 * and permute-add :421+437 compute bf16(float(dst) + float(src)), one
 * rounding per element. */
int arrow_gather_rows_bf16(const uint16_t *src_dev, uint16_t *dst_dev,
                           const int64_t *idx_dev, int64_t n, int64_t k,
                           void *stream);
int arrow_scatter_rows_bf16(uint16_t *dst_dev, const uint16_t *src_dev,
                            const int64_t *idx_dev, int64_t n, int64_t k,
                            void *stream);
int arrow_scatter_add_rows_bf16(uint16_t *dst_dev, const uint16_t *src_dev,
                                const int64_t *idx_dev, int64_t n, int64_t k,
                                void *stream);
int arrow_permute_rows_bf16(uint16_t *dst_dev, const uint16_t *src_dev,
                            const int64_t *dst_idx_dev,
                            const int64_t *src_idx_dev, int64_t n, int64_t k,
                            void *stream);
int arrow_permute_add_rows_bf16(uint16_t *dst_dev, const uint16_t *src_dev,
                                const int64_t *dst_idx_dev,
                                const int64_t *src_idx_dev, int64_t n,
                                int64_t k, void *stream);

/* ---------------------------------------------------------------------
 * Affine step (ABI 1005). The workloads that iterate an SpMM (PageRank,
 * APPNP / label propagation, damped diffusion, Chebyshev filters) want
 *
 *     C[row] = alpha * (A @ X)[row] + gamma * R[row] + beta * C[row]
 *
 * for every output row the structure writes, with beta 0 or 1. The
 * reference has no such call (its callers run an elementwise pass after
 * `A @ X`); here the step is fused into the write-back of the SAME launches
 * the plain entry points make: one extra read of R, C still written once.
 *
 * R is a row-major matrix of the feature type, shaped like C and indexed by
 * OUTPUT row (after row_ids). Empty rows yield gamma * R[row] (+ C[row]).
 * alpha and gamma are doubles in every precision and are applied in the
 * accumulator type: float for fp32 and bf16 features, double for float64.
 * bf16: one rounding per element, split rows included (their finalise pass
 * computes bf16(alpha * sum + gamma * float(R) + (beta ? float(C) : 0))).
 * fp32 / f64 split rows: the pre-launch pass writes gamma * R (adds it at
 * beta = 1) and the items add alpha * partial with the hardware atomic.
 *
 * Rules; a broken one returns a negative code, sets arrow_last_error(),
 * launches nothing and leaves C untouched:
 *   - R == NULL is allowed only when gamma == 0; R is then never read;
 *   - R == C is refused (X may alias R);
 *   - beta other than 0 or 1 is refused;
 *   - a handle of the other precision, and bf16 k % 8 != 0, are refused
 *     exactly as on the plain entry points.
 *
 * The launch plan is the plain one: arrow_spmm_plan / _f64 / _bf16 are
 * unchanged and describe an affine launch too. (alpha, gamma, R) =
 * (1, 0, NULL) computes what the plain entry point computes, bit for bit.
 * The bf16 warm-up rule before stream capture applies unchanged.
 * ------------------------------------------------------------------- */
int arrow_spmm_affine(int64_t handle, const float *X_dev, float *C_dev,
                      const float *R_dev, int64_t k, double alpha,
                      double gamma, int beta, void *stream);
int arrow_spmm_dual_affine(int64_t handle, const float *X0_dev,
                           const float *X1_dev, float *C_dev,
                           const float *R_dev, int64_t k, double alpha,
                           double gamma, int beta, void *stream);
int arrow_spmm_affine_f64(int64_t handle, const double *X_dev, double *C_dev,
                          const double *R_dev, int64_t k, double alpha,
                          double gamma, int beta, void *stream);
int arrow_spmm_dual_affine_f64(int64_t handle, const double *X0_dev,
                               const double *X1_dev, double *C_dev,
                               const double *R_dev, int64_t k, double alpha,
                               double gamma, int beta, void *stream);
int arrow_spmm_affine_bf16(int64_t handle, const uint16_t *X_dev,
                           uint16_t *C_dev, const uint16_t *R_dev, int64_t k,
                           double alpha, double gamma, int beta,
                           void *stream);
int arrow_spmm_dual_affine_bf16(int64_t handle, const uint16_t *X0_dev,
                                const uint16_t *X1_dev, uint16_t *C_dev,
                                const uint16_t *R_dev, int64_t k,
                                double alpha, double gamma, int beta,
                                void *stream);

/* The stand-alone tail of the affine step, for results that no single
 * launch finishes: C = alpha * C + gamma * R over n contiguous rows of
 * width k (device, row-major). bf16 (k % 8 == 0) moves 16-byte lanes,
 * computes in fp32 and rounds once. R == NULL only with gamma == 0; R == C
 * is refused; n == 0 is a no-op. */
int arrow_axpby_rows_f32(float *C_dev, const float *R_dev, int64_t n,
                         int64_t k, double alpha, double gamma, void *stream);
int arrow_axpby_rows_f64(double *C_dev, const double *R_dev, int64_t n,
                         int64_t k, double alpha, double gamma, void *stream);
int arrow_axpby_rows_bf16(uint16_t *C_dev, const uint16_t *R_dev, int64_t n,
                          int64_t k, double alpha, double gamma,
                          void *stream);

/* ---------------------------------------------------------------------
 * Step norms (ABI 1006). The workloads of the affine step run until the
 * iterate stops moving, so the same launches can also measure the step:
 *
 *     acc[0] += sum (c - d)^2        acc[1] += sum c^2
 *
 * over every element of every output row the structure writes (after
 * row_ids, empty rows included, columns 0..k-1). c is the value AS STORED in
 * C (bf16: after the single rounding), d the stored value of D[row]. D is a
 * row-major matrix of the feature type, shaped like C and indexed by OUTPUT
 * row exactly as R is; D == NULL means d = 0. c - d is formed in the
 * accumulator type (float for fp32 and bf16 features, double for float64);
 * both squares and all summation are double in every precision.
 *
 * acc points at two doubles in device memory. The call ADDS into them: the
 * caller zeroes them, so several launches can share one pair. Non-split rows
 * are measured in the write-back of the launch that computes them (one more
 * row read, no extra pass); each workgroup reduces its lanes' sums and adds
 * them with one float64 atomic per accumulator. Split hub rows are measured
 * once per call after the last column tile: fp32 / f64 by a small pass over
 * the split-row table, bf16 in the finalise pass that writes them.
 *
 * Rules, in addition to the affine step's (which carry over unchanged); a
 * broken one returns a negative code, sets arrow_last_error(), launches
 * nothing and leaves C and acc untouched:
 *   - beta other than 0 is refused: a launch that does not finish its rows
 *     has no business measuring them;
 *   - acc == NULL is refused;
 *   - D == C is refused. D may alias X or R.
 *
 * C is what the affine entry point writes, bit for bit, in every precision;
 * (alpha, gamma, R) = (1, 0, NULL) writes the plain product bit for bit.
 * The launch plan is the plain one (arrow_spmm_plan / _f64 / _bf16).
 * ------------------------------------------------------------------- */
int arrow_spmm_affine_norm(int64_t handle, const float *X_dev, float *C_dev,
                           const float *R_dev, const float *D_dev,
                           double *acc_dev, int64_t k, double alpha,
                           double gamma, int beta, void *stream);
int arrow_spmm_dual_affine_norm(int64_t handle, const float *X0_dev,
                                const float *X1_dev, float *C_dev,
                                const float *R_dev, const float *D_dev,
                                double *acc_dev, int64_t k, double alpha,
                                double gamma, int beta, void *stream);
int arrow_spmm_affine_norm_f64(int64_t handle, const double *X_dev,
                               double *C_dev, const double *R_dev,
                               const double *D_dev, double *acc_dev,
                               int64_t k, double alpha, double gamma,
                               int beta, void *stream);
int arrow_spmm_dual_affine_norm_f64(int64_t handle, const double *X0_dev,
                                    const double *X1_dev, double *C_dev,
                                    const double *R_dev, const double *D_dev,
                                    double *acc_dev, int64_t k, double alpha,
                                    double gamma, int beta, void *stream);
int arrow_spmm_affine_norm_bf16(int64_t handle, const uint16_t *X_dev,
                                uint16_t *C_dev, const uint16_t *R_dev,
                                const uint16_t *D_dev, double *acc_dev,
                                int64_t k, double alpha, double gamma,
                                int beta, void *stream);
int arrow_spmm_dual_affine_norm_bf16(int64_t handle, const uint16_t *X0_dev,
                                     const uint16_t *X1_dev, uint16_t *C_dev,
                                     const uint16_t *R_dev,
                                     const uint16_t *D_dev, double *acc_dev,
                                     int64_t k, double alpha, double gamma,
                                     int beta, void *stream);

/* The stand-alone form of the measure, for results that no single launch
 * finishes: the same two sums over n contiguous rows of width k (device,
 * row-major), added into acc. bf16 needs k % 8 == 0. D == NULL means d = 0;
 * acc == NULL and D == C are refused; n == 0 is a no-op. */
int arrow_diffnorm_rows_f32(const float *C_dev, const float *D_dev, int64_t n,
                            int64_t k, double *acc_dev, void *stream);
int arrow_diffnorm_rows_f64(const double *C_dev, const double *D_dev,
                            int64_t n, int64_t k, double *acc_dev,
                            void *stream);
int arrow_diffnorm_rows_bf16(const uint16_t *C_dev, const uint16_t *D_dev,
                             int64_t n, int64_t k, double *acc_dev,
                             void *stream);

/* ---------------------------------------------------------------------
 * Operator scaling (ABI 1007). The loops of the affine step converge only
 * on a normalised operator: PageRank wants the column-stochastic A D^-1,
 * random-walk diffusion D^-1 A, GCN / APPNP D^-1/2 A D^-1/2. The reference
 * has no such call (its callers normalise the scipy matrix before they
 * decompose it); here the RESIDENT values are summed, and rescaled in
 * place as A <- diag(r) A diag(c), in one streaming pass each, with no
 * re-upload.
 *
 * Indexing, the same in both calls and the same as in the SpMM launches:
 * a row vector is indexed by OUTPUT row (after row_ids), as C and R are; a
 * column index c >= 0 indexes the *0 vector, as X0; c < 0 indexes the *1
 * vector at -c-1, as X1. The *1 vector may be the *0 vector. All vectors
 * are doubles in device memory, in every precision; the caller sizes them
 * as it sizes C, X0 and X1.
 *
 * arrow_csr_sums ADDS into its outputs (the caller zeroes them, so several
 * structures can share one vector): with f(v) = v, or |v| when absolute is
 * not 0, row_sum[row] += f(v), col_sum0[c] += f(v) or col_sum1[-c-1] +=
 * f(v), for every stored nonzero. All summation is double. A NULL output is
 * skipped; all three NULL is refused.
 *
 * arrow_csr_scale rewrites every stored value as
 *     val = (T)(((double)val * r) * c)
 * with r = row_scale[row], c the column factor, T the structure's
 * precision: two double multiplies in this order, ONE rounding to T (a
 * plain cast). A NULL vector is the factor 1; all three NULL returns 0 and
 * launches nothing.
 *
 * Both take float32 and float64 handles (bf16 features share the float32
 * structure) and leave work items, split table, queue segments and launch
 * plan untouched. A bad handle returns a negative code, sets
 * arrow_last_error() and launches nothing; nnz == 0 is a no-op returning
 * 0. Neither allocates nor reads on the host: both are legal under stream
 * capture. A SCALE MUST NOT OVERLAP IN TIME WITH AN SpMM, A SUMS OR ANOTHER
 * SCALE ON THE SAME STRUCTURE (order them on one stream, or synchronise).
 * ------------------------------------------------------------------- */
int arrow_csr_sums(int64_t handle, double *row_sum_dev, double *col_sum0_dev,
                   double *col_sum1_dev, int absolute, void *stream);
int arrow_csr_scale(int64_t handle, const double *row_scale_dev,
                    const double *col_scale0_dev, const double *col_scale1_dev,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* ARROW_SPMM_H */
