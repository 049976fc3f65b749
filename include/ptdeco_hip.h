/* ptdeco_hip.h -- C ABI of libptdeco_hip.so (gfx950 / MI355X).
 *
 * The reference (TCLResearchEurope/ptdeco v0.5.9) has no FFI layer: its hot
 * path is a sequence of ATen calls inside src/ptdeco/{dwain,falor}/decomposition.py.
 * Each entry point below replaces one group of those call sites; the citation
 * after each declaration names the reference lines it stands in for
 * (dwain.py = src/ptdeco/dwain/decomposition.py, falor.py = src/ptdeco/falor/decomposition.py,
 * losses.py = src/ptdeco/utils/losses_primitives.py).
 *
 * Conventions
 *  - plain C types only; every pointer except `stream` is a DEVICE pointer
 *  - matrices are row-major with an explicit leading dimension in ELEMENTS
 *  - `stream` is a hipStream_t passed as void*; every call is asynchronous on it
 *    unless stated otherwise, and never allocates or frees device memory: the
 *    caller passes workspaces sized by the matching *_workspace_bytes query
 *  - return value: 0 = ok, negative = ptd_status; ptd_last_error() gives the
 *    message of the last failing call on the calling thread
 *  - re-entrant across streams, devices and host threads.  Mutable state is kept per DEVICE and is
 *    advisory only (it selects between equivalent kernels, never results): lazily loaded code objects,
 *    the device facts queried once (CU count, architecture, occupancy of the whole-chip kernels), the
 *    ptd_set_concurrent_chains hint, the count of eigendecompositions this library has in flight on the
 *    device, and a back-off counter after a whole-chip kernel timed out
 */
#ifndef PTDECO_HIP_H
#define PTDECO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTD_ABI_VERSION 6   /* 2: ptd_nsr workspaces are initialised once (ptd_nsr_workspace_init); ptd_chol_inverse
                             * 3: ptd_streams_wall_us and a two-stream form of it, ptd_syrk_accumulate_multi
                             * 4: ptd_eigh_topk_batched, ptd_eigh_factored_prepare / _finish; ptd_band_reduce and the
                             *    two-stage reduction behind it are gone (2.2 x behind the default for three rounds)
                             * 5: the two-stream form of ptd_streams_wall_us is gone (the same call with count = 2)
                             * 6: PTD_F16 (IEEE half) wherever PTD_BF16 is accepted, same shapes, workspaces and codes
                             *    (added since, no entry changed: ptd_lowrank_decode_workspace_bytes, ptd_lowrank_decode,
                             *    ptd_lowrank_skinny_workspace_bytes, ptd_lowrank_skinny,
                             *    ptd_launch_trace_begin, ptd_launch_trace_end,
                             *    ptd_lowrank_decode_group_workspace_bytes, ptd_lowrank_decode_group,
                             *    ptd_lowrank_decode_gated_workspace_bytes, ptd_lowrank_decode_gated,
                             *    ptd_lowrank_skinny_gated_workspace_bytes, ptd_lowrank_skinny_gated,
                             *    ptd_lowrank_decode_w8_workspace_bytes, ptd_lowrank_decode_w8,
                             *    ptd_lowrank_skinny_w8_workspace_bytes, ptd_lowrank_skinny_w8,
                             *    ptd_lowrank_decode_w4_workspace_bytes, ptd_lowrank_decode_w4,
                             *    ptd_lowrank_plan,
                             *    ptd_lowrank_skinny_w4_workspace_bytes, ptd_lowrank_skinny_w4,
                             *    ptd_lowrank_decode_w6_workspace_bytes, ptd_lowrank_decode_w6,
                             *    ptd_lowrank_skinny_w6_workspace_bytes, ptd_lowrank_skinny_w6,
                             *    ptd_lowrank_dequant_w4, ptd_lowrank_dequant_w6,
                             *    ptd_lowrank_tile_w4_workspace_bytes, ptd_lowrank_tile_w4,
                             *    ptd_lowrank_tile_w6_workspace_bytes, ptd_lowrank_tile_w6,
                             *    ptd_lowrank_decode_group_q_workspace_bytes, ptd_lowrank_decode_group_q,
                             *    ptd_lowrank_decode_gated_q_workspace_bytes, ptd_lowrank_decode_gated_q,
                             *    ptd_lowrank_skinny_group_q_workspace_bytes, ptd_lowrank_skinny_group_q,
                             *    ptd_lowrank_skinny_gated_q_workspace_bytes, ptd_lowrank_skinny_gated_q,
                             *    ptd_mxfp8_quantize_rows, ptd_mx_product_a8,
                             *    ptd_lowrank_a8_w4_workspace_bytes, ptd_lowrank_a8_w4,
                             *    ptd_lowrank_a8_w6_workspace_bytes, ptd_lowrank_a8_w6,
                             *    ptd_mx_product_a8_tile,
                             *    ptd_lowrank_a8_tile_w4_workspace_bytes, ptd_lowrank_a8_tile_w4,
                             *    ptd_lowrank_a8_tile_w6_workspace_bytes, ptd_lowrank_a8_tile_w6,
                             *    ptd_nsr_plan,
                             *    ptd_gemm_f64_form) */

typedef enum { PTD_F32 = 0, PTD_F64 = 1, PTD_BF16 = 2, PTD_F16 = 3 } ptd_dtype;

typedef enum {
  PTD_OK = 0,
  PTD_ERR_INVALID = -1,     /* bad argument (shape, stride, dtype, alignment, null) */
  PTD_ERR_UNSUPPORTED = -2, /* dtype / layout combination not implemented */
  PTD_ERR_WORKSPACE = -3,   /* workspace too small */
  PTD_ERR_LAUNCH = -4,      /* HIP runtime reported an error */
  PTD_ERR_NOCONV = -5       /* eigensolver did not converge in max sweeps */
} ptd_status;

int ptd_version(void);
const char* ptd_last_error(void);

/* Host diagnostic for tests: which kernels did a call launch?  Every launch site of the library names its kernel family
 * in a label ("gemm_bf16 (short K)", "gemm_f32 (split K)", ...; one label may stand for two launches that always go
 * together, such as a split-K product and its reduction).  ptd_launch_trace_begin clears the trace of the CALLING
 * THREAD and switches it on; from then on each successful launch of that thread appends its label: 32 are kept, further
 * ones are only counted.  ptd_launch_trace_end switches the trace off and writes the kept labels in launch order,
 * joined by '\n', NUL-terminated and truncated to `cap` bytes (buf may be NULL when cap is 0); it returns the number of
 * labels recorded since begin (not of kernels: see above), those beyond 32 included, and 0 with an empty string without a begin.  Host state only: no
 * device code, no allocation, no environment variable; switched off (the default) a launch pays one thread-local flag
 * test.  No reference counterpart. */
void ptd_launch_trace_begin(void);
int ptd_launch_trace_end(char* buf, size_t cap);

/* Hint: the caller is about to run `chains` independent eigendecompositions at once, each on its own stream
 * (the reference has no counterpart: torch.linalg.eigh calls are serial, dwain.py:155-163).  With chains > 1 the
 * solver avoids kernels that claim a whole XCD or the whole chip for milliseconds (the resident kernels of the
 * tridiagonalisation), which shorten one chain and stall the others.  Applies to the CURRENT device (hipGetDevice of the
 * calling thread), default 1; returns the previous value.  Without the hint the library still notices its own
 * overlapping calls on a device (they take the blocked path), and the whole-chip kernels only run at all on an
 * unpartitioned 256-CU gfx950 whose occupancy query admits them; every inter-workgroup wait in them is bounded by a
 * 10 ms wall-clock time-out after which the reduction is repeated on the blocked path. */
int ptd_set_concurrent_chains(int chains);

/* Host diagnostic (synchronous): do these streams overlap?  The ROCm runtime maps the streams of a process onto 4
 * hardware queues per priority level, and two chains of dependent launches whose streams share one are executed one
 * packet after the other.  Launches one single-wave kernel that holds its queue for `spin_us` microseconds on each of
 * `count` streams (a HOST array of hipStream_t) and returns the wall time in *wall_us: about spin_us when all of them
 * ran side by side, a multiple when some were serialised.  Every stream is synchronised before and after.  No reference
 * counterpart (torch.linalg.eigh calls are serial, dwain.py:155-163); the tests check the dedicated streams below
 * with it. */
int ptd_streams_wall_us(void* const* streams, int count, int spin_us, double* wall_us);

/* A HIP stream with a hardware queue OF ITS OWN (ABI 4): hipExtStreamCreateWithCUMask over CUs [cu_first, cu_first +
 * cu_count) of the current device, cu_count = 0: every CU.  The runtime multiplexes ordinary streams onto four hardware
 * queues per priority (see above) and which streams share one cannot be told without measuring; a stream created with a
 * CU mask gets a queue that no other stream uses.  ptdeco_amd._engine runs the lanes of a precompute pass -- independent
 * chains of dependent launches, dwain.py:580-633's eigendecompositions -- on such streams, so that their overlap does not
 * depend on the creation order of every stream in the process.  *stream_out is a hipStream_t; the caller destroys it
 * with ptd_stream_destroy (or hipStreamDestroy).  No reference counterpart. */
int ptd_stream_create_dedicated(int cu_first, int cu_count, void** stream_out);
int ptd_stream_destroy(void* stream);

/* ---- covariance accumulation ------------------------------------------- */

/* E[i][j] += scale * sum_t Y[t][i] * Y[t][j]  for i >= j  (LOWER triangle only;
 * ptd_cov_finalize mirrors it).  Y is [T, n] (f32, bf16 or f16), E is [n, n] (f64 or f32).
 * The product is accumulated in f32 on the matrix cores and promoted on the add.
 * Replaces `Eyyt += einsum("bp,bq->pq", y, y) / T`: dwain.py:147-152, falor.py:160. */
int ptd_syrk_accumulate(const void* y, int64_t T, int64_t n, int64_t ldy, int y_dtype,
                        void* E, int64_t ldE, int E_dtype, double scale, void* stream);

/* The same sum over `steps` calibration steps in ONE pass over E (round 5, ABI 3):
 *   E[i][j] += sum_s ( scale * sum_t Y_s[t][i] * Y_s[t][j] ),  i >= j,
 * `ys` a HOST array of `steps` device pointers to [T, n] matrices of one dtype and row pitch.  dwain.py:147-152 is
 * called once per calibration step (D times per layer) and each call reads and writes the live triangle of the f64
 * accumulator: 8 n (n + 1) bytes against 2 T n of bf16 activations -- at n = 4096, T = 2048 that traffic, not the
 * matrix cores, bounds the call.  Here a tile's f64 sum stays in registers across the steps (each step's f32 product
 * is promoted at its end, in step order) and E is read and written once.  bf16 / f16: one launch per 8 steps; f32 (bound by
 * the matrix cores): step by step, identical to `steps` calls of ptd_syrk_accumulate. */
int ptd_syrk_accumulate_multi(const void* const* ys, int steps, int64_t T, int64_t n, int64_t ldy, int y_dtype,
                              void* E, int64_t ldE, int E_dtype, double scale, void* stream);

/* ey[j] += scale * sum_t Y[t][j], Y f32, bf16 or f16.   Replaces `Ey += y.mean(dim=0)`: falor.py:161. */
int ptd_colsum_accumulate(const void* y, int64_t T, int64_t n, int64_t ldy, int y_dtype,
                          void* ey, int ey_dtype, double scale, void* stream);

/* C = sym(E) / steps - (ey ? (ey / steps)(ey / steps)^T : 0);
 * C[i][i] += damp_factor * mean(diag(C)).   C is always f64 [n, n], full symmetric.
 * sym(E) reads the lower triangle of E; ey may be NULL, else it has E's dtype.
 * ws needs ptd_cov_finalize_workspace_bytes(n).
 * Replaces dwain.py:158-160, 207, 242 and falor.py:192-205. */
size_t ptd_cov_finalize_workspace_bytes(int64_t n);
int ptd_cov_finalize(const void* E, int64_t ldE, int E_dtype, const void* ey, int ey_dtype,
                     int64_t n, double steps, double damp_factor, double* C, int64_t ldC,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- symmetric eigendecomposition ---------------------------------------- */

/* All eigenpairs of the symmetric positive semi-definite f64 matrix A [n, n]
 * (full storage), eigenvalues ascending in evals[n], eigenvectors in the COLUMNS
 * of evecs [n, n] (row-major, ld ldv) -- the layout torch.linalg.eigh returns.
 * A is not modified.  Two solvers (env PTD_EIGH_METHOD = auto | tridiag | jacobi, default auto):
 *   tridiagonal route (n >= 256 in auto): blocked Householder reduction whose per-column
 *     SYMV streams the trailing matrix from HBM / Infinity Cache, eigenvalues by multisection,
 *     eigenvectors by inverse iteration, compact-WY back-transformation on the f64 matrix
 *     cores.  Requested eigenvalues closer than 1e-10 |A|, or chains of more than 48 closer than 1e-7 |A| (a
 *     dominant outlier above a dense bulk), get all computed vectors orthonormalised by one Cholesky-QR pass; a
 *     cluster at the BOTTOM of the spectrum that reaches into the request (a rank-deficient covariance on its
 *     damping floor) is completed with an orthonormal basis of the complement of the vectors above it, each of
 *     which is an eigenvector of the cluster.  Refused -- and handed to the solver below -- only when requested
 *     eigenvalues elsewhere are closer than 1e-13 |A| (PTD_EIGH_LONG_CHAINS=0, PTD_EIGH_NULL_COMPLETION=0:
 *     the earlier, stricter rule);
 *   one-sided block Jacobi on the f64 matrix cores: any PSD matrix.  It diagonalises A^2, so an indefinite A (told
 *     from a semi-definite one by sum |lambda_i| - trace(A) > 16 n eps sum |lambda_i|) is solved a second time as
 *     A + s I, s just above |A|, and the eigenvalues are shifted back: absolute accuracy eps (|A| + s) for a matrix
 *     the test detects.  Below its threshold it is blind: negative eigenvalues whose moduli sum to less than
 *     8 n eps sum |lambda_i| pass for the rounding of a semi-definite matrix and are returned as + |lambda| (up to
 *     ~4e-11 |A| at n = 130).  The tridiagonal route needs no sign.
 * NOT fully asynchronous: synchronises `stream` to read small decisions back (cluster
 * check, Jacobi convergence flag).  sweeps_out (host pointer, may be NULL) receives the number
 * of Jacobi sweeps (0 for the tridiagonal route; the sum of both passes, up to 80, for an indefinite matrix).
 * Replaces `torch.linalg.eigh`: dwain.py:162, falor.py:207. */
size_t ptd_eigh_workspace_bytes(int64_t n);
int ptd_eigh(const double* A, int64_t lda, int64_t n, double* evals, double* evecs, int64_t ldv,
             void* ws, size_t ws_bytes, int* sweeps_out, void* stream);

/* Same, but only the eigenvectors of the k LARGEST eigenvalues are formed: evecs is [n, k]
 * (ld ldv >= k), column c holds the eigenvector of evals[n - k + c].  evals always has n entries:
 * with all_values != 0 every eigenvalue is computed; with all_values == 0 the tridiagonal route
 * computes only evals[n - k - 1 .. n) and fills the rest with NaN (the Jacobi route always
 * returns all of them) -- the drivers never read eigenvalues.  dwain never looks above the largest
 * candidate rank it evaluates (dwain.py:407-421, 424-426), so most of the inverse iterations and of
 * the back-transformation are skipped, and a dense cluster at the low end of the spectrum no
 * longer forces the Jacobi fallback.
 * With all_values == 0, n >= 2048 (a multiple of 128) and 7 k <= 2 n the eigenpairs come from a
 * Chebyshev-filtered subspace iteration on the f64 matrix cores (only evals[n - k .. n) are set then,
 * NaN below; every returned pair has passed a residual check |A v - lambda v| <= 1e-10 |lambda_max|,
 * eigenvector signs: largest entry positive); where that route does not apply -- a flat spectrum, a
 * breakdown -- the direct reduction answers with the same contract.  A is read only. */
int ptd_eigh_topk(const double* A, int64_t lda, int64_t n, int64_t k, int all_values, double* evals,
                  double* evecs, int64_t ldv, void* ws, size_t ws_bytes, int* sweeps_out, void* stream);

/* The f32 face of ptd_eigh_topk: A [n, n] f32 (full storage, symmetric), evals[n] and evecs [n, k] f32, same conventions.
 * The arithmetic is f64 on a converted copy (the routes above), the results are rounded to f32 -- at least as accurate as
 * the f32 `torch.linalg.eigh` the reference runs with decompose_in_float64=False (dwain.py:224-233, 162; falor's
 * use_float64=False, falor.py:181-186, 207). */
size_t ptd_eigh_f32_workspace_bytes(int64_t n, int64_t k);
int ptd_eigh_topk_f32(const float* A, int64_t lda, int64_t n, int64_t k, int all_values, float* evals, float* evecs,
                      int64_t ldv, void* ws, size_t ws_bytes, int* sweeps_out, void* stream);

/* ptd_eigh_topk for `count` matrices of ONE order and ONE k in a single call (ABI 4): As / evals / evecs are HOST arrays
 * of `count` device pointers, every matrix [n, n] with leading dimension lda, every evecs [n, k] with ldv; results and
 * contract per matrix exactly as ptd_eigh_topk.  Replaces the LOOP of `torch.linalg.eigh` calls of dwain's precompute
 * pass (dwain.py:580-633 calls get_eigenvectors -> :162 once per layer of a split): the direct reduction is a chain
 * of ~2 n dependent launches per matrix, so the matrices advance column by column in lockstep and every launch
 * serves all of them (blockIdx.y = matrix) -- one host thread, one stream, one host synchronisation for the batch,
 * where round 5 ran one thread and one stream per layer.  Requests the filtered route serves (see above) and single
 * matrices are solved one after the other exactly as ptd_eigh_topk would; two matrices are batched from n = 512 on
 * (PTD_EIGH_BATCH_MIN_N), three or more always.  `all_values` is a set of flags: bit 0 = every
 * eigenvalue is wanted (as in ptd_eigh_topk), bit 1 (PTD_EIGH_FLAG_DIRECT) = take the direct reduction also where the
 * filtered route would serve the request, so that the matrices are batched: for a caller whose pass already runs
 * latency-bound reductions of this order on other streams, beside which the filter's f64 products only share the matrix
 * cores (two Llama blocks: q / o as two filtered problems each 75-127 ms in the pass, as one more batch 40).  stats (HOST pointer, may be NULL): the
 * ptd_eigh_profiled figures of the batch (method 1: `sweeps` = matrices per launch, work[0] = algorithmic bytes of
 * all of them) or of the last matrix when solved one by one.  Workspace: ptd_eigh_batched_workspace_bytes. */
#define PTD_EIGH_FLAG_ALL_VALUES 1
#define PTD_EIGH_FLAG_DIRECT 2
size_t ptd_eigh_batched_workspace_bytes(int64_t n, int64_t k, int count);
struct ptd_eigh_stats_s;
int ptd_eigh_topk_batched(const double* const* As, int64_t lda, int count, int64_t n, int64_t k, int all_values,
                          double* const* evals, double* const* evecs, int64_t ldv, void* ws, size_t ws_bytes,
                          struct ptd_eigh_stats_s* stats, void* stream);

/* The filtered route remembers LATE declines (a breakdown after its products were spent) per calling thread, device and
 * shape, and sends the next requests of that shape straight to the direct route (1, 2, 4, ... of them after the second
 * decline in a row).  This call clears the calling thread's memory: the drivers issue it at the start of every
 * decompose_in_place, so that the route a layer takes depends on that call's own sequence of requests only (two runs in
 * one process produce identical results).  No reference counterpart. */
void ptd_eigh_forget_declines(void);

/* The solver ptd_eigh_topk would try FIRST for this request: 3 = filtered subspace iteration (chip-filling f64
 * products: concurrent chains gain nothing), 1 = direct tridiagonal reduction (a latency-bound chain of short
 * launches: independent matrices overlap well on separate streams), 0 = Jacobi.  A host-side query; the filtered
 * route may still decline at run time (flat spectrum) and hand over to the direct one. */
int ptd_eigh_route(int64_t n, int64_t k, int all_values);

/* Top-k eigenpairs of C = W Ex W^T without forming C, for a layer that widens its input
 * (n_o > n_i; Llama gate / up: 4096 -> 14336): W [n_o, n_i] (f32, bf16, f16 or f64, ld ldw),
 * Ex [n_i, n_i] f64 full symmetric = sum over steps of x^T x / T / steps (the INPUT second
 * moment; C is then exactly the feature covariance the reference accumulates, dwain.py:147-152,
 * since y = x W^T).  U [n_o, k] f64 gets the eigenvectors of the k largest eigenvalues
 * (ascending, same convention as ptd_eigh_topk), evals_k[k] (may be NULL) the eigenvalues of C.
 * G = W^T W = L L^T, B = L^T Ex L, B s = lambda s, u = W L^-T s: a n_i^2 eigenproblem plus
 * five f64 MFMA products.  Returns PTD_ERR_UNSUPPORTED if W^T W is not numerically positive
 * definite (then accumulate Y^T Y and call ptd_eigh_topk). */
size_t ptd_eigh_factored_workspace_bytes(int64_t n_o, int64_t n_i, int64_t k);
int ptd_eigh_factored(const void* W, int64_t ldw, int w_dtype, int64_t n_o, int64_t n_i,
                      const double* Ex, int64_t ldx, int64_t k, double* evals_k, double* U, int64_t ldu,
                      void* ws, size_t ws_bytes, void* stream);

/* ptd_eigh_factored in two halves around an eigendecomposition the CALLER runs (ABI 4), so that the inner n_i-sized
 * problems of several layers (Llama gate, up) and the same-sized covariances of others (down) share one
 * ptd_eigh_topk_batched call.  prepare: G = W^T W = L L^T, B = L^T Ex L; *B_out (HOST pointers to results) receives the
 * device address of B [np, np] (f64, full symmetric, ld np) inside the workspace and *np_out = np = n_i rounded up to
 * 64 (the padding carries exact, tiny eigenvalues that never reach the top k).  Synchronises the stream once (the
 * Cholesky status); PTD_ERR_UNSUPPORTED as ptd_eigh_factored.  finish: evals [np] ascending and S [np, k] (ld lds)
 * = eigenvectors of B's k largest eigenvalues -> U [n_o, k] = W L^-T S, evals_k (may be NULL).  The SAME workspace
 * (ptd_eigh_factored_workspace_bytes(n_o, n_i, k)), untouched in between.  Same reference lines as ptd_eigh_factored
 * (dwain.py:147-163). */
int ptd_eigh_factored_prepare(const void* W, int64_t ldw, int w_dtype, int64_t n_o, int64_t n_i, const double* Ex,
                              int64_t ldx, int64_t k, void* ws, size_t ws_bytes, double** B_out, int64_t* np_out,
                              void* stream);
int ptd_eigh_factored_finish(int64_t n_o, int64_t n_i, int64_t k, const double* evals, const double* S, int64_t lds,
                             double* evals_k, double* U, int64_t ldu, void* ws, size_t ws_bytes, void* stream);

/* Same, with per-phase device timing (HIP events on `stream` around the launches of each
 * phase; a few percent slower, for bench.py's roofline lines).  `stats` is a HOST pointer.
 *   method 0 (Jacobi):       phase 0 jac_gram, 1 jac_inner, 2 jac_update            (work = f64 flops executed)
 *   method 1 (tridiagonal):  phase 0 the per-column SYMV launches (work = algorithmic BYTES: the full
 *                            trailing square a one-stage SYMV streams, 8/3 n^3 in total; ms from
 *                            dispatch-attached events on every 8th launch, scaled), 1 the rest of the
 *                            reduction (alpha kernels, rank-2k updates, launch gaps), 2 work only
 *                            (flops of the rank-2k updates), 3 eigenvalues + inverse iteration +
 *                            back-transformation
 *   method 3 (filtered subspace iteration, the route of ptd_eigh_topk with all_values = 0, n >= 2048, 7 k <= 2 n):
 *                            ms = {Lanczos bounds, filter rounds (products with C + Cholesky-QR passes), the
 *                            Rayleigh-Ritz eigenproblem of order launches[2], Ritz products + residual check};
 *                            launches = {Lanczos steps, products with C, subspace dimension m, 0};
 *                            work[1] = flop of the products with C (2 n^2 m each) */
typedef struct ptd_eigh_stats_s {
  int method;
  int sweeps;        /* Jacobi sweeps; 0 for the tridiagonal route (ptd_eigh_topk_batched: matrices per launch) */
  int launches[4];
  float ms[4];       /* summed device time of the phase's launches */
  double work[4];
  float total_ms;    /* first launch to last launch of the call */
} ptd_eigh_stats;
int ptd_eigh_profiled(const double* A, int64_t lda, int64_t n, int64_t k, int all_values, double* evals,
                      double* evecs, int64_t ldv, void* ws, size_t ws_bytes, ptd_eigh_stats* stats, void* stream);

/* Diagnostic: Householder tridiagonalisation T = Q^T A Q of a symmetric f64 matrix (full
 * storage) and the eigenvalues of T by bisection.  d[n], e[n] (e[n-1] unused), evals[n]
 * ascending; any of the three may be NULL. */
size_t ptd_tridiagonalize_workspace_bytes(int64_t n);
int ptd_tridiagonalize(const double* A, int64_t lda, int64_t n, double* d, double* e, double* evals,
                       void* ws, size_t ws_bytes, void* stream);

/* Diagnostic: the Cholesky sweep of the filtered eigensolver's orthonormalisation passes on its own (the
 * step that replaces nothing in the reference -- torch.linalg.eigh hides it -- but is the latency-critical
 * part of ptd_eigh_topk's filtered route).  G [m, m] row-major f64, symmetric positive definite, lower
 * 64 x 64 tiles read, DESTROYED; Wt [m, m] receives L^-T (upper triangular, G = L L^T), so that X Wt has
 * orthonormal columns when G = X^T X.  m a multiple of 64 in [64, 8192].  Synchronises the stream once;
 * PTD_ERR_UNSUPPORTED when a pivot is not positive. */
size_t ptd_chol_inverse_workspace_bytes(int64_t m);
int ptd_chol_inverse(double* G, int64_t m, double* Wt, void* ws, size_t ws_bytes, void* stream);

/* ---- dense products (layer output, factor construction) ----------------- */

/* C[M,N] = alpha * sum_k A(m,k) * B(k,n) (+ bias[n]),  f32, bf16 or f16 operands,
 * f32 accumulation on the matrix cores.  Operands are addressed with explicit
 * element strides: A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]; exactly
 * one stride of each operand must be 1.  C is row-major [M, N] with ld ldc, of
 * dtype c_dtype (f32, or the operands' type when they are bf16 or f16 -- bias of that type too, 16-bit results rounded
 * to nearest even, f16 beyond +-65504 to +-inf; f64 x f64 -> f64 without bias
 * is also available, it is what the eigensolver uses internally).
 * Replaces `x @ weight.T` (dwain.py:194, 239; falor.py:159), `orig_weight.T @ uk`
 * and `(U @ V).T` (dwain.py:427-429, 511; falor.py:347-348). */
int ptd_gemm(const void* A, int64_t sam, int64_t sak, const void* B, int64_t sbk, int64_t sbn,
             void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int ab_dtype, int c_dtype,
             double alpha, const void* bias, void* stream);

/* The same product with a workspace (ABI 4).  A product with few output tiles -- T = 1576 rows of a ViT batch
 * against a 768-column layer are 78 tiles of 128 x 128 for 256 CUs -- has its K range split over workgroups; the
 * partial tiles go to f32 slabs in the workspace and a second launch adds them in index order (results do not
 * depend on scheduling).  ptd_gemm_workspace_bytes returns 0 where no split would be made; ws may be NULL
 * (= ptd_gemm). */
size_t ptd_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int ab_dtype, int c_dtype);
int ptd_gemm_ws(const void* A, int64_t sam, int64_t sak, const void* B, int64_t sbk, int64_t sbn,
                void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int ab_dtype, int c_dtype,
                double alpha, const void* bias, void* ws, size_t ws_bytes, void* stream);

/* Diagnostic for tests: the f64 product in the forms the eigensolver calls it in, which ptd_gemm (always the plain form)
 * does not reach.  The entry forwards to the functions the solver itself calls and has no arithmetic or routing of its
 * own; operands are addressed as in ptd_gemm, C is row-major with ld ldc.
 *   PTD_GEMM_F64_PLAIN       C  = alpha A B
 *   PTD_GEMM_F64_ACCUMULATE  C += alpha A B                      (ksplit must be 1: see below)
 *   PTD_GEMM_F64_SLABS       K is cut into at most `ksplit` ranges of a multiple of 16; range y writes alpha A(:, range)
 *                            B(range, :) to C + y * slab (slab in elements, >= M * ldc); *nslabs gets the number of
 *                            ranges.  lower_only != 0: tiles that lie entirely above the diagonal may be left unwritten
 *   PTD_GEMM_F64_PAIR        C += alpha (A B + A2 B2), both pairs with the same strides; row0_out (optional) also gets the
 *                            updated row 0 of C; batch > 1: the same update on `batch` operand sets, EVERY pointer
 *                            (row0_out included) moving by bstride elements per member
 * Arguments a form does not use are ignored (A2, B2, row0_out, nslabs may then be NULL).  PTD_ERR_INVALID for a null
 * pointer the form needs, ldc < N, an operand without exactly one unit stride, a negative dimension or one of 2^31 or
 * more, ksplit < 1, batch < 1, a negative bstride, slab < M * ldc or an unknown form.  ACCUMULATE with ksplit > 1 is the
 * K split with f64 atomics: it has no caller, its result depends on scheduling, and this entry answers
 * PTD_ERR_UNSUPPORTED for it.
 * Launch labels: "gemm_f64 (lds-dma)" for the 128-row LDS-DMA kernel, "gemm_f64" for the 64 x 64 kernel. */
#define PTD_GEMM_F64_PLAIN 0
#define PTD_GEMM_F64_ACCUMULATE 1
#define PTD_GEMM_F64_SLABS 2
#define PTD_GEMM_F64_PAIR 3
int ptd_gemm_f64_form(int form, const double* A, int64_t sam, int64_t sak, const double* B, int64_t sbk, int64_t sbn,
                      const double* A2, const double* B2, double* C, int64_t ldc, int64_t slab, int64_t M, int64_t N,
                      int64_t K, double alpha, int ksplit, int lower_only, int* nslabs, double* row0_out, int batch,
                      int64_t bstride, void* stream);

/* y[T,n_o] = (x[T,n_i] @ A[r,n_i]^T) @ B[n_o,r]^T (+ bias[n_o]), dtype f32, bf16 or f16.  The workspace holds the
 * [T, r] intermediate of the operand dtype and, for f32 operands with a small rank, the partial
 * tiles of the first product's K split (added in a fixed order: results do not depend on
 * scheduling).  The decomposed layer's forward: dwain.py:74-85 / falor.py:84-95 (two nn.Linear),
 * dwain.py:126-144 (two 1x1 convs, x viewed as [B*H*W, C]). */
size_t ptd_lowrank_forward_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_forward(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda,
                        int64_t r, const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y,
                        int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream);

/* The same pair for 1 <= T <= 16 tokens (token-by-token generation): two weight-streaming kernels on the caller's
 * stream that read every factor element once (arguments as ptd_lowrank_forward; same rounding points: f32 sums, h
 * rounded once to the operand dtype, y once).  Row t of y depends on row t of x alone, bit for bit, whatever T is.
 * Served: dtype f32 / bf16 / f16, 1 <= T <= 16, r >= 8, n_i, r and the leading dimensions ldx, lda, ldb multiples of 8
 * (f32: 4), x, A and B 16-byte aligned, any n_o >= 1, bias optional.  Anything else returns PTD_ERR_UNSUPPORTED
 * before a kernel is launched (the caller then takes ptd_lowrank_forward); null pointers, a leading dimension below
 * its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The workspace holds
 * the f32 partial sums of the first product's K split, added in a fixed order. */
size_t ptd_lowrank_decode_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_decode(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r,
                       const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy,
                       void* ws, size_t ws_bytes, int dtype, void* stream);

/* The pair at 1 <= T <= 16 tokens with 8-bit factors (weight-only quantisation: 8-bit weights, 16-bit activations):
 * x [T, n_i], bias [n_o] and y [T, n_o] in dtype D = bf16 or f16, Aq [r, n_i] and Bq [n_o, r] in OCP e4m3fn (one byte
 * per weight, lda / ldb in bytes = elements), scale_a [r] and scale_b [n_o] in f32, one scale per factor row:
 *   h[t, i] = round_D(scale_a[i] * sum_k x[t, k] Aq[i, k]),   y[t, o] = round_D(scale_b[o] * sum_i h[t, i] Bq[o, i] + bias[o])
 * with the sums in f32, each rounded ONCE.  Two weight-streaming kernels on the caller's stream, as ptd_lowrank_decode:
 * every weight byte is read once and converted to D in registers (exactly: every e4m3 value is a bf16 and an f16
 * value), no dequantised copy is kept, and row t of y depends on row t of x alone, bit for bit, whatever T is.
 * w_format: PTD_W8_FP8_E4M3.  Served: dtype bf16 / f16, 1 <= T <= 16, r >= 16, n_i and r multiples of 16, lda and ldb
 * multiples of 16, ldx a multiple of 8, x, Aq and Bq 16-byte aligned, the scales 4-byte aligned, any n_o >= 1, bias
 * optional.  Anything else (f32, another w_format) returns PTD_ERR_UNSUPPORTED before a kernel is launched; null
 * pointers, a leading dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace
 * PTD_ERR_WORKSPACE.  The workspace holds the f32 partial sums of the first product's K split, added in a fixed order.
 * No reference counterpart. */
#define PTD_W8_FP8_E4M3 0
size_t ptd_lowrank_decode_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_decode_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                          const void* Aq, int64_t lda, const float* scale_a, int64_t r,
                          const void* Bq, int64_t ldb, const float* scale_b, int64_t n_o, const void* bias,
                          void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* The pair at 1 <= T <= 16 tokens with OCP MXFP4 factors (weight-only quantisation: 4.25 bits per weight, 16-bit
 * activations): x [T, n_i], bias [n_o] and y [T, n_o] in dtype D = bf16 or f16; Aq [r, n_i / 2] and Bq [n_o, r / 2] bytes of
 * packed e2m1 codes, scale_a [r, n_i / 32] and scale_b [n_o, r / 32] bytes of e8m0 block scales, one per 32 consecutive
 * weights of a row; lda, ldb, ldsa and ldsb in bytes.
 *   code(W, i, k) = (Wq[i, k >> 1] >> (4 * (k & 1))) & 15          (low nibble = even k)
 *   val(c)        = (c & 8 ? -1 : 1) * {0, .5, 1, 1.5, 2, 3, 4, 6}[c & 7]
 *   W^[i, k]      = val(code(W, i, k)) * 2^(clamp(scale[i, k >> 5], 114, 140) - 127)
 *   h[t, i] = round_D(sum_k x[t, k] A^[i, k]),   y[t, o] = round_D(sum_i h[t, i] B^[o, i] + bias[o])
 * with the sums in f32, each rounded ONCE.  The clamp is part of the semantics: a block exponent in [-13, 13] makes every
 * W^ a normal number of bf16 and of f16, so the conversion in registers rounds nothing and the result does not depend on
 * denormal modes.  There are no per-row scales: this is ptd_lowrank_decode on the dequantised factors, with its rounding
 * points.  Two weight-streaming kernels on the caller's stream: a lane's 16-byte load is one block, converted to D in
 * registers with the block scale applied by the same instruction; no dequantised copy is kept, and row t of y depends on
 * row t of x alone, bit for bit, whatever T is.  w_format: PTD_W4_MXFP4.  Served: dtype bf16 / f16, 1 <= T <= 16,
 * r >= 32, n_i and r multiples of 32, lda and ldb multiples of 16 (lda >= n_i / 2, ldb >= r / 2), ldsa >= n_i / 32 and
 * ldsb >= r / 32 (the scale rows need no alignment), ldx a multiple of 8, x, Aq and Bq 16-byte aligned, any n_o >= 1,
 * bias optional.  Anything else (f32, another w_format) returns PTD_ERR_UNSUPPORTED before a kernel is launched; null
 * pointers, a leading dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace
 * PTD_ERR_WORKSPACE.  The workspace holds the f32 partial sums of the first product's K split, added in a fixed order.
 * No reference counterpart. */
#define PTD_W4_MXFP4 0
size_t ptd_lowrank_decode_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_decode_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                          const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                          const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                          void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* 1 <= count <= PTD_LOWRANK_GROUP_MAX pairs that read the same x at decode shapes (the q / k / v or gate / up projections
 * of a decomposed transformer block) in two launches on the caller's stream instead of two per pair.  Member m has its
 * own A[m] [r[m], n_i], B[m] [n_o[m], r[m]], optional bias[m] and output y[m] [T, n_o[m]] with row pitch ldy[m] (the
 * column blocks of one [T, sum n_o] tensor, or unrelated buffers); x, T, n_i and dtype are common.  Every y[m] holds the
 * bits ptd_lowrank_decode gives for that member alone.  The argument arrays are read before the call returns and not
 * after it (the call may be captured in a graph).  Served when every member is served by ptd_lowrank_decode with the
 * common x, T, n_i and dtype; anything else, count outside 1 .. PTD_LOWRANK_GROUP_MAX included, returns
 * PTD_ERR_UNSUPPORTED before a kernel is launched.  Null pointers (bias, or an entry of it, may be NULL), a leading
 * dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The
 * workspace is the sum of the members' ptd_lowrank_decode workspaces (each a multiple of 256 bytes). */
#define PTD_LOWRANK_GROUP_MAX 4
size_t ptd_lowrank_decode_group_workspace_bytes(int count, int64_t T, int64_t n_i, const int64_t* r, int dtype);
int ptd_lowrank_decode_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                             const void* const* A, const int64_t* lda, const int64_t* r,
                             const void* const* B, const int64_t* ldb, const int64_t* n_o,
                             const void* const* bias /* entries may be NULL; the array may be NULL */,
                             void* const* y, const int64_t* ldy,
                             void* ws, size_t ws_bytes, int dtype, void* stream);

/* The gated pair of a decomposed MLP at decode shapes, y = act(gate(x)) * up(x) with gate = (Ag [r_g, n_i], Bg [n_ff, r_g],
 * bias_g) and up = (Au [r_u, n_i], Bu [n_ff, r_u], bias_u) on the same x [T, n_i], in two launches on the caller's stream:
 * both first products, then a kernel that forms both second products row tile by row tile and applies the activation
 * and the product in the lane that holds both sums (no [T, 2 n_ff] intermediate, no elementwise launch).  g and u are
 * the bits ptd_lowrank_decode stores for gate and up; the activation is evaluated in f32 on g and rounded once to the
 * dtype, its product with u is formed in f32 and rounded once -- the rounding points of the unfused act(g) * u.
 * act: PTD_ACT_SILU v / (1 + exp(-v)), PTD_ACT_GELU_TANH 0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3))),
 * PTD_ACT_RELU.  Served when both members are served by ptd_lowrank_decode with the common x, T, n_i, n_ff and dtype
 * and act is one of the three; anything else returns PTD_ERR_UNSUPPORTED before a kernel is launched.  Null pointers
 * (either bias may be NULL), a leading dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a
 * short workspace PTD_ERR_WORKSPACE.  The workspace is the sum of the two members' ptd_lowrank_decode workspaces. */
#define PTD_ACT_SILU 0
#define PTD_ACT_GELU_TANH 1
#define PTD_ACT_RELU 2
size_t ptd_lowrank_decode_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype);
int ptd_lowrank_decode_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                             const void* Ag, int64_t lda_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* bias_g,
                             const void* Au, int64_t lda_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* bias_u,
                             int64_t n_ff, int act, void* y, int64_t ldy,
                             void* ws, size_t ws_bytes, int dtype, void* stream);

/* The same pair for 32 <= T <= 96 tokens (continuous batching, speculative verification, short prompt chunks) in
 * bf16 / f16: skinny products on the caller's stream in which the first product's K range is split into f32 slabs,
 * added in a fixed order and rounded once to h (arguments as ptd_lowrank_forward; same rounding points: f32 sums, h
 * rounded once to the operand dtype, the bias added in f32, y rounded once).  The split depends on (n_i, r) alone: row
 * t of y depends on row t of x alone, bit for bit, whatever T is.  Served: dtype bf16 / f16, 32 <= T <= 96, r >= 8,
 * n_i, r and the leading dimensions ldx, lda, ldb multiples of 8, x, A and B 16-byte aligned, any n_o >= 1, bias
 * optional.  Anything else (f32 included) returns PTD_ERR_UNSUPPORTED before a kernel is launched (the caller then
 * takes ptd_lowrank_forward); null pointers, a leading dimension below its row length or a misaligned workspace
 * PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The workspace holds the slabs and h. */
size_t ptd_lowrank_skinny_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_skinny(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r,
                       const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy,
                       void* ws, size_t ws_bytes, int dtype, void* stream);

/* The pair with 8-bit factors (arguments, formats and semantics of ptd_lowrank_decode_w8: h and y from f32 sums, each
 * scaled in f32 and rounded ONCE) for 32 <= T <= PTD_LOWRANK_SKINNY_W8_MAX_T tokens, with the structure of
 * ptd_lowrank_skinny: three launches on the caller's stream (first product into f32 slabs of a K split that depends on
 * (n_i, r) alone, slab sum with scale_a into a 16-bit h, second product with scale_b and the bias).  Every weight byte
 * is converted to D in registers on its way to the matrix cores; no dequantised copy is kept; row t of y depends on
 * row t of x alone, bit for bit, whatever T is.  Served: dtype bf16 / f16, w_format PTD_W8_FP8_E4M3, 32 <= T <=
 * PTD_LOWRANK_SKINNY_W8_MAX_T, r >= 16, n_i and r multiples of 16, lda and ldb multiples of 16, ldx a multiple of 8,
 * x, Aq and Bq 16-byte aligned, the scales 4-byte aligned, any n_o >= 1, bias optional.  Anything else returns
 * PTD_ERR_UNSUPPORTED before a kernel is launched; null pointers, a leading dimension below its row length or a
 * misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The workspace holds the slabs and h (the
 * formula of ptd_lowrank_skinny_workspace_bytes).  No reference counterpart. */
#define PTD_LOWRANK_SKINNY_W8_MAX_T 96
size_t ptd_lowrank_skinny_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_skinny_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                          const void* Aq, int64_t lda, const float* scale_a, int64_t r,
                          const void* Bq, int64_t ldb, const float* scale_b, int64_t n_o, const void* bias,
                          void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* The pair with OCP MXFP4 factors (arguments, formats and semantics of ptd_lowrank_decode_w4, clamp included: h and y
 * from f32 sums, each rounded ONCE; no per-row scales) for 32 <= T <= PTD_LOWRANK_SKINNY_W4_MAX_T tokens, with the
 * structure of ptd_lowrank_skinny_w8: three launches on the caller's stream (first product into f32 slabs of a K split
 * that depends on (n_i, r) alone, slab sum into a 16-bit h, second product with the bias).  A lane's 8-byte load is half
 * an MX block, converted to D in registers with the clamped block scale applied by the same instruction; no dequantised
 * copy is kept; row t of y depends on row t of x alone, bit for bit, whatever T is.  Served: dtype bf16 / f16, w_format
 * PTD_W4_MXFP4, 32 <= T <= PTD_LOWRANK_SKINNY_W4_MAX_T, r >= 32, n_i and r multiples of 32, lda and ldb multiples of 8
 * bytes (lda >= n_i / 2, ldb >= r / 2), ldsa >= n_i / 32 and ldsb >= r / 32 (the scale rows need no alignment), ldx a
 * multiple of 8, x 16-byte aligned, Aq and Bq 8-byte aligned, bias 2-byte aligned and optional, n_i < 2^30, r < 2^27,
 * 1 <= n_o < 2^30.  Anything else returns PTD_ERR_UNSUPPORTED before a kernel is launched; null pointers, a leading
 * dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The
 * workspace holds the slabs and h (the formula of ptd_lowrank_skinny_workspace_bytes).  The cap is measured
 * (profiles/pair_skinny_w4.json).  No reference counterpart. */
#define PTD_LOWRANK_SKINNY_W4_MAX_T 96
size_t ptd_lowrank_skinny_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_skinny_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                          const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                          const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                          void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* The pair at 1 <= T <= 16 tokens with OCP MXFP6 factors, E2M3 elements (weight-only quantisation: 6.25 bits per weight,
 * 16-bit activations): x [T, n_i], bias [n_o] and y [T, n_o] in dtype D = bf16 or f16; Aq [r, 3 n_i / 4] and
 * Bq [n_o, 3 r / 4] bytes of packed 6-bit codes, scale_a [r, n_i / 32] and scale_b [n_o, r / 32] bytes of e8m0 block
 * scales, one per 32 consecutive weights of a row; lda, ldb, ldsa and ldsb in bytes.  Block b of row i is bytes
 * 24 b .. 24 b + 23 of the row, read as one 192-bit little-endian integer; the code of k = 32 b + j sits at its bits
 * 6 j .. 6 j + 5:
 *   code(W, i, k) = (block(W, i, k >> 5) >> (6 * (k & 31))) & 63
 *   val(c)        = (c & 32 ? -1 : 1) * (E == 0 ? M / 8 : (1 + M / 8) * 2^(E - 1)),   E = (c >> 3) & 3,  M = c & 7
 *                   (magnitudes 0, 0.125, ..., 7.5)
 *   W^[i, k]      = val(code(W, i, k)) * 2^(clamp(scale[i, k >> 5], 116, 140) - 127)
 *   h[t, i] = round_D(sum_k x[t, k] A^[i, k]),   y[t, o] = round_D(sum_i h[t, i] B^[o, i] + bias[o])
 * with the sums in f32, each rounded ONCE.  The clamp is part of the semantics: a block exponent in [-11, 13] makes every
 * non-zero W^ a normal number of f16 (2^-3 * 2^-11 = 2^-14, 7.5 * 2^13 = 61440) and of bf16, so the conversion in
 * registers rounds nothing and the result does not depend on denormal modes.  There are no per-row scales: this is
 * ptd_lowrank_decode on the dequantised factors, with its rounding points.  Two weight-streaming kernels on the caller's
 * stream: a lane's 24-byte load is one block, converted to D in registers by one instruction that applies the block
 * scale; no dequantised copy is kept, and row t of y depends on row t of x alone, bit for bit, whatever T is.  w_format:
 * PTD_W6_MXFP6_E2M3.  Served: dtype bf16 / f16, 1 <= T <= 16, r >= 32, n_i and r multiples of 32, lda and ldb multiples
 * of 8 (lda >= 3 n_i / 4, ldb >= 3 r / 4), ldsa >= n_i / 32 and ldsb >= r / 32 (the scale rows need no alignment), ldx a
 * multiple of 8, x 16-byte aligned, Aq and Bq 8-byte aligned, any n_o >= 1, bias optional.  Anything else (f32, another
 * w_format) returns PTD_ERR_UNSUPPORTED before a kernel is launched; null pointers, a leading dimension below its row
 * length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The workspace holds the f32
 * partial sums of the first product's K split, added in a fixed order.  No reference counterpart. */
#define PTD_W6_MXFP6_E2M3 0
size_t ptd_lowrank_decode_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_decode_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                          const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                          const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                          void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* 1 <= count <= PTD_LOWRANK_GROUP_MAX pairs with quantised factors of ONE format that read the same x at decode shapes
 * (the q / k / v or gate / up projections of a quantised, decomposed transformer block) in two launches on the caller's
 * stream instead of two per pair.  q_format: PTD_Q_FP8_E4M3 (operands and semantics of ptd_lowrank_decode_w8: sa[m] [r[m]]
 * and sb[m] [n_o[m]] are f32 row scales, ldsa and ldsb are ignored and may be NULL), PTD_Q_MXFP4 (ptd_lowrank_decode_w4)
 * or PTD_Q_MXFP6_E2M3 (ptd_lowrank_decode_w6): sa[m] [r[m], n_i / 32] and sb[m] [n_o[m], r[m] / 32] are e8m0 scale rows
 * with the pitches ldsa[m] and ldsb[m]; lda and ldb are in bytes.  Member m has its own output y[m] [T, n_o[m]] with row
 * pitch ldy[m] (the column blocks of one [T, sum n_o] tensor, or unrelated buffers); x, T, n_i and dtype are common.
 * Every y[m] holds the bits the format's own decode entry gives for that member alone: each member runs with the K
 * split, the grid and the kernel variant it would have there (ptd_lowrank_plan).  The argument arrays are read before
 * the call returns and not after it (the call may be captured in a graph).  Served when every member is served by the
 * format's decode entry with the common x, T, n_i and dtype; anything else, an unknown q_format and count outside
 * 1 .. PTD_LOWRANK_GROUP_MAX included, returns PTD_ERR_UNSUPPORTED before a kernel is launched.  Null pointers (bias, or
 * an entry of it, may be NULL), a leading dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a
 * short workspace PTD_ERR_WORKSPACE.  The workspace is the sum of the members' decode workspaces of that format. */
#define PTD_Q_FP8_E4M3 1
#define PTD_Q_MXFP4 2
#define PTD_Q_MXFP6_E2M3 3
size_t ptd_lowrank_decode_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r,
                                                  int dtype);
int ptd_lowrank_decode_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                               const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                               const int64_t* r,
                               const void* const* Bq, const int64_t* ldb, const void* const* sb, const int64_t* ldsb,
                               const int64_t* n_o,
                               const void* const* bias /* entries may be NULL; the array may be NULL */,
                               void* const* y, const int64_t* ldy,
                               void* ws, size_t ws_bytes, int dtype, void* stream);

/* The gated pair of a quantised, decomposed MLP at decode shapes, y = act(gate(x)) * up(x), gate and up pairs with
 * factors of one q_format (operands per member as in ptd_lowrank_decode_group_q; for fp8 ldsa_* and ldsb_* are ignored)
 * on the same x [T, n_i], in two launches on the caller's stream: both first products, then a kernel that forms both
 * second products row tile by row tile and applies the activation and the product in the lane that holds both sums.
 * With D the dtype: g = round_D(sb_g * acc_g + bias_g) (MX: no sb factor) and u likewise are the bits the format's decode
 * entry stores for gate and up, and y = round_D(round_D(act(g)) * u) -- the rounding points of the unfused act(g) * u,
 * act as in ptd_lowrank_decode_gated.  Served when both members are served by the format's decode entry with the common
 * x, T, n_i, n_ff and dtype and act is one of PTD_ACT_*; anything else, an unknown q_format included, returns
 * PTD_ERR_UNSUPPORTED before a kernel is launched.  Null pointers (either bias may be NULL), a leading dimension below
 * its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The workspace is the
 * sum of the two members' decode workspaces of that format. */
size_t ptd_lowrank_decode_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u,
                                                  int dtype);
int ptd_lowrank_decode_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i,
                               const void* Aq_g, int64_t lda_g, const void* sa_g, int64_t ldsa_g, int64_t r_g,
                               const void* Bq_g, int64_t ldb_g, const void* sb_g, int64_t ldsb_g, const void* bias_g,
                               const void* Aq_u, int64_t lda_u, const void* sa_u, int64_t ldsa_u, int64_t r_u,
                               const void* Bq_u, int64_t ldb_u, const void* sb_u, int64_t ldsb_u, const void* bias_u,
                               int64_t n_ff, int act, void* y, int64_t ldy,
                               void* ws, size_t ws_bytes, int dtype, void* stream);

/* The pair with OCP MXFP6 (e2m3) factors (arguments, formats and semantics of ptd_lowrank_decode_w6, clamp to
 * [116, 140] included: h and y from f32 sums, each rounded ONCE; no per-row scales) for 32 <= T <=
 * PTD_LOWRANK_SKINNY_W6_MAX_T tokens, with the structure of ptd_lowrank_skinny_w4 -- the same kernel template: three
 * launches on the caller's stream (first product into f32 slabs of a K split that depends on (n_i, r) alone, slab sum
 * into a 16-bit h, second product with the bias).  A lane's 12-byte load is half an MX block (16 six-bit codes),
 * converted to D in registers by one instruction that applies the clamped block scale; no dequantised copy is kept; row
 * t of y depends on row t of x alone, bit for bit, whatever T is.  Served: dtype bf16 / f16, w_format
 * PTD_W6_MXFP6_E2M3, 32 <= T <= PTD_LOWRANK_SKINNY_W6_MAX_T, r >= 32, n_i and r multiples of 32, lda and ldb multiples
 * of 8 bytes (lda >= 3 n_i / 4, ldb >= 3 r / 4), ldsa >= n_i / 32 and ldsb >= r / 32 (the scale rows need no alignment),
 * ldx a multiple of 8, x 16-byte aligned, Aq and Bq 8-byte aligned, bias 2-byte aligned and optional, n_i < 2^30,
 * r < 2^27, 1 <= n_o < 2^30.  Anything else returns PTD_ERR_UNSUPPORTED before a kernel is launched; null pointers, a
 * leading dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.
 * The workspace holds the slabs and h (the formula of ptd_lowrank_skinny_w4_workspace_bytes).  The cap is measured
 * (profiles/pair_skinny_w6.json).  No reference counterpart. */
#define PTD_LOWRANK_SKINNY_W6_MAX_T 96
size_t ptd_lowrank_skinny_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype);
int ptd_lowrank_skinny_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                          const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                          const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                          void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* An OCP MX factor written out as its 16-bit values: codes [rows, cols / 2] (MXFP4, ptd_lowrank_dequant_w4) or
 * [rows, 3 cols / 4] (MXFP6 e2m3, ptd_lowrank_dequant_w6) bytes with row pitch ldq, scales [rows, cols / 32] e8m0 bytes
 * with row pitch lds, out [rows, cols] elements of dtype D = bf16 or f16 with row pitch ldo (in elements):
 *   out[i, k] = W^[i, k] = val(code(W, i, k)) * 2^(clamp(scale[i, k >> 5], E_MIN, 140) - 127)
 * with code, val and the clamp (E_MIN = 114 / 116) of ptd_lowrank_decode_w4 / _w6.  EXACT: the clamp makes every W^ a
 * normal number (or zero) of bf16 and of f16, so nothing is rounded and out equals torch's dequantisation of the same
 * bytes bit for bit.  One launch on the caller's stream; a lane takes one MX block (its 16- or 24-byte code load, one
 * scale byte, the conversion instructions of the decode kernels, four 16-byte stores); nothing is written outside
 * [rows, cols] of out.  Null pointers, rows < 1, ldq below a row's code bytes, lds < cols / 32 or ldo < cols:
 * PTD_ERR_INVALID.  A dtype other than bf16 / f16, an unknown w_format, cols not a positive multiple of 32, code rows
 * that are not 8-byte aligned (address and ldq), output rows that are not 16-byte aligned (address, ldo a multiple of
 * 8), or more than 2^38 blocks: PTD_ERR_UNSUPPORTED before anything is launched.  No reference counterpart. */
int ptd_lowrank_dequant_w4(const void* codes, int64_t ldq, const void* scales, int64_t lds, int64_t rows, int64_t cols,
                           void* out, int64_t ldo, int dtype, int w_format, void* stream);
int ptd_lowrank_dequant_w6(const void* codes, int64_t ldq, const void* scales, int64_t lds, int64_t rows, int64_t cols,
                           void* out, int64_t ldo, int dtype, int w_format, void* stream);

/* The pair with OCP MX factors at ANY token count T >= 1 (arguments, formats and semantics of ptd_lowrank_skinny_w4 /
 * _w6, clamp included): ONE launch dequantises both factors into the workspace (the kernel of ptd_lowrank_dequant_w4 /
 * _w6, A's blocks and then B's in one grid; exact), then ptd_lowrank_forward runs on (x, A^, B^, bias) with the rest of
 * the workspace -- the 16-bit tile products, untouched.  The result is, bit for bit, what ptd_lowrank_forward returns
 * on the dequantised factors (contiguous, pitch = row length): f32 sums, h rounded ONCE to D, y once -- the rounding
 * points of the decode and skinny MX entries (the order of the f32 additions is the tile products', so the last bit may
 * differ from theirs).  No dequantised copy outlives the call.  Everything runs on the caller's stream without a host
 * read or an allocation: the call can be captured in a graph.  Served: the operands of ptd_lowrank_skinny_w4 / _w6 (dtype
 * bf16 / f16, r >= 32, n_i and r multiples of 32, lda and ldb multiples of 8 bytes, ldsa >= n_i / 32, ldsb >= r / 32,
 * ldx a multiple of 8, x 16-byte aligned, Aq and Bq 8-byte aligned, bias 2-byte aligned and optional, n_i < 2^30,
 * r < 2^27, 1 <= n_o < 2^30) at any T >= 1, at most 2^38 blocks in both factors.  Anything else returns
 * PTD_ERR_UNSUPPORTED before a kernel is launched; null pointers, a leading dimension below its row length or a
 * misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The workspace is
 *   align256(2 r n_i) + align256(2 n_o r) + ptd_lowrank_forward_workspace_bytes(T, n_i, r, dtype)
 * bytes: A^ [r, n_i], B^ [n_o, r], then the 16-bit entry's own (the query takes n_o for B^).  Which T the Python package
 * sends here is measured (profiles/pair_tile_mx.json).  No reference counterpart. */
size_t ptd_lowrank_tile_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype);
int ptd_lowrank_tile_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                        const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                        const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                        void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);
size_t ptd_lowrank_tile_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype);
int ptd_lowrank_tile_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                        const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                        const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                        void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* MXFP8 activations on the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4): OPT-IN entries beside the ones above,
 * because quantising the activations changes numerics.  D = bf16 / f16.
 *
 * Q8 of a row of n values of D, n a multiple of 32, per block of 32 consecutive elements with m = max |v_j|:
 *   s = clamp(floor(log2 m) - 8 + 127, 0, 254) (0 for an all-zero block), the e8m0 scale byte;
 *   code_j = e4m3fn (OCP), round to nearest even, of clamp(v_j 2^(127 - s), -448, 448); value_j = val(code_j) 2^(s - 127).
 * A block whose scaled maximum lies in (464, 512) saturates, as OCP MX specifies.  Finite inputs only: an Inf becomes
 * +-448 2^120 and a NaN -448 2^(s - 127), neither is propagated.
 *
 * ptd_mxfp8_quantize_rows: x [T, n] of D (pitch ldx elements) -> codes [T, n] bytes (pitch ldc) and scales [T, n / 32]
 * bytes (pitch lds), bit for bit Q8.  One launch, a lane per block.  Served: bf16 / f16, n a positive multiple of 32
 * below 2^30, x 16-byte aligned with ldx a multiple of 8, codes 16-byte aligned with ldc a multiple of 16, T <= 2^24 and
 * T n < 2^40; anything else PTD_ERR_UNSUPPORTED, null pointers / T < 1 / short pitches PTD_ERR_INVALID.
 *
 * ptd_mx_product_a8: out [T, N] (pitch ldo elements) = round_D(Xq^ W^^T + bias) in one launch, with Xq^ the values of
 * (xq [T, K] codes, ex [T, K / 32] scales) and W^ [N, K] the MXFP4 (q_format PTD_Q_MXFP4; Wq [N, K / 2]) or MXFP6 e2m3
 * (PTD_Q_MXFP6_E2M3; Wq [N, 3 K / 4]) factor of ptd_lowrank_decode_w4 / _w6, its scale bytes ew [N, K / 32] clamped to
 * [114, 140] / [116, 140] before they reach the instruction.  Sums in f32 across the K steps; inside a step the
 * instruction aligns its 128 products before it adds them and is coarser than an f32 sum (measured: up to 2^-15 of
 * sum |a b|; exact where the products share a grid),
 * one accumulator per output over the whole of K in ascending steps of 128: row t of out depends on row t of xq alone
 * and is the same bits at every T.  Served: bf16 / f16 (out and bias), K a positive multiple of 32 (not of 128: lanes
 * beyond K feed zero codes), any N >= 1 below 2^30, xq 16-byte aligned with ldxq a multiple of 16, Wq 8-byte aligned with
 * ldw a multiple of 8, bias 2-byte aligned and optional, T <= 2^24, T max(K, N) < 2^40.
 *
 * ptd_lowrank_a8_w4 / _w6 (arguments of ptd_lowrank_tile_w4 / _w6):
 *   h = round_D(Q8(x) A^^T)        y = round_D(Q8(h) B^^T + bias)
 * in four launches on the caller's stream -- quantise x, product, quantise h, product -- bit for bit the composition of
 * the two entries above.  The workspace holds Q8(x), h and Q8(h) (each part 256-aligned):
 *   align256(T n_i) + align256(T n_i / 32) + align256(2 T r) + align256(T r) + align256(T r / 32)
 * bytes; nothing outlives the call, no host read, no allocation: the call can be captured in a graph.  Served: the
 * operands of ptd_lowrank_tile_w4 / _w6 at 1 <= T <= 2^24 with T max(n_i, r, n_o) < 2^40.  Anything else, a wrong w_format
 * included, returns PTD_ERR_UNSUPPORTED before a kernel is launched; null pointers, a leading dimension below its row
 * length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  No reference counterpart. */
int ptd_mxfp8_quantize_rows(const void* x, int64_t ldx, int64_t T, int64_t n, void* codes, int64_t ldc, void* scales,
                            int64_t lds, int dtype, void* stream);
int ptd_mx_product_a8(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K,
                      const void* Wq, int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias,
                      void* out, int64_t ldo, int dtype, int q_format, void* stream);
size_t ptd_lowrank_a8_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype);
int ptd_lowrank_a8_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                      const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                      const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                      void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);
size_t ptd_lowrank_a8_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype);
int ptd_lowrank_a8_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                      const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                      const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                      void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* MXFP8 activations at prefill sizes: the same mathematics on an LDS-staged tiled GEMM.  OPT-IN, as the entries above.
 *
 * ptd_mx_product_a8_tile: ptd_mx_product_a8 with the mapping of a GEMM -- a workgroup of four waves owns a tile of BN
 * weight rows x BT tokens, (BN, BT) one of (128, 128), (64, 128), (64, 64), (32, 64): the first whose grid has 256
 * workgroups, else the last; the activation codes and scale bytes of a K step of 128 are staged in LDS (two buffers, the
 * next step's loads issued ahead of this step's MFMAs) and shared by the waves, the weights stream into registers.  One
 * accumulator per output over the whole of K in ascending steps of 128, no K split, blocks beyond K fed as zero codes
 * under scale byte 127, bias added in f32, one rounding: out is bit for bit ptd_mx_product_a8's at every shape and under
 * every tile shape, and row t does not depend on T.  With outq / eout (both or neither) the launch also stores
 * Q8(out): codes [T, N] bytes (pitch ldoq) and scale bytes [T, N / 32] (pitch ldeo), bit for bit
 * ptd_mxfp8_quantize_rows of out; out may then be null (the D values are not stored).  Served: what ptd_mx_product_a8
 * serves, with at least one of out and outq; outq needs N a multiple of 32, 16-byte alignment and ldoq a multiple of 16.
 * Anything else PTD_ERR_UNSUPPORTED; null operands, outq without eout, T < 1 or short pitches PTD_ERR_INVALID.
 *
 * ptd_lowrank_a8_tile_w4 / _w6 (arguments of ptd_lowrank_tile_w4 / _w6): the pair of ptd_lowrank_a8_w4 / _w6 in three
 * launches on the caller's stream -- quantise x, first product with the quantising epilogue (h leaves it as MXFP8 and
 * never exists in D), second product -- bit for bit ptd_lowrank_a8_w4 / _w6.  The workspace holds Q8(x) and Q8(h)
 * (each part 256-aligned):
 *   align256(T n_i) + align256(T n_i / 32) + align256(T r) + align256(T r / 32)
 * bytes.  Served and refused exactly as ptd_lowrank_a8_w4 / _w6 (every T >= 1 the grids index). */
int ptd_mx_product_a8_tile(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K,
                           const void* Wq, int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias,
                           void* out, int64_t ldo, void* outq, int64_t ldoq, void* eout, int64_t ldeo,
                           int dtype, int q_format, void* stream);
size_t ptd_lowrank_a8_tile_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype);
int ptd_lowrank_a8_tile_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                      const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                      const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                      void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);
size_t ptd_lowrank_a8_tile_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype);
int ptd_lowrank_a8_tile_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                      const void* Aq, int64_t lda, const void* scale_a, int64_t ldsa, int64_t r,
                      const void* Bq, int64_t ldb, const void* scale_b, int64_t ldsb, int64_t n_o, const void* bias,
                      void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format, void* stream);

/* The gated pair of a decomposed MLP at the same 32 <= T <= 96 tokens in bf16 / f16, y = act(gate(x)) * up(x) (arguments
 * and activations as ptd_lowrank_decode_gated), in three launches on the caller's stream: both first products, both
 * slab sums, then a kernel that forms both second products for the same 32 rows and 64 tokens and applies the activation
 * and the product in the lanes that hold both sums -- no [T, 2 n_ff] intermediate and no elementwise launch.  g and u
 * are the bits ptd_lowrank_skinny stores for gate and up (each member keeps its own K split, wave ranges and orders of
 * addition, so row t of y depends on row t of x alone); the activation is evaluated in f32 on g and rounded once, its
 * product with u is formed in f32 and rounded once -- the rounding points of the unfused act(g) * u.  Served when both
 * members are served by ptd_lowrank_skinny with the common x, T, n_i, n_ff and dtype and act is one of PTD_ACT_*;
 * anything else, f32 included, returns PTD_ERR_UNSUPPORTED before a kernel is launched.  Null pointers (either bias may
 * be NULL), a leading dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace
 * PTD_ERR_WORKSPACE.  The workspace is the sum of the two members' ptd_lowrank_skinny workspaces. */
size_t ptd_lowrank_skinny_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype);
int ptd_lowrank_skinny_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i,
                             const void* Ag, int64_t lda_g, int64_t r_g, const void* Bg, int64_t ldb_g, const void* bias_g,
                             const void* Au, int64_t lda_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* bias_u,
                             int64_t n_ff, int act, void* y, int64_t ldy,
                             void* ws, size_t ws_bytes, int dtype, void* stream);

/* 1 <= count <= PTD_LOWRANK_GROUP_MAX pairs with quantised factors of ONE format that read the same x at small batches,
 * 32 <= T <= the format's PTD_LOWRANK_SKINNY_W8_MAX_T / _W4_MAX_T / _W6_MAX_T (arguments of ptd_lowrank_decode_group_q;
 * operands and semantics per member those of ptd_lowrank_skinny_w8 / _w4 / _w6), in THREE launches on the caller's stream
 * instead of three per pair: every member's first product into its own f32 slabs (the members' grids laid end to end,
 * the token tile in the grid's z), every member's slab sum into its own 16-bit h (fp8: with sa), every member's second
 * product into its own y[m] with row pitch ldy[m].  Each member keeps the K split, the slab order, the wave quarters, the
 * step order, the scale-byte variant and the rounding points of its format's skinny entry, so every y[m] holds the bits
 * that entry gives for the member alone and row t of y depends on row t of x alone.  No floating-point atomics; one
 * writer per output element.  The argument arrays are read before the call returns and not after it (the call may be
 * captured in a graph).  Served when every member is served by the format's skinny entry with the common x, T, n_i and
 * dtype (bf16 / f16); anything else, an unknown q_format and count outside 1 .. PTD_LOWRANK_GROUP_MAX included, returns
 * PTD_ERR_UNSUPPORTED before a kernel is launched.  Null pointers (bias, or an entry of it, may be NULL), a leading
 * dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short workspace PTD_ERR_WORKSPACE.  The
 * workspace is the sum of the members' skinny workspaces of that format (each a multiple of 256 bytes: member m's region
 * starts where member m - 1's ends).  No reference counterpart. */
size_t ptd_lowrank_skinny_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r,
                                                  int dtype);
int ptd_lowrank_skinny_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                               const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                               const int64_t* r,
                               const void* const* Bq, const int64_t* ldb, const void* const* sb, const int64_t* ldsb,
                               const int64_t* n_o,
                               const void* const* bias /* entries may be NULL; the array may be NULL */,
                               void* const* y, const int64_t* ldy,
                               void* ws, size_t ws_bytes, int dtype, void* stream);

/* The gated pair of a quantised, decomposed MLP at the same token counts, y = act(gate(x)) * up(x) (arguments of
 * ptd_lowrank_decode_gated_q), in THREE launches on the caller's stream: the first two launches of
 * ptd_lowrank_skinny_group_q on (gate, up), then a kernel in which a workgroup forms both second products for the same
 * 32 rows and 64 tokens -- gate's loop and its wave sums, then up's -- and applies the activation and the product in the
 * lanes that hold both sums: no [T, 2 n_ff] intermediate and no elementwise launch.  With D the dtype:
 * g = round_D(sb_g * acc_g + bias_g) (MX: no sb factor) and u likewise are the bits the format's skinny entry stores for
 * gate and up, and y = round_D(round_D(act(g)) * u), act as in ptd_lowrank_decode_gated.  Served when both members are
 * served by the format's skinny entry with the common x, T, n_i, n_ff and dtype and act is one of PTD_ACT_*; anything
 * else, an unknown q_format included, returns PTD_ERR_UNSUPPORTED before a kernel is launched.  Null pointers (either
 * bias may be NULL), a leading dimension below its row length or a misaligned workspace PTD_ERR_INVALID; a short
 * workspace PTD_ERR_WORKSPACE.  The workspace is the sum of the two members' skinny workspaces of that format.  No
 * reference counterpart. */
size_t ptd_lowrank_skinny_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u,
                                                  int dtype);
int ptd_lowrank_skinny_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i,
                               const void* Aq_g, int64_t lda_g, const void* sa_g, int64_t ldsa_g, int64_t r_g,
                               const void* Bq_g, int64_t ldb_g, const void* sb_g, int64_t ldsb_g, const void* bias_g,
                               const void* Aq_u, int64_t lda_u, const void* sa_u, int64_t ldsa_u, int64_t r_u,
                               const void* Bq_u, int64_t ldb_u, const void* sb_u, int64_t ldsb_u, const void* bias_u,
                               int64_t n_ff, int act, void* y, int64_t ldy,
                               void* ws, size_t ws_bytes, int dtype, void* stream);

/* Host query for tests and tools: the numbers a launch of one serving family of the pair would use for (T, n_i, r, n_o,
 * dtype) with contiguous, aligned operands -- computed by the functions the launchers and kernels themselves call, so a
 * test can prove which branch combination a shape reaches.  family: PTD_PLAN_DECODE (ptd_lowrank_decode; every member
 * of ptd_lowrank_decode_group and both members of ptd_lowrank_decode_gated take the plan of that member alone),
 * PTD_PLAN_DECODE_W8, PTD_PLAN_DECODE_W4 (every member of ptd_lowrank_decode_group_q and both members of
 * ptd_lowrank_decode_gated_q take the plan of PTD_PLAN_DECODE_W8 / _W4 / _W6 for that member alone, the kernel variants
 * xa_u and hb_u included), PTD_PLAN_SKINNY (ptd_lowrank_skinny; both members of
 * ptd_lowrank_skinny_gated take the plan of that member alone), PTD_PLAN_SKINNY_W8, PTD_PLAN_SKINNY_W4 (xa_u and hb_u:
 * the scale bytes of one load, 1 or 2; the tail fields: blocks of a row % that -- non-zero: the last block's scale byte
 * comes out of the clamped, shifted load), PTD_PLAN_DECODE_W6 (ptd_lowrank_decode_w6: every field with the meaning
 * PTD_PLAN_DECODE_W4 gives it, "MXFP4" below read as "MXFP4 and MXFP6"), PTD_PLAN_SKINNY_W6 (ptd_lowrank_skinny_w6: every
 * field with the meaning PTD_PLAN_SKINNY_W4 gives it -- the two share one kernel template; every member of
 * ptd_lowrank_skinny_group_q and both members of ptd_lowrank_skinny_gated_q take the plan of PTD_PLAN_SKINNY_W8 / _W4 /
 * _W6 for that member alone, xa_u and hb_u included).  Writes out[PTD_PLAN_*] for the
 * PTD_PLAN_LEN indices below and returns PTD_PLAN_LEN; PTD_ERR_UNSUPPORTED where the family does not serve the shape or
 * the family is unknown, PTD_ERR_INVALID for a null `out` or cap < PTD_PLAN_LEN.  "First product" is x A^T into K slabs,
 * "second" h B^T.  A wave's "load step" is the k its 64 lanes cover with one 16-byte load each (32 for bf16 / f16, 16 for
 * f32, 64 for fp8 and the skinny kernels, 128 for MXFP4).  No device code, no launch, no allocation: works without a
 * GPU.  No reference counterpart. */
#define PTD_PLAN_DECODE 0
#define PTD_PLAN_DECODE_W8 1
#define PTD_PLAN_DECODE_W4 2
#define PTD_PLAN_SKINNY 3
#define PTD_PLAN_SKINNY_W8 4
#define PTD_PLAN_SKINNY_W4 5
#define PTD_PLAN_DECODE_W6 6
#define PTD_PLAN_SKINNY_W6 7
#define PTD_PLAN_NSLABS 0             /* K slabs of the first product */
#define PTD_PLAN_KCHUNK 1             /* k of one slab (four wave ranges of kchunk / 4) */
#define PTD_PLAN_XA_GRID_X 2          /* first product: row tiles, */
#define PTD_PLAN_XA_GRID_Y 3          /*   slabs, */
#define PTD_PLAN_XA_GRID_Z 4          /*   token tiles (1 at decode) */
#define PTD_PLAN_XA_EMPTY_WAVES 5     /* of the LAST slab's four waves, those whose K range is empty */
#define PTD_PLAN_XA_TAIL_IN_STEP 6    /* 1: the last non-empty wave's range ends inside a load step */
#define PTD_PLAN_XA_U 7               /* first product's kernel variant: loads in flight per lane (MXFP4: blocks per lane, U) */
#define PTD_PLAN_XA_TAIL_BLOCKS 8     /* MXFP4: (n_i / 32) % U -- non-zero: a valid block's scale byte is a shifted one; else 0 */
#define PTD_PLAN_HB_GRID 9            /* second product: workgroups (skinny: row tiles of 32) */
#define PTD_PLAN_HB_NCHUNKS 10        /* decode: LDS chunks of h per tile (skinny: 1) */
#define PTD_PLAN_HB_CHUNK_K 11        /* k of a full chunk (a wave takes a quarter) */
#define PTD_PLAN_HB_LAST_CHUNK_K 12   /* k of the last chunk */
#define PTD_PLAN_HB_TILES_MAX 13      /* decode: tiles of 16 rows per workgroup, the most */
#define PTD_PLAN_HB_TILES_MIN 14      /*   and the fewest (workgroup b takes tiles b, b + grid, ...); skinny: 1 and 1 */
#define PTD_PLAN_HB_LAST_TILE_ROWS 15 /* rows of n_o in the last row tile (16 at decode, 32 skinny, when it is full) */
#define PTD_PLAN_HB_U 16              /* second product's variant: loads per lane and chunk (MXFP4: blocks per lane, U) */
#define PTD_PLAN_HB_TAIL_BLOCKS 17    /* MXFP4: (r / 32) % U; else 0 */
#define PTD_PLAN_COMBINE_GRID 18      /* skinny: workgroups of the slab sum (decode: 0, the second product sums the slabs) */
#define PTD_PLAN_TOKEN_TILES 19       /* skinny: tiles of 64 tokens (decode: 1) */
#define PTD_PLAN_SLABS_ASKED 20      /* the slab count the rank asks for: what the split gives a row of 2^20 k (nslabs is
                                      * smaller where n_i is too short to be cut that often) */
#define PTD_PLAN_LEN 21
int ptd_lowrank_plan(int family, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int32_t* out, int cap);

/* The same pair for a 1x1-convolution input in NCHW layout, without the NHWC copy the reference makes
 * (`permute(0,2,3,1).reshape(-1,C)`, dwain.py:116; falor.py:126): per image b, x_b = x + b*n_i*hw is an
 * [n_i, hw] matrix with the hw = H*W pixels contiguous; h_b[r,hw] = A x_b, y_b[n_o,hw] = B h_b + bias[:,None],
 * y written straight into NCHW (contiguous [batch, n_o, hw]).  The workspace holds h.  Replaces the two
 * nn.Conv2d(kernel_size=1) of dwain.py:126-144 / falor.py:136-153. */
size_t ptd_lowrank_forward_nchw_workspace_bytes(int64_t batch, int64_t hw, int64_t r, int dtype);
int ptd_lowrank_forward_nchw(const void* x, int64_t batch, int64_t n_i, int64_t hw, const void* A, int64_t lda,
                             int64_t r, const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y,
                             void* ws, size_t ws_bytes, int dtype, void* stream);

/* ---- rank-selection metrics ------------------------------------------------ */

/* out[0] (f64) = mean_c( mean_r (x-y)^2 / (var_r(y) + eps) ), x,y (f32, f64, bf16 or f16) viewed as [R, C],
 * var unbiased.  Replaces calc_per_channel_noise_to_signal_ratio (losses.py:10-22)
 * for non_channel_dim = all leading dims. */
/* (ABI 2) The workspace carries the arrival counters of the one-launch reduction: initialise it ONCE with
 * ptd_nsr_workspace_init (any size >= the query for the shapes it will serve); ptd_nsr leaves it initialised, so the
 * same workspace serves any number of stream-ordered calls.  Calls that may overlap need a workspace each.
 * One row (R = 1) gives NaN, as torch.std of one sample does.  A NaN anywhere in x or y, or an infinity in y, gives NaN, and an
 * infinity in x alone gives +inf, both as the reference does; the workspace is left initialised all the same, so the
 * next call on it is right.
 * Launch labels (ptd_launch_trace_*): "nsr (16-byte loads)" when the partial sums are formed with 16-byte loads,
 * "nsr (one element per lane)" otherwise. */
size_t ptd_nsr_workspace_bytes(int64_t R, int64_t C);
/* Host diagnostic for tests, no device code and no GPU needed: what ptd_nsr would launch for x, y [R, C] of `dtype`,
 * computed by the functions ptd_nsr itself calls.  `aligned`: non-zero when x and y both lie on 16-byte boundaries.
 * The 16-byte form serves f32 (4 channels a lane) and bf16 / f16 (8 channels a lane) when C >= 64, C is a multiple of
 * the lane's channels and both operands are aligned; everything else, f64 included, takes the one-element-per-lane
 * form.  Writes PTD_NSR_PLAN_LEN values to out (cap = the room in out) and returns PTD_NSR_PLAN_LEN;
 * PTD_ERR_INVALID for a null out, a cap too small or R, C < 1, PTD_ERR_UNSUPPORTED for an unknown dtype.  The chunk
 * count of the 16-byte form honours the environment variable PTD_NSR_BLOCKS, read once per process. */
#define PTD_NSR_PLAN_VEC 0             /* channels a lane loads at once: 4 or 8 in the 16-byte form, 0 otherwise */
#define PTD_NSR_PLAN_CT 1              /* channels of a column tile (one workgroup): 64 lanes of vec channels, or Ct lanes */
#define PTD_NSR_PLAN_RT 2              /* row lanes of a workgroup: (lanes of a tile) * Rt <= 256 threads work */
#define PTD_NSR_PLAN_COLTILES 3        /* grid x of the partial kernel */
#define PTD_NSR_PLAN_NCHUNK 4          /* grid y of the partial kernel: row chunks, none of them empty */
#define PTD_NSR_PLAN_ROWS_PER_CHUNK 5  /* rows of every chunk but the last (clamped to INT32_MAX) */
#define PTD_NSR_PLAN_FINAL_BLOCKS 6    /* workgroups of the final kernel: ceil(C / 64) */
#define PTD_NSR_PLAN_LEN 7
int ptd_nsr_plan(int64_t R, int64_t C, int dtype, int aligned, int32_t* out, int cap);
int ptd_nsr_workspace_init(void* ws, size_t ws_bytes, void* stream);
int ptd_nsr(const void* x, const void* y, int64_t R, int64_t C, int dtype, double eps, double* out,
            void* ws, size_t ws_bytes, void* stream);

/* out[0] (f64) = mean_b max(KL(t_b || s_b), KL(s_b || t_b)) over softmax(dim=-1) of
 * logits s, t [B, C] (f32, bf16 or f16).  Replaces calc_kl_loss (losses.py:48-63).
 * Computed from log-probabilities (row maximum subtracted, log-sum-exp in f64): finite logits give a finite result,
 * also where the reference program forms softmax first, lets a probability underflow to 0 and returns NaN.  A row that
 * holds a NaN or an infinite logit is NaN and makes out[0] NaN. */
size_t ptd_sym_kl_workspace_bytes(int64_t B);
int ptd_sym_kl(const void* s, const void* t, int64_t B, int64_t C, int dtype, double* out, void* ws,
               size_t ws_bytes, void* stream);

/* rows[b] (f64) = KL(p_b || q_b) = sum_c p log(p / q) over softmax(dim=-1) of logits q, p [B, C].
 * f32, bf16 or f16.  Replaces calc_kl_divergence(q_logits, p_logits) (losses.py:48-54).
 * Finite logits give a finite row where the reference program underflows to NaN (see ptd_sym_kl).  A row that holds a
 * NaN or an infinite logit is NaN; it stays in its own row: every other row of the call is bit for bit what it is
 * without it. */
int ptd_kl_rows(const void* q, const void* p, int64_t B, int64_t C, int dtype, double* rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTDECO_HIP_H */
