// extern "C" surface of libptdeco_hip.so (declared in include/ptdeco_hip.h).
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "kernels.h"

namespace ptd {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

__thread LaunchTrace g_launch_trace = {false, 0, {nullptr}};

}  // namespace ptd

using namespace ptd;

// one wave that holds its hardware queue for `ticks` of the 100 MHz wall clock (ptd_streams_wall_us: do streams overlap?)
__global__ void stream_spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

extern "C" {

int ptd_version(void) { return PTD_ABI_VERSION; }

const char* ptd_last_error(void) { return g_err; }

void ptd_launch_trace_begin(void) {
  g_launch_trace.count = 0;
  g_launch_trace.on = true;
}

int ptd_launch_trace_end(char* buf, size_t cap) {
  LaunchTrace& t = g_launch_trace;
  const int count = t.on ? t.count : 0;
  t.on = false;
  t.count = 0;
  if (buf && cap) {
    size_t pos = 0;
    for (int i = 0; i < std::min(count, 32); ++i) {
      if (i && pos + 1 < cap) buf[pos++] = '\n';
      for (const char* s = t.what[i]; *s && pos + 1 < cap; ++s) buf[pos++] = *s;
    }
    buf[pos] = '\0';
  }
  return count;
}

int ptd_set_concurrent_chains(int chains) { return concurrent_chains_exchange(chains < 1 ? 1 : chains); }

int ptd_streams_wall_us(void* const* streams, int count, int spin_us, double* wall_us) {
  PTD_REQUIRE(streams && wall_us && count >= 1 && count <= 64 && spin_us >= 1 && spin_us <= 100000,
              "ptd_streams_wall_us: bad argument");
  for (int i = 0; i < count; ++i) PTD_CHECK_HIP(hipStreamSynchronize(static_cast<hipStream_t>(streams[i])));
  const long long ticks = (long long)spin_us * 100;
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < count; ++i)
    hipLaunchKernelGGL(stream_spin_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(streams[i]), ticks);
  for (int i = 0; i < count; ++i) PTD_CHECK_HIP(hipStreamSynchronize(static_cast<hipStream_t>(streams[i])));
  *wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  PTD_CHECK_LAUNCH("ptd_streams_wall_us");
  return PTD_OK;
}

int ptd_stream_create_dedicated(int cu_first, int cu_count, void** stream_out) {
  PTD_REQUIRE(stream_out && cu_first >= 0 && cu_count >= 0, "ptd_stream_create_dedicated: bad argument");
  int dev = 0, cus = 0;
  PTD_CHECK_HIP(hipGetDevice(&dev));
  PTD_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (cu_count == 0) { cu_first = 0; cu_count = cus; }
  PTD_REQUIRE(cu_first + cu_count <= cus, "ptd_stream_create_dedicated: CUs [%d, %d) of %d", cu_first, cu_first + cu_count, cus);
  uint32_t mask[32] = {0};
  for (int c = cu_first; c < cu_first + cu_count && c < 1024; ++c) mask[c >> 5] |= 1u << (c & 31);
  hipStream_t st = nullptr;
  PTD_CHECK_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)((cus + 31) / 32), mask));
  *stream_out = st;
  return PTD_OK;
}

int ptd_stream_destroy(void* stream) {
  PTD_CHECK_HIP(hipStreamDestroy(static_cast<hipStream_t>(stream)));
  return PTD_OK;
}

int ptd_syrk_accumulate(const void* y, int64_t T, int64_t n, int64_t ldy, int y_dtype, void* E, int64_t ldE,
                        int E_dtype, double scale, void* stream) {
  PTD_REQUIRE(y && E, "ptd_syrk_accumulate: null pointer");
  PTD_REQUIRE(T >= 0 && n >= 0 && ldy >= n && ldE >= n, "ptd_syrk_accumulate: bad shape T=%lld n=%lld ldy=%lld ldE=%lld",
              (long long)T, (long long)n, (long long)ldy, (long long)ldE);
  PTD_REQUIRE(E_dtype == PTD_F64 || E_dtype == PTD_F32, "ptd_syrk_accumulate: E must be f64 or f32");
  PTD_REQUIRE(T < (1ll << 31) && n < (1ll << 31), "ptd_syrk_accumulate: dimension too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (y_dtype == PTD_F32)
    return syrk_f32(static_cast<const float*>(y), T, n, ldy, E, ldE, E_dtype == PTD_F64, scale, st);
  if (y_dtype == PTD_BF16)
    return syrk_bf16(static_cast<const unsigned short*>(y), T, n, ldy, E, ldE, E_dtype == PTD_F64, scale, st);
  if (y_dtype == PTD_F16)
    return syrk_f16(static_cast<const unsigned short*>(y), T, n, ldy, E, ldE, E_dtype == PTD_F64, scale, st);
  set_error("ptd_syrk_accumulate: y dtype must be f32, bf16 or f16");
  return PTD_ERR_UNSUPPORTED;
}

int ptd_syrk_accumulate_multi(const void* const* ys, int steps, int64_t T, int64_t n, int64_t ldy, int y_dtype, void* E,
                              int64_t ldE, int E_dtype, double scale, void* stream) {
  PTD_REQUIRE(ys && E && steps >= 0 && steps <= 4096, "ptd_syrk_accumulate_multi: bad argument");
  for (int s = 0; s < steps; ++s) PTD_REQUIRE(ys[s], "ptd_syrk_accumulate_multi: null pointer (step %d)", s);
  PTD_REQUIRE(T >= 0 && n >= 0 && ldy >= n && ldE >= n, "ptd_syrk_accumulate_multi: bad shape T=%lld n=%lld ldy=%lld ldE=%lld",
              (long long)T, (long long)n, (long long)ldy, (long long)ldE);
  PTD_REQUIRE(E_dtype == PTD_F64 || E_dtype == PTD_F32, "ptd_syrk_accumulate_multi: E must be f64 or f32");
  PTD_REQUIRE(T < (1ll << 31) && n < (1ll << 31), "ptd_syrk_accumulate_multi: dimension too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (y_dtype == PTD_BF16)
    return syrk_bf16_multi(reinterpret_cast<const unsigned short* const*>(ys), steps, T, n, ldy, E, ldE,
                           E_dtype == PTD_F64, scale, st);
  if (y_dtype == PTD_F16)
    return syrk_f16_multi(reinterpret_cast<const unsigned short* const*>(ys), steps, T, n, ldy, E, ldE,
                          E_dtype == PTD_F64, scale, st);
  if (y_dtype == PTD_F32) {
    // the f32 product is bound by the matrix cores, not by the accumulator's read-modify-write: step by step
    for (int s = 0; s < steps; ++s) {
      const int rc = syrk_f32(static_cast<const float*>(ys[s]), T, n, ldy, E, ldE, E_dtype == PTD_F64, scale, st);
      if (rc != PTD_OK) return rc;
    }
    return PTD_OK;
  }
  set_error("ptd_syrk_accumulate_multi: y dtype must be f32, bf16 or f16");
  return PTD_ERR_UNSUPPORTED;
}

int ptd_colsum_accumulate(const void* y, int64_t T, int64_t n, int64_t ldy, int y_dtype, void* ey, int ey_dtype,
                          double scale, void* stream) {
  return colsum_accumulate(y, T, n, ldy, y_dtype, ey, ey_dtype, scale, static_cast<hipStream_t>(stream));
}

size_t ptd_cov_finalize_workspace_bytes(int64_t n) { return cov_finalize_workspace_bytes(n); }

int ptd_cov_finalize(const void* E, int64_t ldE, int E_dtype, const void* ey, int ey_dtype, int64_t n, double steps,
                     double damp_factor, double* C, int64_t ldC, void* ws, size_t ws_bytes, void* stream) {
  return cov_finalize(E, ldE, E_dtype, ey, ey_dtype, n, steps, damp_factor, C, ldC, ws, ws_bytes,
                      static_cast<hipStream_t>(stream));
}

// Solver choice (see include/ptdeco_hip.h).  Read on every call so a process can switch.
static int eigh_method() {
  const char* e = getenv("PTD_EIGH_METHOD");
  if (!e || !strcmp(e, "auto")) return 2;
  if (!strcmp(e, "tridiag")) return 1;
  return 0;
}

size_t ptd_eigh_workspace_bytes(int64_t n) {
  return std::max(std::max(eigh_workspace_bytes(n), tridiag_workspace_bytes(n)), eigh_filtered_workspace_bytes(n));
}

static int eigh_dispatch(const double* A, int64_t lda, int64_t n, int64_t k, double* evals, double* evecs,
                         int64_t ldv, void* ws, size_t ws_bytes, int* sweeps_out, bool all_values,
                         ptd_eigh_stats* stats, hipStream_t st, bool direct = false) {
  const int method = direct && eigh_method() == 2 ? 1 : eigh_method();
  // a quarter of the spectrum of a large matrix: filtered subspace iteration on the f64 matrix cores; it declines
  // (flat spectrum, breakdown, residual above tolerance) with PTD_ERR_UNSUPPORTED and the direct route below runs
  if (method == 2 && A && evals && evecs && ws && lda >= n && k >= 1 && k <= n && ldv >= k && (lda % 2) == 0 &&
      (reinterpret_cast<uintptr_t>(A) & 15) == 0 &&
      eigh_filtered_applies(n, k, all_values) && ws_bytes >= eigh_filtered_workspace_bytes(n, k) &&
      !eigh_filtered_backed_off(n, k)) {
    const int rc = eigh_filtered(A, lda, n, k, evals, evecs, ldv, ws, ws_bytes, stats, st);
    if (rc != PTD_ERR_UNSUPPORTED && rc != PTD_ERR_WORKSPACE) {
      if (sweeps_out) *sweeps_out = 0;
      return rc;
    }
  }
  if (method != 0 && (method == 1 || n >= 256) && A && evals && evecs && ws && n >= 2 && lda >= n && k >= 1 &&
      k <= n && ldv >= k) {
    const char* ct = getenv("PTD_EIGH_CLUSTER_TOL");
    const int rc = eigh_tridiag(A, lda, n, k, evals, evecs, ldv, ws, ws_bytes, ct ? atof(ct) : 1e-10, all_values, stats, st);
    if (rc != PTD_ERR_UNSUPPORTED) {
      if (sweeps_out) *sweeps_out = 0;
      return rc;
    }
  }
  return eigh_jacobi(A, lda, n, k, evals, evecs, ldv, ws, ws_bytes, sweeps_out, stats, st);
}

void ptd_eigh_forget_declines(void) { eigh_filtered_forget_declines(); }

int ptd_eigh_route(int64_t n, int64_t k, int all_values) {
  // what eigh_dispatch would try first for this request (the filtered route may still decline at run time)
  const int method = eigh_method();
  if (method == 2 && eigh_filtered_applies(n, k, all_values != 0)) return 3;
  if (method != 0 && (method == 1 || n >= 256) && n >= 2) return 1;
  return 0;
}

// ---- several matrices of one order in one call
// count == 2 matrices are batched from this order on (two matrices of order 1024 take 8.3 ms either way -- a shared
// blocked column of ~8 us against two resident ones of ~4 -- but the batched pair keeps that time beside another
// stream's work, where single calls lose their resident kernels: 9 ms each); count >= 3: always
static int batch_min_n() {
  const char* e = getenv("PTD_EIGH_BATCH_MIN_N");
  return e ? atoi(e) : 512;
}

static bool batch_route(int count, int64_t n, int64_t k, bool all_values, bool direct = false) {
  const int method = eigh_method();
  if (count < 2 || method == 0 || n < 256) return false;
  // (the filtered route's f64 products fill the chip: one by one -- unless the caller asks for the direct reduction)
  if (!direct && method == 2 && eigh_filtered_applies(n, k, all_values)) return false;
  return count >= 3 || n >= batch_min_n();
}

size_t ptd_eigh_batched_workspace_bytes(int64_t n, int64_t k, int count) {
  (void)k;
  return std::max(ptd_eigh_workspace_bytes(n), tridiag_batched_workspace_bytes(n, count));
}

int ptd_eigh_topk_batched(const double* const* As, int64_t lda, int count, int64_t n, int64_t k, int all_values,
                          double* const* evals, double* const* evecs, int64_t ldv, void* ws, size_t ws_bytes,
                          ptd_eigh_stats* stats, void* stream) {
  PTD_REQUIRE(As && evals && evecs && ws && count >= 1 && count <= 64 && n >= 1 && lda >= n && k >= 1 && k <= n && ldv >= k,
              "ptd_eigh_topk_batched: bad argument");
  for (int b = 0; b < count; ++b)
    PTD_REQUIRE(As[b] && evals[b] && evecs[b], "ptd_eigh_topk_batched: null pointer (matrix %d)", b);
  if (ws_bytes < ptd_eigh_batched_workspace_bytes(n, k, count)) {
    set_error("ptd_eigh_topk_batched: workspace %zu < required %zu bytes", ws_bytes,
              ptd_eigh_batched_workspace_bytes(n, k, count));
    return PTD_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (stats) memset(stats, 0, sizeof(*stats));
  // all_values is a set of flags: bit 0 = every eigenvalue, bit 1 (PTD_EIGH_FLAG_DIRECT) = the direct reduction also
  // where the filtered route would serve the request (a caller whose pass already runs latency-bound reductions of
  // this order beside this call: the filter's products would share the matrix cores with them)
  const bool direct = (all_values & 2) != 0;
  all_values &= 1;
  if (!batch_route(count, n, k, all_values != 0, direct)) {
    // one by one, each with the whole chip (the filtered route's products fill it; a single direct reduction keeps
    // its resident kernels); stats describe the LAST matrix
    for (int b = 0; b < count; ++b) {
      const int rc = eigh_dispatch(As[b], lda, n, k, evals[b], evecs[b], ldv, ws, ws_bytes, nullptr, all_values != 0,
                                   stats, st, direct);
      if (rc != PTD_OK) return rc;
    }
    return PTD_OK;
  }
  int rcs[64];
  const char* ct = getenv("PTD_EIGH_CLUSTER_TOL");
  int rc = eigh_tridiag_batched(As, lda, count, n, k, evals, evecs, ldv, ws, ws_bytes, ct ? atof(ct) : 1e-10,
                                all_values != 0, rcs, stats, st);
  if (rc != PTD_OK) return rc;
  for (int b = 0; b < count; ++b)
    if (rcs[b] == PTD_ERR_UNSUPPORTED) {     // clustered beyond what the tridiagonal route serves: Jacobi needs no gap
      rc = eigh_jacobi(As[b], lda, n, k, evals[b], evecs[b], ldv, ws, ws_bytes, nullptr, nullptr, st);
      if (rc != PTD_OK) return rc;
    }
  return PTD_OK;
}

size_t ptd_eigh_factored_workspace_bytes(int64_t n_o, int64_t n_i, int64_t k) {
  return eigh_factored_workspace_bytes(n_o, n_i, k);
}

int ptd_eigh_factored_prepare(const void* W, int64_t ldw, int w_dtype, int64_t n_o, int64_t n_i, const double* Ex,
                              int64_t ldx, int64_t k, void* ws, size_t ws_bytes, double** B_out, int64_t* np_out,
                              void* stream) {
  return eigh_factored_prepare(W, ldw, w_dtype, n_o, n_i, Ex, ldx, k, ws, ws_bytes, B_out, np_out,
                               static_cast<hipStream_t>(stream));
}

int ptd_eigh_factored_finish(int64_t n_o, int64_t n_i, int64_t k, const double* evals, const double* S, int64_t lds,
                             double* evals_k, double* U, int64_t ldu, void* ws, size_t ws_bytes, void* stream) {
  return eigh_factored_finish(n_o, n_i, k, evals, S, lds, evals_k, U, ldu, ws, ws_bytes,
                              static_cast<hipStream_t>(stream));
}

int ptd_eigh_factored(const void* W, int64_t ldw, int w_dtype, int64_t n_o, int64_t n_i, const double* Ex,
                      int64_t ldx, int64_t k, double* evals_k, double* U, int64_t ldu, void* ws, size_t ws_bytes,
                      void* stream) {
  return eigh_factored(W, ldw, w_dtype, n_o, n_i, Ex, ldx, k, evals_k, U, ldu, ws, ws_bytes,
                       static_cast<hipStream_t>(stream));
}

int ptd_eigh(const double* A, int64_t lda, int64_t n, double* evals, double* evecs, int64_t ldv, void* ws,
             size_t ws_bytes, int* sweeps_out, void* stream) {
  return eigh_dispatch(A, lda, n, n, evals, evecs, ldv, ws, ws_bytes, sweeps_out, true, nullptr,
                       static_cast<hipStream_t>(stream));
}

int ptd_eigh_topk(const double* A, int64_t lda, int64_t n, int64_t k, int all_values, double* evals, double* evecs,
                  int64_t ldv, void* ws, size_t ws_bytes, int* sweeps_out, void* stream) {
  return eigh_dispatch(A, lda, n, k, evals, evecs, ldv, ws, ws_bytes, sweeps_out, all_values != 0, nullptr,
                       static_cast<hipStream_t>(stream));
}

// The f32 face of ptd_eigh_topk (decompose_in_float64=False runs torch.linalg.eigh on an f32 matrix, dwain.py:224-233 +
// 162): f32 in, f32 out, the arithmetic in between in f64 -- the routes above on a converted copy -- so the result is
// the f32 rounding of the f64 eigenpairs of the f32 matrix (at least as accurate as an f32 LAPACK call).
size_t ptd_eigh_f32_workspace_bytes(int64_t n, int64_t k) {
  if (n < 1) return 0;
  k = std::max<int64_t>(1, std::min(k, n));
  return align_up((size_t)n * n * 8, 256) + align_up((size_t)n * 8, 256) + align_up((size_t)n * k * 8, 256) +
         ptd_eigh_workspace_bytes(n);
}

int ptd_eigh_topk_f32(const float* A, int64_t lda, int64_t n, int64_t k, int all_values, float* evals, float* evecs,
                      int64_t ldv, void* ws, size_t ws_bytes, int* sweeps_out, void* stream) {
  PTD_REQUIRE(A && evals && evecs && ws && n >= 1 && lda >= n && k >= 1 && k <= n && ldv >= k,
              "ptd_eigh_topk_f32: bad argument");
  if (ws_bytes < ptd_eigh_f32_workspace_bytes(n, k)) {
    set_error("ptd_eigh_topk_f32: workspace %zu < required %zu bytes", ws_bytes, ptd_eigh_f32_workspace_bytes(n, k));
    return PTD_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  double* A64 = reinterpret_cast<double*>(base);
  double* w64 = reinterpret_cast<double*>(base + align_up((size_t)n * n * 8, 256));
  double* v64 = reinterpret_cast<double*>(base + align_up((size_t)n * n * 8, 256) + align_up((size_t)n * 8, 256));
  char* rest = base + align_up((size_t)n * n * 8, 256) + align_up((size_t)n * 8, 256) + align_up((size_t)n * k * 8, 256);
  int rc = convert_f32_to_f64(A, lda, A64, n, n, n, st);
  if (rc != PTD_OK) return rc;
  rc = eigh_dispatch(A64, n, n, k, w64, v64, k, rest, ws_bytes - (size_t)(rest - base), sweeps_out, all_values != 0, nullptr, st);
  if (rc != PTD_OK) return rc;
  rc = convert_f64_to_f32(w64, n, evals, n, 1, n, st);      // (NaN where the route did not compute an eigenvalue stays NaN)
  if (rc != PTD_OK) return rc;
  return convert_f64_to_f32(v64, k, evecs, ldv, n, k, st);
}

int ptd_eigh_profiled(const double* A, int64_t lda, int64_t n, int64_t k, int all_values, double* evals,
                      double* evecs, int64_t ldv, void* ws, size_t ws_bytes, ptd_eigh_stats* stats, void* stream) {
  PTD_REQUIRE(stats, "ptd_eigh_profiled: stats must not be null");
  return eigh_dispatch(A, lda, n, k, evals, evecs, ldv, ws, ws_bytes, nullptr, all_values != 0, stats,
                       static_cast<hipStream_t>(stream));
}

size_t ptd_chol_inverse_workspace_bytes(int64_t m) { return chol_inverse_workspace_bytes(m); }

int ptd_chol_inverse(double* G, int64_t m, double* Wt, void* ws, size_t ws_bytes, void* stream) {
  return chol_inverse(G, m, Wt, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ptd_tridiagonalize_workspace_bytes(int64_t n) { return tridiag_workspace_bytes(n); }

int ptd_tridiagonalize(const double* A, int64_t lda, int64_t n, double* d, double* e, double* evals, void* ws,
                       size_t ws_bytes, void* stream) {
  return tridiagonalize_f64(A, lda, n, d, e, evals, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ptd_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int ab_dtype, int c_dtype) {
  if (ab_dtype == PTD_F32 && c_dtype == PTD_F32) return gemm_f32_workspace_bytes(M, N, K);
  if ((ab_dtype == PTD_BF16 || ab_dtype == PTD_F16) && (c_dtype == ab_dtype || c_dtype == PTD_F32))
    return gemm_bf16_workspace_bytes(M, N, K);
  return 0;
}

int ptd_gemm(const void* A, int64_t sam, int64_t sak, const void* B, int64_t sbk, int64_t sbn, void* C, int64_t ldc,
             int64_t M, int64_t N, int64_t K, int ab_dtype, int c_dtype, double alpha, const void* bias,
             void* stream) {
  return ptd_gemm_ws(A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, ab_dtype, c_dtype, alpha, bias, nullptr, 0, stream);
}

int ptd_gemm_ws(const void* A, int64_t sam, int64_t sak, const void* B, int64_t sbk, int64_t sbn, void* C, int64_t ldc,
                int64_t M, int64_t N, int64_t K, int ab_dtype, int c_dtype, double alpha, const void* bias, void* ws,
                size_t ws_bytes, void* stream) {
  PTD_REQUIRE(A && B && C, "ptd_gemm: null pointer");
  PTD_REQUIRE(M >= 0 && N >= 0 && K >= 0 && ldc >= N, "ptd_gemm: bad shape");
  PTD_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "ptd_gemm: dimension too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!ws) ws_bytes = 0;
  if (ab_dtype == PTD_F32 && c_dtype == PTD_F32)
    return gemm_f32(static_cast<const float*>(A), sam, sak, static_cast<const float*>(B), sbk, sbn,
                    static_cast<float*>(C), ldc, M, N, K, alpha, static_cast<const float*>(bias), ws, ws_bytes, st);
  if (ab_dtype == PTD_BF16 && (c_dtype == PTD_BF16 || c_dtype == PTD_F32))
    return gemm_bf16(static_cast<const unsigned short*>(A), sam, sak, static_cast<const unsigned short*>(B), sbk,
                     sbn, C, ldc, M, N, K, c_dtype == PTD_BF16, alpha, static_cast<const unsigned short*>(bias),
                     ws, ws_bytes, st);
  if (ab_dtype == PTD_F16 && (c_dtype == PTD_F16 || c_dtype == PTD_F32))
    return gemm_f16(static_cast<const unsigned short*>(A), sam, sak, static_cast<const unsigned short*>(B), sbk,
                    sbn, C, ldc, M, N, K, c_dtype == PTD_F16, alpha, static_cast<const unsigned short*>(bias),
                    ws, ws_bytes, st);
  if (ab_dtype == PTD_F64 && c_dtype == PTD_F64 && !bias)
    return gemm_f64(static_cast<const double*>(A), sam, sak, static_cast<const double*>(B), sbk, sbn,
                    static_cast<double*>(C), ldc, M, N, K, alpha, false, 1, st);
  set_error("ptd_gemm: unsupported dtype combination ab=%d c=%d", ab_dtype, c_dtype);
  return PTD_ERR_UNSUPPORTED;
}

int ptd_gemm_f64_form(int form, const double* A, int64_t sam, int64_t sak, const double* B, int64_t sbk, int64_t sbn,
                      const double* A2, const double* B2, double* C, int64_t ldc, int64_t slab, int64_t M, int64_t N,
                      int64_t K, double alpha, int ksplit, int lower_only, int* nslabs, double* row0_out, int batch,
                      int64_t bstride, void* stream) {
  PTD_REQUIRE(form >= PTD_GEMM_F64_PLAIN && form <= PTD_GEMM_F64_PAIR, "ptd_gemm_f64_form: unknown form %d", form);
  PTD_REQUIRE(A && B && C, "ptd_gemm_f64_form: null pointer");
  PTD_REQUIRE(form != PTD_GEMM_F64_PAIR || (A2 && B2), "ptd_gemm_f64_form: null pointer (second operand pair)");
  PTD_REQUIRE(form != PTD_GEMM_F64_SLABS || nslabs, "ptd_gemm_f64_form: null pointer (nslabs)");
  PTD_REQUIRE(M >= 0 && N >= 0 && K >= 0 && ldc >= N, "ptd_gemm_f64_form: bad shape");
  PTD_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "ptd_gemm_f64_form: dimension too large");
  PTD_REQUIRE((sam == 1) != (sak == 1) && (sbk == 1) != (sbn == 1),
              "ptd_gemm_f64_form: exactly one stride of each operand must be 1");
  PTD_REQUIRE(ksplit >= 1 && batch >= 1 && bstride >= 0, "ptd_gemm_f64_form: bad ksplit, batch or bstride");
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (form) {
    case PTD_GEMM_F64_PLAIN:
      return gemm_f64(A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, alpha, false, ksplit, st);
    case PTD_GEMM_F64_ACCUMULATE:
      if (ksplit > 1) {
        set_error("ptd_gemm_f64_form: ACCUMULATE with ksplit = %d is the atomic K split, which has no caller", ksplit);
        return PTD_ERR_UNSUPPORTED;
      }
      return gemm_f64(A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, alpha, true, 1, st);
    case PTD_GEMM_F64_SLABS:
      PTD_REQUIRE(slab >= M * ldc, "ptd_gemm_f64_form: slab %lld < M * ldc", (long long)slab);
      return gemm_f64_slabs(A, sam, sak, B, sbk, sbn, C, ldc, slab, M, N, K, alpha, ksplit, nslabs, lower_only != 0, st);
    default:
      return gemm_f64_pair(A, B, A2, B2, sam, sak, sbk, sbn, C, ldc, M, N, K, alpha, row0_out, st, batch, bstride);
  }
}

static size_t elt_bytes(int dtype) { return dtype == PTD_F32 ? 4 : 2; }

// the 16-bit products of an operand dtype (bf16 or f16: the same kernels, see gemm_bf16.hip)
static decltype(&gemm_bf16) gemm16_of(int dtype) { return dtype == PTD_F16 ? gemm_f16 : gemm_bf16; }

// 16-bit ranks that are not a multiple of 128 (a dwain search ends at 32 .. 96 on wide layers: Llama gate / up): the first
// product's output would have fewer than 128 columns -- a handful of 128-row tiles for the whole chip (x A^T at
// T = 2048, r = 32: 98 us on 16 workgroups, the library 20) -- and K = r of the second product no whole 64-deep step.
// The pair then runs on the rank padded with zeros: A's rows to a multiple of 128 (a copy in the workspace: the first
// product takes the split-K path of a 128-column tile row and leaves h [T, r128] with exact zeros behind column r),
// K of the second product to a multiple of 64 (B is read in place: its pieces behind column r are fetched from the
// row's start, h is zero there).  The results are those of the unpadded products: the padding adds exact zeros.
static int64_t lowrank_pad128(int64_t r, int dtype) {
  static const bool off = getenv("PTD_LOWRANK_PAD") && atoi(getenv("PTD_LOWRANK_PAD")) == 0;
  if (off || (dtype != PTD_BF16 && dtype != PTD_F16) || r % 8 != 0 || r % 128 == 0 || r > 1024) return r;
  return r <= 64 ? 64 : (int64_t)align_up((size_t)r, 128);     // (one column of 128 x 64 tiles serves a rank up to 64)
}

size_t ptd_lowrank_forward_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  const int64_t rp = lowrank_pad128(r, dtype);
  size_t b = align_up((size_t)T * (size_t)rp * elt_bytes(dtype), 256);
  if (rp != r) b += align_up((size_t)rp * (size_t)n_i * elt_bytes(dtype), 256);
  if (dtype == PTD_F32) b += gemm_f32_workspace_bytes(T, r, n_i);
  else b += gemm_bf16_workspace_bytes(T, rp, n_i);
  return b;
}

int ptd_lowrank_forward(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r,
                        const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
                        size_t ws_bytes, int dtype, void* stream) {
  PTD_REQUIRE(x && A && B && y && ws, "ptd_lowrank_forward: null pointer");
  PTD_REQUIRE(ldx >= n_i && lda >= n_i && ldb >= r && ldy >= n_o, "ptd_lowrank_forward: bad leading dimension");
  PTD_REQUIRE(dtype == PTD_F32 || dtype == PTD_BF16 || dtype == PTD_F16, "ptd_lowrank_forward: dtype must be f32, bf16 or f16");
  const int64_t rp = lowrank_pad128(r, dtype);
  if (rp != r && n_i % 8 == 0 && lda % 8 == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0 &&
      ws_bytes >= ptd_lowrank_forward_workspace_bytes(T, n_i, r, dtype)) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    typedef unsigned short u16;
    const auto gemm16 = gemm16_of(dtype);
    const size_t hp_bytes = align_up((size_t)T * (size_t)rp * 2, 256), ap_bytes = align_up((size_t)rp * (size_t)n_i * 2, 256);
    u16* hp = static_cast<u16*>(ws);
    u16* Ap = reinterpret_cast<u16*>(static_cast<char*>(ws) + hp_bytes);
    char* rest = static_cast<char*>(ws) + hp_bytes + ap_bytes;
    // the first product on the padded rank: A read in place -- its rows behind r are fetched from row 0 and the columns
    // they would produce are written as zeros (GemmBf16Args::nvalid); where no LDS-DMA kernel serves the shape, on a
    // zero-padded copy of A
    int rc = gemm16(static_cast<const u16*>(x), ldx, 1, static_cast<const u16*>(A), 1, lda, hp, rp, T, rp, n_i, true, 1.0,
                       nullptr, rest, ws_bytes - hp_bytes - ap_bytes, st, 0, r);
    if (rc == PTD_ERR_UNSUPPORTED) {
      rc = pad_rows_bf16(static_cast<const u16*>(A), lda, r, n_i, Ap, rp, st);
      if (rc != PTD_OK) return rc;
      rc = gemm16(static_cast<const u16*>(x), ldx, 1, Ap, 1, n_i, hp, rp, T, rp, n_i, true, 1.0, nullptr, rest,
                  ws_bytes - hp_bytes - ap_bytes, st, 0, 0);
    }
    if (rc != PTD_OK) return rc;
    // y = h B^T + bias with K padded to whole 64-deep steps where a short-K kernel serves the shape, else with K = r
    const int64_t k64 = (int64_t)align_up((size_t)r, 64);
    if (k64 != r && k64 <= 256) {
      rc = gemm16(hp, rp, 1, static_cast<const u16*>(B), 1, ldb, y, ldy, T, n_o, k64, true, 1.0,
                  static_cast<const u16*>(bias), nullptr, 0, st, r, 0);
      if (rc != PTD_ERR_UNSUPPORTED) return rc;
    }
    return ptd_gemm(hp, rp, 1, B, 1, ldb, y, ldy, T, n_o, r, dtype, dtype, 1.0, bias, stream);
  }
  const size_t h_bytes = align_up((size_t)T * (size_t)r * elt_bytes(dtype), 256);
  if (ws_bytes < h_bytes) {
    set_error("ptd_lowrank_forward: workspace %zu < required %zu bytes", ws_bytes, h_bytes);
    return PTD_ERR_WORKSPACE;
  }
  void* h = ws;
  // h = x A^T : A(m,k) = x[m*ldx + k], B(k,n) = A[n*lda + k];   y = h B^T + bias
  int rc;
  if (dtype == PTD_F32) {
    // a small rank leaves the first product with few output tiles: its K range is split over
    // workgroups through the rest of the workspace (deterministic two-pass reduction)
    rc = gemm_f32(static_cast<const float*>(x), ldx, 1, static_cast<const float*>(A), 1, lda, static_cast<float*>(h), r,
                  T, r, n_i, 1.0, nullptr, static_cast<char*>(ws) + h_bytes, ws_bytes - h_bytes,
                  static_cast<hipStream_t>(stream));
  } else {
    rc = gemm16_of(dtype)(static_cast<const unsigned short*>(x), ldx, 1, static_cast<const unsigned short*>(A), 1, lda,
                          h, r, T, r, n_i, true, 1.0, nullptr, static_cast<char*>(ws) + h_bytes, ws_bytes - h_bytes,
                          static_cast<hipStream_t>(stream), 0, 0);
  }
  if (rc != PTD_OK) return rc;
  return ptd_gemm(h, r, 1, B, 1, ldb, y, ldy, T, n_o, r, dtype, dtype, 1.0, bias, stream);
}

size_t ptd_lowrank_decode_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_decode_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_decode(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r,
                       const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
                       size_t ws_bytes, int dtype, void* stream) {
  PTD_REQUIRE(x && A && B && y && ws, "ptd_lowrank_decode: null pointer");
  PTD_REQUIRE(ldx >= n_i && lda >= n_i && ldb >= r && ldy >= n_o, "ptd_lowrank_decode: bad leading dimension");
  PTD_REQUIRE(dtype == PTD_F32 || dtype == PTD_BF16 || dtype == PTD_F16, "ptd_lowrank_decode: dtype must be f32, bf16 or f16");
  PTD_REQUIRE(aligned16(ws), "ptd_lowrank_decode: the workspace must be 16-byte aligned");
  // (nothing is launched for a shape the decode kernels do not serve: the caller takes ptd_lowrank_forward)
  if (!lowrank_decode_serves(T, n_i, r, n_o, dtype, x, ldx, A, lda, B, ldb)) {
    set_error("ptd_lowrank_decode: not served (T=%lld n_i=%lld r=%lld n_o=%lld dtype=%d: 1 <= T <= 16, r >= 8, n_i and r "
              "multiples of %d, 16-byte aligned rows)", (long long)T, (long long)n_i, (long long)r, (long long)n_o, dtype,
              dtype == PTD_F32 ? 4 : 8);
    return PTD_ERR_UNSUPPORTED;
  }
  if (ws_bytes < lowrank_decode_workspace_bytes(T, n_i, r, dtype)) {
    set_error("ptd_lowrank_decode: workspace %zu < required %zu bytes", ws_bytes,
              lowrank_decode_workspace_bytes(T, n_i, r, dtype));
    return PTD_ERR_WORKSPACE;
  }
  return lowrank_decode(x, ldx, T, n_i, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, dtype, static_cast<hipStream_t>(stream));
}

// What precedes a launch of the quantised-pair entry `name`, in the order it is reported: null pointers, leading
// dimensions (lda and ldb in bytes: code_a / code_b code bytes per row of A / B -- n for fp8, n / 2 for MXFP4, 3 (n / 4)
// for MXFP6; with `block_scales`, the MX formats, ldsa and ldsb too: one scale byte per 32 weights -- fp8's row scales have
// no pitch), the workspace's alignment, what the kernels serve (`served`: the entry's *_serves; `rule`:
// what it asks for, for the message) and the workspace's size (`need`: the entry's *_workspace_bytes).
#define PTD_STR_(v) #v
#define PTD_STR(v) PTD_STR_(v)
static int q_entry_checks(const char* name, const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                          const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                          int64_t ldsb, int64_t n_o, const void* y, int64_t ldy, const void* ws, size_t ws_bytes, int dtype,
                          int w_format, int64_t code_a, int64_t code_b, bool block_scales, bool served, const char* rule,
                          size_t need) {
  PTD_REQUIRE(x && Aq && scale_a && Bq && scale_b && y && ws, "%s: null pointer", name);
  PTD_REQUIRE(ldx >= n_i && lda >= code_a && ldb >= code_b && (!block_scales || (ldsa >= n_i / 32 && ldsb >= r / 32)) &&
                  ldy >= n_o,
              "%s: bad leading dimension", name);
  PTD_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", name);
  // (nothing is launched for what the kernels do not serve: the caller evaluates the expression on 16-bit copies)
  if (!served) {
    set_error("%s: not served (T=%lld n_i=%lld r=%lld n_o=%lld dtype=%d w_format=%d: bf16 / f16, %s)", name, (long long)T,
              (long long)n_i, (long long)r, (long long)n_o, dtype, w_format, rule);
    return PTD_ERR_UNSUPPORTED;
  }
  if (ws_bytes < need) {
    set_error("%s: workspace %zu < required %zu bytes", name, ws_bytes, need);
    return PTD_ERR_WORKSPACE;
  }
  return PTD_OK;
}

size_t ptd_lowrank_decode_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_decode_w8_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_decode_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                          const float* scale_a, int64_t r, const void* Bq, int64_t ldb, const float* scale_b, int64_t n_o,
                          const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format,
                          void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_decode_w8", x, ldx, T, n_i, Aq, lda, scale_a, 0, r, Bq, ldb, scale_b, 0, n_o, y,
                                ldy, ws, ws_bytes, dtype, w_format, n_i, r, false,
                                lowrank_decode_w8_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, scale_a, Bq, ldb,
                                                         scale_b, bias),
                                "PTD_W8_FP8_E4M3, 1 <= T <= 16, r >= 16, n_i and r multiples of 16, 16-byte aligned rows",
                                lowrank_decode_w8_workspace_bytes(T, n_i, r, dtype));
  if (rc != PTD_OK) return rc;
  return lowrank_decode_w8(x, ldx, T, n_i, Aq, lda, scale_a, r, Bq, ldb, scale_b, n_o, bias, y, ldy, ws, dtype,
                           static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_decode_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_decode_w4_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_decode_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                          const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                          int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                          int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_decode_w4", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b,
                                ldsb, n_o, y, ldy, ws, ws_bytes, dtype, w_format, n_i / 2, r / 2, true,
                                lowrank_decode_w4_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W4_MXFP4, 1 <= T <= 16, r >= 32, n_i and r multiples of 32, 16-byte aligned rows",
                                lowrank_decode_w4_workspace_bytes(T, n_i, r, dtype));
  if (rc != PTD_OK) return rc;
  return lowrank_decode_w4(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                           static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_decode_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_decode_w6_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_decode_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                          const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                          int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                          int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_decode_w6", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b,
                                ldsb, n_o, y, ldy, ws, ws_bytes, dtype, w_format, 3 * (n_i / 4), 3 * (r / 4), true,
                                lowrank_decode_w6_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W6_MXFP6_E2M3, 1 <= T <= 16, r >= 32, n_i and r multiples of 32, 8-byte aligned rows",
                                lowrank_decode_w6_workspace_bytes(T, n_i, r, dtype));
  if (rc != PTD_OK) return rc;
  return lowrank_decode_w6(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                           static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_decode_group_workspace_bytes(int count, int64_t T, int64_t n_i, const int64_t* r, int dtype) {
  if (!r || count < 1 || count > PTD_LOWRANK_GROUP_MAX) return 0;
  return lowrank_decode_group_workspace_bytes(count, T, n_i, r, dtype);
}

int ptd_lowrank_decode_group(const void* x, int64_t ldx, int64_t T, int64_t n_i, int count, const void* const* A,
                             const int64_t* lda, const int64_t* r, const void* const* B, const int64_t* ldb,
                             const int64_t* n_o, const void* const* bias, void* const* y, const int64_t* ldy, void* ws,
                             size_t ws_bytes, int dtype, void* stream) {
  PTD_REQUIRE(x && A && lda && r && B && ldb && n_o && y && ldy && ws, "ptd_lowrank_decode_group: null pointer");
  if (count < 1 || count > PTD_LOWRANK_GROUP_MAX) {
    set_error("ptd_lowrank_decode_group: not served (count=%d: 1 <= count <= %d)", count, PTD_LOWRANK_GROUP_MAX);
    return PTD_ERR_UNSUPPORTED;
  }
  PTD_REQUIRE(dtype == PTD_F32 || dtype == PTD_BF16 || dtype == PTD_F16,
              "ptd_lowrank_decode_group: dtype must be f32, bf16 or f16");
  PTD_REQUIRE(ldx >= n_i, "ptd_lowrank_decode_group: bad leading dimension");
  for (int m = 0; m < count; ++m) {
    PTD_REQUIRE(A[m] && B[m] && y[m], "ptd_lowrank_decode_group: null pointer (member %d)", m);
    PTD_REQUIRE(lda[m] >= n_i && ldb[m] >= r[m] && ldy[m] >= n_o[m],
                "ptd_lowrank_decode_group: bad leading dimension (member %d)", m);
  }
  PTD_REQUIRE(aligned16(ws), "ptd_lowrank_decode_group: the workspace must be 16-byte aligned");
  // (nothing is launched for a group the kernels do not serve: the caller runs the members one by one)
  if (!lowrank_decode_group_serves(count, T, n_i, r, n_o, dtype, x, ldx, A, lda, B, ldb)) {
    set_error("ptd_lowrank_decode_group: not served (count=%d T=%lld n_i=%lld dtype=%d: for every member 1 <= T <= 16, "
              "r >= 8, n_i and r multiples of %d, 16-byte aligned rows)", count, (long long)T, (long long)n_i, dtype,
              dtype == PTD_F32 ? 4 : 8);
    return PTD_ERR_UNSUPPORTED;
  }
  const size_t need = lowrank_decode_group_workspace_bytes(count, T, n_i, r, dtype);
  if (ws_bytes < need) {
    set_error("ptd_lowrank_decode_group: workspace %zu < required %zu bytes", ws_bytes, need);
    return PTD_ERR_WORKSPACE;
  }
  return lowrank_decode_group(x, ldx, T, n_i, count, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, dtype,
                              static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_decode_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype) {
  return lowrank_decode_gated_workspace_bytes(T, n_i, r_g, r_u, dtype);
}

int ptd_lowrank_decode_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g,
                             int64_t r_g, const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au,
                             int64_t lda_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_ff,
                             int act, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream) {
  PTD_REQUIRE(x && Ag && Bg && Au && Bu && y && ws, "ptd_lowrank_decode_gated: null pointer");
  PTD_REQUIRE(ldx >= n_i && lda_g >= n_i && lda_u >= n_i && ldb_g >= r_g && ldb_u >= r_u && ldy >= n_ff,
              "ptd_lowrank_decode_gated: bad leading dimension");
  PTD_REQUIRE(dtype == PTD_F32 || dtype == PTD_BF16 || dtype == PTD_F16,
              "ptd_lowrank_decode_gated: dtype must be f32, bf16 or f16");
  PTD_REQUIRE(aligned16(ws), "ptd_lowrank_decode_gated: the workspace must be 16-byte aligned");
  // (nothing is launched for what the kernels do not serve: the caller forms g and u and applies the activation itself)
  if (!lowrank_decode_gated_serves(T, n_i, r_g, r_u, n_ff, act, dtype, x, ldx, Ag, lda_g, Bg, ldb_g, Au, lda_u, Bu, ldb_u)) {
    set_error("ptd_lowrank_decode_gated: not served (T=%lld n_i=%lld r_g=%lld r_u=%lld n_ff=%lld act=%d dtype=%d: "
              "1 <= T <= 16, both r >= 8, n_i and both r multiples of %d, 16-byte aligned rows, act 0 (silu), "
              "1 (gelu_tanh) or 2 (relu))", (long long)T, (long long)n_i, (long long)r_g, (long long)r_u,
              (long long)n_ff, act, dtype, dtype == PTD_F32 ? 4 : 8);
    return PTD_ERR_UNSUPPORTED;
  }
  const size_t need = lowrank_decode_gated_workspace_bytes(T, n_i, r_g, r_u, dtype);
  if (ws_bytes < need) {
    set_error("ptd_lowrank_decode_gated: workspace %zu < required %zu bytes", ws_bytes, need);
    return PTD_ERR_WORKSPACE;
  }
  return lowrank_decode_gated(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u, n_ff,
                              act, y, ldy, ws, dtype, static_cast<hipStream_t>(stream));
}

// code bytes of a row of n weights in q_format (PTD_Q_*); -1 for an unknown format
static int64_t q_code_bytes(int q_format, int64_t n) {
  switch (q_format) {
    case PTD_Q_FP8_E4M3:
      return n;
    case PTD_Q_MXFP4:
      return n / 2;
    case PTD_Q_MXFP6_E2M3:
      return 3 * (n / 4);
  }
  return -1;
}

// whether one member of a quantised group or gated pair has its leading dimensions (MX: the scale rows' too)
static bool q_member_pitches(int q_format, int64_t n_i, int64_t r, int64_t n_o, int64_t lda, int64_t ldsa, int64_t ldb,
                             int64_t ldsb, int64_t ldy) {
  if (lda < q_code_bytes(q_format, n_i) || ldb < q_code_bytes(q_format, r) || ldy < n_o) return false;
  return q_format == PTD_Q_FP8_E4M3 || (ldsa >= n_i / 32 && ldsb >= r / 32);
}

// What precedes the launches of a quantised group entry `name` (ptd_lowrank_<regime>_group_q), in the order it is
// reported: null pointers, the format and the member count, leading dimensions, the workspace's alignment, what the
// kernels serve (`serves`: the entry's *_serves) and the workspace's size (`workspace`: the entry's *_workspace_bytes)
typedef bool (*q_group_serves_fn)(int, int, int64_t, int64_t, const int64_t*, const int64_t*, int, const void*, int64_t,
                                  const void* const*, const int64_t*, const void* const*, const void* const*,
                                  const int64_t*, const void* const*, const void* const*);
typedef size_t (*q_group_workspace_fn)(int, int, int64_t, int64_t, const int64_t*, int);
static int q_group_entry_checks(const char* name, const char* regime, q_group_serves_fn serves,
                                q_group_workspace_fn workspace, int q_format, const void* x, int64_t ldx, int64_t T,
                                int64_t n_i, int count, const void* const* Aq, const int64_t* lda, const void* const* sa,
                                const int64_t* ldsa, const int64_t* r, const void* const* Bq, const int64_t* ldb,
                                const void* const* sb, const int64_t* ldsb, const int64_t* n_o, const void* const* bias,
                                void* const* y, const int64_t* ldy, const void* ws, size_t ws_bytes, int dtype) {
  PTD_REQUIRE(x && Aq && lda && sa && r && Bq && ldb && sb && n_o && y && ldy && ws, "%s: null pointer", name);
  if (q_code_bytes(q_format, 0) < 0 || count < 1 || count > PTD_LOWRANK_GROUP_MAX) {
    set_error("%s: not served (q_format=%d count=%d: PTD_Q_FP8_E4M3, PTD_Q_MXFP4 or PTD_Q_MXFP6_E2M3, 1 <= count <= %d)",
              name, q_format, count, PTD_LOWRANK_GROUP_MAX);
    return PTD_ERR_UNSUPPORTED;
  }
  const bool mx = q_format != PTD_Q_FP8_E4M3;
  PTD_REQUIRE(!mx || (ldsa && ldsb), "%s: null pointer", name);
  PTD_REQUIRE(ldx >= n_i, "%s: bad leading dimension", name);
  for (int m = 0; m < count; ++m) {
    PTD_REQUIRE(Aq[m] && sa[m] && Bq[m] && sb[m] && y[m], "%s: null pointer (member %d)", name, m);
    PTD_REQUIRE(q_member_pitches(q_format, n_i, r[m], n_o[m], lda[m], mx ? ldsa[m] : 0, ldb[m], mx ? ldsb[m] : 0, ldy[m]),
                "%s: bad leading dimension (member %d)", name, m);
  }
  PTD_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", name);
  // (nothing is launched for a group the kernels do not serve: the caller runs the members one by one)
  if (!serves(q_format, count, T, n_i, r, n_o, dtype, x, ldx, Aq, lda, sa, Bq, ldb, sb, bias)) {
    set_error("%s: not served (q_format=%d count=%d T=%lld n_i=%lld dtype=%d: every member as the format's %s entry "
              "serves it)", name, q_format, count, (long long)T, (long long)n_i, dtype, regime);
    return PTD_ERR_UNSUPPORTED;
  }
  const size_t need = workspace(q_format, count, T, n_i, r, dtype);
  if (ws_bytes < need) {
    set_error("%s: workspace %zu < required %zu bytes", name, ws_bytes, need);
    return PTD_ERR_WORKSPACE;
  }
  return PTD_OK;
}

// The same for a quantised gated entry `name` (ptd_lowrank_<regime>_gated_q)
typedef bool (*q_gated_serves_fn)(int, int64_t, int64_t, int64_t, int64_t, int64_t, int, int, const void*, int64_t,
                                  const void*, int64_t, const void*, const void*, int64_t, const void*, const void*,
                                  const void*, int64_t, const void*, const void*, int64_t, const void*, const void*);
typedef size_t (*q_gated_workspace_fn)(int, int64_t, int64_t, int64_t, int64_t, int);
static int q_gated_entry_checks(const char* name, const char* regime, q_gated_serves_fn serves,
                                q_gated_workspace_fn workspace, int q_format, const void* x, int64_t ldx, int64_t T,
                                int64_t n_i, const void* Aq_g, int64_t lda_g, const void* sa_g, int64_t ldsa_g, int64_t r_g,
                                const void* Bq_g, int64_t ldb_g, const void* sb_g, int64_t ldsb_g, const void* bias_g,
                                const void* Aq_u, int64_t lda_u, const void* sa_u, int64_t ldsa_u, int64_t r_u,
                                const void* Bq_u, int64_t ldb_u, const void* sb_u, int64_t ldsb_u, const void* bias_u,
                                int64_t n_ff, int act, const void* y, int64_t ldy, const void* ws, size_t ws_bytes,
                                int dtype) {
  PTD_REQUIRE(x && Aq_g && sa_g && Bq_g && sb_g && Aq_u && sa_u && Bq_u && sb_u && y && ws, "%s: null pointer", name);
  if (q_code_bytes(q_format, 0) < 0) {
    set_error("%s: not served (q_format=%d: PTD_Q_FP8_E4M3, PTD_Q_MXFP4 or PTD_Q_MXFP6_E2M3)", name, q_format);
    return PTD_ERR_UNSUPPORTED;
  }
  PTD_REQUIRE(ldx >= n_i && q_member_pitches(q_format, n_i, r_g, n_ff, lda_g, ldsa_g, ldb_g, ldsb_g, ldy) &&
                  q_member_pitches(q_format, n_i, r_u, n_ff, lda_u, ldsa_u, ldb_u, ldsb_u, ldy),
              "%s: bad leading dimension", name);
  PTD_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", name);
  // (nothing is launched for what the kernels do not serve: the caller forms g and u and applies the activation itself)
  if (!serves(q_format, T, n_i, r_g, r_u, n_ff, act, dtype, x, ldx, Aq_g, lda_g, sa_g, Bq_g, ldb_g, sb_g, bias_g, Aq_u,
              lda_u, sa_u, Bq_u, ldb_u, sb_u, bias_u)) {
    set_error("%s: not served (q_format=%d T=%lld n_i=%lld r_g=%lld r_u=%lld n_ff=%lld act=%d dtype=%d: both members as "
              "the format's %s entry serves them, act 0 (silu), 1 (gelu_tanh) or 2 (relu))", name, q_format, (long long)T,
              (long long)n_i, (long long)r_g, (long long)r_u, (long long)n_ff, act, dtype, regime);
    return PTD_ERR_UNSUPPORTED;
  }
  const size_t need = workspace(q_format, T, n_i, r_g, r_u, dtype);
  if (ws_bytes < need) {
    set_error("%s: workspace %zu < required %zu bytes", name, ws_bytes, need);
    return PTD_ERR_WORKSPACE;
  }
  return PTD_OK;
}

size_t ptd_lowrank_decode_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r,
                                                  int dtype) {
  if (!r || count < 1 || count > PTD_LOWRANK_GROUP_MAX) return 0;
  return lowrank_decode_group_q_workspace_bytes(q_format, count, T, n_i, r, dtype);
}

int ptd_lowrank_decode_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                               const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                               const int64_t* r, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                               const int64_t* ldsb, const int64_t* n_o, const void* const* bias, void* const* y,
                               const int64_t* ldy, void* ws, size_t ws_bytes, int dtype, void* stream) {
  const int rc = q_group_entry_checks("ptd_lowrank_decode_group_q", "decode", lowrank_decode_group_q_serves,
                                      lowrank_decode_group_q_workspace_bytes, q_format, x, ldx, T, n_i, count, Aq, lda, sa,
                                      ldsa, r, Bq, ldb, sb, ldsb, n_o, bias, y, ldy, ws, ws_bytes, dtype);
  if (rc != PTD_OK) return rc;
  const bool mx = q_format != PTD_Q_FP8_E4M3;
  return lowrank_decode_group_q(q_format, x, ldx, T, n_i, count, Aq, lda, sa, mx ? ldsa : nullptr, r, Bq, ldb, sb,
                                mx ? ldsb : nullptr, n_o, bias, y, ldy, ws, dtype, static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_decode_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u,
                                                  int dtype) {
  return lowrank_decode_gated_q_workspace_bytes(q_format, T, n_i, r_g, r_u, dtype);
}

int ptd_lowrank_decode_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq_g,
                               int64_t lda_g, const void* sa_g, int64_t ldsa_g, int64_t r_g, const void* Bq_g,
                               int64_t ldb_g, const void* sb_g, int64_t ldsb_g, const void* bias_g, const void* Aq_u,
                               int64_t lda_u, const void* sa_u, int64_t ldsa_u, int64_t r_u, const void* Bq_u,
                               int64_t ldb_u, const void* sb_u, int64_t ldsb_u, const void* bias_u, int64_t n_ff, int act,
                               void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream) {
  const int rc = q_gated_entry_checks("ptd_lowrank_decode_gated_q", "decode", lowrank_decode_gated_q_serves,
                                      lowrank_decode_gated_q_workspace_bytes, q_format, x, ldx, T, n_i, Aq_g, lda_g, sa_g,
                                      ldsa_g, r_g, Bq_g, ldb_g, sb_g, ldsb_g, bias_g, Aq_u, lda_u, sa_u, ldsa_u, r_u, Bq_u,
                                      ldb_u, sb_u, ldsb_u, bias_u, n_ff, act, y, ldy, ws, ws_bytes, dtype);
  if (rc != PTD_OK) return rc;
  return lowrank_decode_gated_q(q_format, x, ldx, T, n_i, Aq_g, lda_g, sa_g, ldsa_g, r_g, Bq_g, ldb_g, sb_g, ldsb_g, bias_g,
                                Aq_u, lda_u, sa_u, ldsa_u, r_u, Bq_u, ldb_u, sb_u, ldsb_u, bias_u, n_ff, act, y, ldy, ws,
                                dtype, static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_skinny_group_q_workspace_bytes(int q_format, int count, int64_t T, int64_t n_i, const int64_t* r,
                                                  int dtype) {
  if (!r || count < 1 || count > PTD_LOWRANK_GROUP_MAX) return 0;
  return lowrank_skinny_group_q_workspace_bytes(q_format, count, T, n_i, r, dtype);
}

int ptd_lowrank_skinny_group_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, int count,
                               const void* const* Aq, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                               const int64_t* r, const void* const* Bq, const int64_t* ldb, const void* const* sb,
                               const int64_t* ldsb, const int64_t* n_o, const void* const* bias, void* const* y,
                               const int64_t* ldy, void* ws, size_t ws_bytes, int dtype, void* stream) {
  const int rc = q_group_entry_checks("ptd_lowrank_skinny_group_q", "skinny", lowrank_skinny_group_q_serves,
                                      lowrank_skinny_group_q_workspace_bytes, q_format, x, ldx, T, n_i, count, Aq, lda, sa,
                                      ldsa, r, Bq, ldb, sb, ldsb, n_o, bias, y, ldy, ws, ws_bytes, dtype);
  if (rc != PTD_OK) return rc;
  const bool mx = q_format != PTD_Q_FP8_E4M3;
  return lowrank_skinny_group_q(q_format, x, ldx, T, n_i, count, Aq, lda, sa, mx ? ldsa : nullptr, r, Bq, ldb, sb,
                                mx ? ldsb : nullptr, n_o, bias, y, ldy, ws, dtype, static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_skinny_gated_q_workspace_bytes(int q_format, int64_t T, int64_t n_i, int64_t r_g, int64_t r_u,
                                                  int dtype) {
  return lowrank_skinny_gated_q_workspace_bytes(q_format, T, n_i, r_g, r_u, dtype);
}

int ptd_lowrank_skinny_gated_q(int q_format, const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq_g,
                               int64_t lda_g, const void* sa_g, int64_t ldsa_g, int64_t r_g, const void* Bq_g,
                               int64_t ldb_g, const void* sb_g, int64_t ldsb_g, const void* bias_g, const void* Aq_u,
                               int64_t lda_u, const void* sa_u, int64_t ldsa_u, int64_t r_u, const void* Bq_u,
                               int64_t ldb_u, const void* sb_u, int64_t ldsb_u, const void* bias_u, int64_t n_ff, int act,
                               void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream) {
  const int rc = q_gated_entry_checks("ptd_lowrank_skinny_gated_q", "skinny", lowrank_skinny_gated_q_serves,
                                      lowrank_skinny_gated_q_workspace_bytes, q_format, x, ldx, T, n_i, Aq_g, lda_g, sa_g,
                                      ldsa_g, r_g, Bq_g, ldb_g, sb_g, ldsb_g, bias_g, Aq_u, lda_u, sa_u, ldsa_u, r_u, Bq_u,
                                      ldb_u, sb_u, ldsb_u, bias_u, n_ff, act, y, ldy, ws, ws_bytes, dtype);
  if (rc != PTD_OK) return rc;
  return lowrank_skinny_gated_q(q_format, x, ldx, T, n_i, Aq_g, lda_g, sa_g, ldsa_g, r_g, Bq_g, ldb_g, sb_g, ldsb_g, bias_g,
                                Aq_u, lda_u, sa_u, ldsa_u, r_u, Bq_u, ldb_u, sb_u, ldsb_u, bias_u, n_ff, act, y, ldy, ws,
                                dtype, static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_skinny_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_skinny_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_skinny(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* A, int64_t lda, int64_t r,
                       const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws,
                       size_t ws_bytes, int dtype, void* stream) {
  PTD_REQUIRE(x && A && B && y && ws, "ptd_lowrank_skinny: null pointer");
  PTD_REQUIRE(ldx >= n_i && lda >= n_i && ldb >= r && ldy >= n_o, "ptd_lowrank_skinny: bad leading dimension");
  PTD_REQUIRE(dtype == PTD_F32 || dtype == PTD_BF16 || dtype == PTD_F16, "ptd_lowrank_skinny: dtype must be f32, bf16 or f16");
  PTD_REQUIRE(aligned16(ws), "ptd_lowrank_skinny: the workspace must be 16-byte aligned");
  // (nothing is launched for a shape the skinny kernels do not serve: the caller takes ptd_lowrank_forward)
  if (!lowrank_skinny_serves(T, n_i, r, n_o, dtype, x, ldx, A, lda, B, ldb)) {
    set_error("ptd_lowrank_skinny: not served (T=%lld n_i=%lld r=%lld n_o=%lld dtype=%d: bf16 or f16, 32 <= T <= 96, "
              "r >= 8, n_i and r multiples of 8, 16-byte aligned rows)", (long long)T, (long long)n_i, (long long)r,
              (long long)n_o, dtype);
    return PTD_ERR_UNSUPPORTED;
  }
  if (ws_bytes < lowrank_skinny_workspace_bytes(T, n_i, r, dtype)) {
    set_error("ptd_lowrank_skinny: workspace %zu < required %zu bytes", ws_bytes,
              lowrank_skinny_workspace_bytes(T, n_i, r, dtype));
    return PTD_ERR_WORKSPACE;
  }
  return lowrank_skinny(x, ldx, T, n_i, A, lda, r, B, ldb, n_o, bias, y, ldy, ws, dtype, static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_skinny_w8_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_skinny_w8_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_skinny_w8(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                          const float* scale_a, int64_t r, const void* Bq, int64_t ldb, const float* scale_b, int64_t n_o,
                          const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, int w_format,
                          void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_skinny_w8", x, ldx, T, n_i, Aq, lda, scale_a, 0, r, Bq, ldb, scale_b, 0, n_o, y,
                                ldy, ws, ws_bytes, dtype, w_format, n_i, r, false,
                                lowrank_skinny_w8_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, scale_a, Bq, ldb,
                                                         scale_b, bias),
                                "PTD_W8_FP8_E4M3, 32 <= T <= " PTD_STR(PTD_LOWRANK_SKINNY_W8_MAX_T)
                                ", r >= 16, n_i and r multiples of 16, 16-byte aligned rows",
                                lowrank_skinny_w8_workspace_bytes(T, n_i, r, dtype));
  if (rc != PTD_OK) return rc;
  return lowrank_skinny_w8(x, ldx, T, n_i, Aq, lda, scale_a, r, Bq, ldb, scale_b, n_o, bias, y, ldy, ws, dtype,
                           static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_skinny_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_skinny_w4_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_skinny_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                          const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                          int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                          int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_skinny_w4", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b,
                                ldsb, n_o, y, ldy, ws, ws_bytes, dtype, w_format, n_i / 2, r / 2, true,
                                lowrank_skinny_w4_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W4_MXFP4, 32 <= T <= " PTD_STR(PTD_LOWRANK_SKINNY_W4_MAX_T)
                                ", r >= 32, n_i and r multiples of 32, 8-byte aligned code rows",
                                lowrank_skinny_w4_workspace_bytes(T, n_i, r, dtype));
  if (rc != PTD_OK) return rc;
  return lowrank_skinny_w4(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                           static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_skinny_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int dtype) {
  return lowrank_skinny_w6_workspace_bytes(T, n_i, r, dtype);
}

int ptd_lowrank_skinny_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                          const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                          int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                          int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_skinny_w6", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b,
                                ldsb, n_o, y, ldy, ws, ws_bytes, dtype, w_format, 3 * (n_i / 4), 3 * (r / 4), true,
                                lowrank_skinny_w6_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W6_MXFP6_E2M3, 32 <= T <= " PTD_STR(PTD_LOWRANK_SKINNY_W6_MAX_T)
                                ", r >= 32, n_i and r multiples of 32, 8-byte aligned code rows",
                                lowrank_skinny_w6_workspace_bytes(T, n_i, r, dtype));
  if (rc != PTD_OK) return rc;
  return lowrank_skinny_w6(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                           static_cast<hipStream_t>(stream));
}

// One MX factor as its 16-bit values (ptd_lowrank_dequant_w4 / _w6): `code_cols` code bytes per row
static int mx_dequant_entry(const char* name, const void* codes, int64_t ldq, const void* scales, int64_t lds, int64_t rows,
                            int64_t cols, const void* out, int64_t ldo, int dtype, int w_format, int64_t code_cols,
                            bool served) {
  PTD_REQUIRE(codes && scales && out, "%s: null pointer", name);
  PTD_REQUIRE(rows >= 1, "%s: rows must be positive", name);
  PTD_REQUIRE(ldq >= code_cols && lds >= cols / 32 && ldo >= cols, "%s: bad leading dimension", name);
  if (!served) {
    set_error("%s: not served (rows=%lld cols=%lld dtype=%d w_format=%d: bf16 / f16, cols a positive multiple of 32, "
              "8-byte aligned code rows, 16-byte aligned output rows)", name, (long long)rows, (long long)cols, dtype,
              w_format);
    return PTD_ERR_UNSUPPORTED;
  }
  return PTD_OK;
}

int ptd_lowrank_dequant_w4(const void* codes, int64_t ldq, const void* scales, int64_t lds, int64_t rows, int64_t cols,
                           void* out, int64_t ldo, int dtype, int w_format, void* stream) {
  const int rc = mx_dequant_entry("ptd_lowrank_dequant_w4", codes, ldq, scales, lds, rows, cols, out, ldo, dtype, w_format,
                                  cols / 2, lowrank_dequant_w4_serves(codes, ldq, rows, cols, out, ldo, dtype, w_format));
  if (rc != PTD_OK) return rc;
  return lowrank_dequant_w4(codes, ldq, scales, lds, rows, cols, out, ldo, dtype, static_cast<hipStream_t>(stream));
}

int ptd_lowrank_dequant_w6(const void* codes, int64_t ldq, const void* scales, int64_t lds, int64_t rows, int64_t cols,
                           void* out, int64_t ldo, int dtype, int w_format, void* stream) {
  const int rc = mx_dequant_entry("ptd_lowrank_dequant_w6", codes, ldq, scales, lds, rows, cols, out, ldo, dtype, w_format,
                                  3 * (cols / 4), lowrank_dequant_w6_serves(codes, ldq, rows, cols, out, ldo, dtype, w_format));
  if (rc != PTD_OK) return rc;
  return lowrank_dequant_w6(codes, ldq, scales, lds, rows, cols, out, ldo, dtype, static_cast<hipStream_t>(stream));
}

// The MX pair on the tile products (ptd_lowrank_tile_w4 / _w6): A^ and B^ in front of the 16-bit entry's own workspace
static size_t lowrank_tile_mx_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype) {
  if (T < 1 || n_i < 1 || r < 1 || n_o < 1) return 0;
  return lowrank_tile_mx_factor_bytes(r, n_i) + lowrank_tile_mx_factor_bytes(n_o, r) +
         ptd_lowrank_forward_workspace_bytes(T, n_i, r, dtype);
}

// ptd_lowrank_forward on the factors the dequantisation launch has just left at the head of the workspace
static int lowrank_tile_mx_products(const void* x, int64_t ldx, int64_t T, int64_t n_i, int64_t r, int64_t n_o,
                                    const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype,
                                    void* stream) {
  const size_t a_bytes = lowrank_tile_mx_factor_bytes(r, n_i), b_bytes = lowrank_tile_mx_factor_bytes(n_o, r);
  char* const a_hat = static_cast<char*>(ws);
  return ptd_lowrank_forward(x, ldx, T, n_i, a_hat, n_i, r, a_hat + a_bytes, r, n_o, bias, y, ldy, a_hat + a_bytes + b_bytes,
                             ws_bytes - a_bytes - b_bytes, dtype, stream);
}

size_t ptd_lowrank_tile_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype) {
  return lowrank_tile_mx_workspace_bytes(T, n_i, r, n_o, dtype);
}

int ptd_lowrank_tile_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                        const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                        int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                        int dtype, int w_format, void* stream) {
  int rc = q_entry_checks("ptd_lowrank_tile_w4", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, y,
                          ldy, ws, ws_bytes, dtype, w_format, n_i / 2, r / 2, true,
                          lowrank_tile_w4_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                          "PTD_W4_MXFP4, T >= 1, r >= 32, n_i and r multiples of 32, 8-byte aligned code rows",
                          lowrank_tile_mx_workspace_bytes(T, n_i, r, n_o, dtype));
  if (rc != PTD_OK) return rc;
  rc = lowrank_tile_w4_dequant(Aq, lda, scale_a, ldsa, n_i, r, Bq, ldb, scale_b, ldsb, n_o, ws, dtype,
                               static_cast<hipStream_t>(stream));
  if (rc != PTD_OK) return rc;
  return lowrank_tile_mx_products(x, ldx, T, n_i, r, n_o, bias, y, ldy, ws, ws_bytes, dtype, stream);
}

size_t ptd_lowrank_tile_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype) {
  return lowrank_tile_mx_workspace_bytes(T, n_i, r, n_o, dtype);
}

int ptd_lowrank_tile_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                        const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                        int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                        int dtype, int w_format, void* stream) {
  int rc = q_entry_checks("ptd_lowrank_tile_w6", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, y,
                          ldy, ws, ws_bytes, dtype, w_format, 3 * (n_i / 4), 3 * (r / 4), true,
                          lowrank_tile_w6_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                          "PTD_W6_MXFP6_E2M3, T >= 1, r >= 32, n_i and r multiples of 32, 8-byte aligned code rows",
                          lowrank_tile_mx_workspace_bytes(T, n_i, r, n_o, dtype));
  if (rc != PTD_OK) return rc;
  rc = lowrank_tile_w6_dequant(Aq, lda, scale_a, ldsa, n_i, r, Bq, ldb, scale_b, ldsb, n_o, ws, dtype,
                               static_cast<hipStream_t>(stream));
  if (rc != PTD_OK) return rc;
  return lowrank_tile_mx_products(x, ldx, T, n_i, r, n_o, bias, y, ldy, ws, ws_bytes, dtype, stream);
}

// MXFP8 activations on the block-scaled MFMA (lowrank_a8.hip)
int ptd_mxfp8_quantize_rows(const void* x, int64_t ldx, int64_t T, int64_t n, void* codes, int64_t ldc, void* scales,
                            int64_t lds, int dtype, void* stream) {
  PTD_REQUIRE(x && codes && scales, "ptd_mxfp8_quantize_rows: null pointer");
  PTD_REQUIRE(T >= 1, "ptd_mxfp8_quantize_rows: T must be positive");
  PTD_REQUIRE(ldx >= n && ldc >= n && lds >= n / 32, "ptd_mxfp8_quantize_rows: bad leading dimension");
  if (!lowrank_a8_quantize_serves(x, ldx, T, n, codes, ldc, dtype)) {
    set_error("ptd_mxfp8_quantize_rows: not served (T=%lld n=%lld dtype=%d: bf16 / f16, n a positive multiple of 32, "
              "16-byte aligned rows of x and of the codes)", (long long)T, (long long)n, dtype);
    return PTD_ERR_UNSUPPORTED;
  }
  return lowrank_a8_quantize(x, ldx, T, n, codes, ldc, scales, lds, dtype, "ptd_mxfp8_quantize_rows",
                             static_cast<hipStream_t>(stream));
}

int ptd_mx_product_a8(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* Wq,
                      int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo,
                      int dtype, int q_format, void* stream) {
  PTD_REQUIRE(xq && ex && Wq && ew && out, "ptd_mx_product_a8: null pointer");
  PTD_REQUIRE(T >= 1, "ptd_mx_product_a8: T must be positive");
  const int64_t code_w = q_format == PTD_Q_MXFP6_E2M3 ? 3 * (K / 4) : K / 2;      // (an unknown format is refused below)
  PTD_REQUIRE(ldxq >= K && ldex >= K / 32 && ldw >= code_w && ldew >= K / 32 && ldo >= N,
              "ptd_mx_product_a8: bad leading dimension");
  if (!lowrank_a8_product_serves(xq, ldxq, T, K, Wq, ldw, N, bias, dtype, q_format)) {
    set_error("ptd_mx_product_a8: not served (T=%lld K=%lld N=%lld dtype=%d q_format=%d: bf16 / f16, PTD_Q_MXFP4 / "
              "PTD_Q_MXFP6_E2M3, K a positive multiple of 32, 16-byte aligned activation code rows, 8-byte aligned weight "
              "code rows)", (long long)T, (long long)K, (long long)N, dtype, q_format);
    return PTD_ERR_UNSUPPORTED;
  }
  return lowrank_a8_product(xq, ldxq, ex, ldex, T, K, Wq, ldw, ew, ldew, N, bias, out, ldo, dtype, q_format,
                            static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_a8_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype) {
  (void)n_o, (void)dtype;
  return lowrank_a8_workspace_bytes(T, n_i, r);
}

int ptd_lowrank_a8_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                      const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                      int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                      int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_a8_w4", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o,
                                y, ldy, ws, ws_bytes, dtype, w_format, n_i / 2, r / 2, true,
                                lowrank_a8_w4_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W4_MXFP4, 1 <= T <= 2^24, r >= 32, n_i and r multiples of 32, 8-byte aligned code rows",
                                lowrank_a8_workspace_bytes(T, n_i, r));
  if (rc != PTD_OK) return rc;
  return lowrank_a8_w4(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                       static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_a8_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype) {
  (void)n_o, (void)dtype;
  return lowrank_a8_workspace_bytes(T, n_i, r);
}

int ptd_lowrank_a8_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                      const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                      int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                      int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_a8_w6", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o,
                                y, ldy, ws, ws_bytes, dtype, w_format, 3 * (n_i / 4), 3 * (r / 4), true,
                                lowrank_a8_w6_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W6_MXFP6_E2M3, 1 <= T <= 2^24, r >= 32, n_i and r multiples of 32, 8-byte aligned code "
                                "rows",
                                lowrank_a8_workspace_bytes(T, n_i, r));
  if (rc != PTD_OK) return rc;
  return lowrank_a8_w6(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                       static_cast<hipStream_t>(stream));
}

// MXFP8 activations at prefill sizes: the LDS-staged tiled product and the pair on it (lowrank_a8_tile.hip)
int ptd_mx_product_a8_tile(const void* xq, int64_t ldxq, const void* ex, int64_t ldex, int64_t T, int64_t K, const void* Wq,
                           int64_t ldw, const void* ew, int64_t ldew, int64_t N, const void* bias, void* out, int64_t ldo,
                           void* outq, int64_t ldoq, void* eout, int64_t ldeo, int dtype, int q_format, void* stream) {
  PTD_REQUIRE(xq && ex && Wq && ew, "ptd_mx_product_a8_tile: null pointer");
  PTD_REQUIRE(!outq == !eout, "ptd_mx_product_a8_tile: outq and eout go together");
  PTD_REQUIRE(T >= 1, "ptd_mx_product_a8_tile: T must be positive");
  const int64_t code_w = q_format == PTD_Q_MXFP6_E2M3 ? 3 * (K / 4) : K / 2;      // (an unknown format is refused below)
  PTD_REQUIRE(ldxq >= K && ldex >= K / 32 && ldw >= code_w && ldew >= K / 32 && (!out || ldo >= N) &&
                  (!outq || (ldoq >= N && ldeo >= N / 32)),
              "ptd_mx_product_a8_tile: bad leading dimension");
  if (!lowrank_a8_tile_product_serves(xq, ldxq, T, K, Wq, ldw, N, bias, out, outq, ldoq, dtype, q_format)) {
    set_error("ptd_mx_product_a8_tile: not served (T=%lld K=%lld N=%lld dtype=%d q_format=%d: what ptd_mx_product_a8 serves, "
              "an output, and for outq N a multiple of 32 with 16-byte aligned code rows)", (long long)T, (long long)K,
              (long long)N, dtype, q_format);
    return PTD_ERR_UNSUPPORTED;
  }
  return lowrank_a8_tile_product(xq, ldxq, ex, ldex, T, K, Wq, ldw, ew, ldew, N, bias, out, ldo, outq, ldoq, eout, ldeo, dtype,
                                 q_format, static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_a8_tile_w4_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype) {
  (void)n_o, (void)dtype;
  return lowrank_a8_tile_workspace_bytes(T, n_i, r);
}

int ptd_lowrank_a8_tile_w4(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                           const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                           int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                           int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_a8_tile_w4", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb,
                                n_o, y, ldy, ws, ws_bytes, dtype, w_format, n_i / 2, r / 2, true,
                                lowrank_a8_w4_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W4_MXFP4, 1 <= T <= 2^24, r >= 32, n_i and r multiples of 32, 8-byte aligned code rows",
                                lowrank_a8_tile_workspace_bytes(T, n_i, r));
  if (rc != PTD_OK) return rc;
  return lowrank_a8_tile_w4(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                            static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_a8_tile_w6_workspace_bytes(int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype) {
  (void)n_o, (void)dtype;
  return lowrank_a8_tile_workspace_bytes(T, n_i, r);
}

int ptd_lowrank_a8_tile_w6(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Aq, int64_t lda,
                           const void* scale_a, int64_t ldsa, int64_t r, const void* Bq, int64_t ldb, const void* scale_b,
                           int64_t ldsb, int64_t n_o, const void* bias, void* y, int64_t ldy, void* ws, size_t ws_bytes,
                           int dtype, int w_format, void* stream) {
  const int rc = q_entry_checks("ptd_lowrank_a8_tile_w6", x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb,
                                n_o, y, ldy, ws, ws_bytes, dtype, w_format, 3 * (n_i / 4), 3 * (r / 4), true,
                                lowrank_a8_w6_serves(T, n_i, r, n_o, dtype, w_format, x, ldx, Aq, lda, Bq, ldb, bias),
                                "PTD_W6_MXFP6_E2M3, 1 <= T <= 2^24, r >= 32, n_i and r multiples of 32, 8-byte aligned code "
                                "rows",
                                lowrank_a8_tile_workspace_bytes(T, n_i, r));
  if (rc != PTD_OK) return rc;
  return lowrank_a8_tile_w6(x, ldx, T, n_i, Aq, lda, scale_a, ldsa, r, Bq, ldb, scale_b, ldsb, n_o, bias, y, ldy, ws, dtype,
                            static_cast<hipStream_t>(stream));
}

int ptd_lowrank_plan(int family, int64_t T, int64_t n_i, int64_t r, int64_t n_o, int dtype, int32_t* out, int cap) {
  PTD_REQUIRE(out, "ptd_lowrank_plan: null pointer");
  PTD_REQUIRE(cap >= PTD_PLAN_LEN, "ptd_lowrank_plan: out holds %d values, the plan has %d", cap, PTD_PLAN_LEN);
  if (lowrank_plan(family, T, n_i, r, n_o, dtype, out) != PTD_OK) {
    set_error("ptd_lowrank_plan: not served (family=%d T=%lld n_i=%lld r=%lld n_o=%lld dtype=%d)", family, (long long)T,
              (long long)n_i, (long long)r, (long long)n_o, dtype);
    return PTD_ERR_UNSUPPORTED;
  }
  return PTD_PLAN_LEN;
}

size_t ptd_lowrank_skinny_gated_workspace_bytes(int64_t T, int64_t n_i, int64_t r_g, int64_t r_u, int dtype) {
  return lowrank_skinny_gated_workspace_bytes(T, n_i, r_g, r_u, dtype);
}

int ptd_lowrank_skinny_gated(const void* x, int64_t ldx, int64_t T, int64_t n_i, const void* Ag, int64_t lda_g,
                             int64_t r_g, const void* Bg, int64_t ldb_g, const void* bias_g, const void* Au,
                             int64_t lda_u, int64_t r_u, const void* Bu, int64_t ldb_u, const void* bias_u, int64_t n_ff,
                             int act, void* y, int64_t ldy, void* ws, size_t ws_bytes, int dtype, void* stream) {
  PTD_REQUIRE(x && Ag && Bg && Au && Bu && y && ws, "ptd_lowrank_skinny_gated: null pointer");
  PTD_REQUIRE(ldx >= n_i && lda_g >= n_i && lda_u >= n_i && ldb_g >= r_g && ldb_u >= r_u && ldy >= n_ff,
              "ptd_lowrank_skinny_gated: bad leading dimension");
  PTD_REQUIRE(dtype == PTD_F32 || dtype == PTD_BF16 || dtype == PTD_F16,
              "ptd_lowrank_skinny_gated: dtype must be f32, bf16 or f16");
  PTD_REQUIRE(aligned16(ws), "ptd_lowrank_skinny_gated: the workspace must be 16-byte aligned");
  // (nothing is launched for what the kernels do not serve: the caller forms g and u and applies the activation itself)
  if (!lowrank_skinny_gated_serves(T, n_i, r_g, r_u, n_ff, act, dtype, x, ldx, Ag, lda_g, Bg, ldb_g, Au, lda_u, Bu, ldb_u)) {
    set_error("ptd_lowrank_skinny_gated: not served (T=%lld n_i=%lld r_g=%lld r_u=%lld n_ff=%lld act=%d dtype=%d: "
              "bf16 or f16, 32 <= T <= 96, both r >= 8, n_i and both r multiples of 8, 16-byte aligned rows, act 0 (silu), "
              "1 (gelu_tanh) or 2 (relu))", (long long)T, (long long)n_i, (long long)r_g, (long long)r_u,
              (long long)n_ff, act, dtype);
    return PTD_ERR_UNSUPPORTED;
  }
  const size_t need = lowrank_skinny_gated_workspace_bytes(T, n_i, r_g, r_u, dtype);
  if (ws_bytes < need) {
    set_error("ptd_lowrank_skinny_gated: workspace %zu < required %zu bytes", ws_bytes, need);
    return PTD_ERR_WORKSPACE;
  }
  return lowrank_skinny_gated(x, ldx, T, n_i, Ag, lda_g, r_g, Bg, ldb_g, bias_g, Au, lda_u, r_u, Bu, ldb_u, bias_u, n_ff,
                              act, y, ldy, ws, dtype, static_cast<hipStream_t>(stream));
}

size_t ptd_lowrank_forward_nchw_workspace_bytes(int64_t batch, int64_t hw, int64_t r, int dtype) {
  return align_up((size_t)batch * (size_t)r * (size_t)hw * elt_bytes(dtype), 256);
}

int ptd_lowrank_forward_nchw(const void* x, int64_t batch, int64_t n_i, int64_t hw, const void* A, int64_t lda,
                             int64_t r, const void* B, int64_t ldb, int64_t n_o, const void* bias, void* y, void* ws,
                             size_t ws_bytes, int dtype, void* stream) {
  PTD_REQUIRE(x && A && B && y && ws, "ptd_lowrank_forward_nchw: null pointer");
  PTD_REQUIRE(batch >= 0 && n_i >= 1 && hw >= 1 && r >= 1 && n_o >= 1 && lda >= n_i && ldb >= r,
              "ptd_lowrank_forward_nchw: bad shape");
  PTD_REQUIRE(dtype == PTD_F32 || dtype == PTD_BF16 || dtype == PTD_F16,
              "ptd_lowrank_forward_nchw: dtype must be f32, bf16 or f16");
  if (ws_bytes < ptd_lowrank_forward_nchw_workspace_bytes(batch, hw, r, dtype)) {
    set_error("ptd_lowrank_forward_nchw: workspace too small");
    return PTD_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  // per image b: h_b[r, hw] = A x_b (x_b = x + b n_i hw viewed [n_i, hw], pixels contiguous), y_b[n_o, hw] = B h_b + bias
  if (dtype == PTD_F32) {
    int rc = gemm_f32_batched(static_cast<const float*>(A), lda, 1, 0, static_cast<const float*>(x), hw, 1, n_i * hw,
                              static_cast<float*>(ws), hw, r * hw, r, hw, n_i, batch, 1.0, nullptr, st);
    if (rc != PTD_OK) return rc;
    return gemm_f32_batched(static_cast<const float*>(B), ldb, 1, 0, static_cast<const float*>(ws), hw, 1, r * hw,
                            static_cast<float*>(y), hw, n_o * hw, n_o, hw, r, batch, 1.0,
                            static_cast<const float*>(bias), st);
  }
  typedef unsigned short u16;
  const auto gemm16_batched = dtype == PTD_F16 ? gemm_f16_batched : gemm_bf16_batched;
  int rc = gemm16_batched(static_cast<const u16*>(A), lda, 1, 0, static_cast<const u16*>(x), hw, 1, n_i * hw,
                             static_cast<u16*>(ws), hw, r * hw, r, hw, n_i, batch, 1.0, nullptr, st);
  if (rc != PTD_OK) return rc;
  return gemm16_batched(static_cast<const u16*>(B), ldb, 1, 0, static_cast<const u16*>(ws), hw, 1, r * hw,
                        static_cast<u16*>(y), hw, n_o * hw, n_o, hw, r, batch, 1.0, static_cast<const u16*>(bias),
                        st);
}

size_t ptd_nsr_workspace_bytes(int64_t R, int64_t C) { return nsr_workspace_bytes(R, C); }

int ptd_nsr_plan(int64_t R, int64_t C, int dtype, int aligned, int32_t* out, int cap) {
  PTD_REQUIRE(out, "ptd_nsr_plan: null pointer");
  PTD_REQUIRE(cap >= PTD_NSR_PLAN_LEN, "ptd_nsr_plan: out holds %d values, the plan has %d", cap, PTD_NSR_PLAN_LEN);
  PTD_REQUIRE(R >= 1 && C >= 1, "ptd_nsr_plan: bad shape");
  if (nsr_plan_query(R, C, dtype, aligned != 0, out) != PTD_OK) {
    set_error("ptd_nsr_plan: unsupported dtype %d", dtype);
    return PTD_ERR_UNSUPPORTED;
  }
  return PTD_NSR_PLAN_LEN;
}

int ptd_nsr_workspace_init(void* ws, size_t ws_bytes, void* stream) {
  return nsr_workspace_init(ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int ptd_nsr(const void* x, const void* y, int64_t R, int64_t C, int dtype, double eps, double* out, void* ws,
            size_t ws_bytes, void* stream) {
  return nsr(x, y, R, C, dtype, eps, out, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

size_t ptd_sym_kl_workspace_bytes(int64_t B) { return sym_kl_workspace_bytes(B); }

int ptd_sym_kl(const void* s, const void* t, int64_t B, int64_t C, int dtype, double* out, void* ws, size_t ws_bytes,
               void* stream) {
  return sym_kl(s, t, B, C, dtype, out, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int ptd_kl_rows(const void* q, const void* p, int64_t B, int64_t C, int dtype, double* rows, void* stream) {
  return kl_rows(q, p, B, C, dtype, rows, static_cast<hipStream_t>(stream));
}

}  // extern "C"

// C++-linkage views of the solver selection for the other translation units (eigh_factored.hip)
namespace ptd {
size_t eigh_select_workspace_bytes(int64_t n) { return ptd_eigh_workspace_bytes(n); }
int eigh_select(const double* A, int64_t lda, int64_t n, int64_t k, double* evals, double* evecs, int64_t ldv,
                void* ws, size_t ws_bytes, int* sweeps_out, ptd_eigh_stats* stats, hipStream_t st) {
  // the factored route reads only the k largest eigenvalues of its reduced problem
  return eigh_dispatch(A, lda, n, k, evals, evecs, ldv, ws, ws_bytes, sweeps_out, false, stats, st);
}
}  // namespace ptd
