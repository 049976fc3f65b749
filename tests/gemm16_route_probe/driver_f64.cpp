// Drives ptd::gemm_f64 / gemm_f64_slabs / gemm_f64_pair of a host-only compile of gemm_f64.hip (see shim.h) with fake
// pointers.  The calls come from standard input, one per line (tests/gemm_f64_routes.py writes them):
//   <form> <M> <N> <K> <layout> <pitch a> <pitch b> <ldc> <A+> <B+> <C+> <ksplit> <lower> <batch>
// form: plain, acc (beta1), slabs, pair.  layout as in tests/test_gemm_routes_gpu.py: first letter 't' = A stored [K, M]
// (sam = 1), second letter 'n' = B stored [K, N] (sbn = 1).  <A+> .. <C+>: bytes added to the 16-byte aligned bases.
// Each call is echoed, followed by
//   > <rc> [ns=<slabs written>] [label; label] [@<handle> <gx>,<gy>,<gz> <block>] ...
// Linked with NO HIP library: the runtime symbols the host objects reference are the no-ops below, so nothing here can
// reach a GPU.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../ptdeco_amd/csrc/kernels.h"

namespace ptd {
void set_error(const char*, ...) {}
__thread LaunchTrace g_launch_trace = {false, 0, {nullptr}};
}  // namespace ptd

static std::string g_launches;

void ptd_probe_launch(const void* kernel, dim3 grid, dim3 block) {
  char buf[96];
  snprintf(buf, sizeof buf, " @%p %u,%u,%u %u", kernel, grid.x, grid.y, grid.z, block.x);
  g_launches += buf;
}
void ptd_probe_int(long long) {}
void ptd_probe_real(double) {}

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipErrorUnknown; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipErrorUnknown; }
const char* hipGetErrorString(hipError_t) { return "no runtime"; }
}

static double* fake(uintptr_t base, long long off) { return reinterpret_cast<double*>(base + 16 + off); }

int main() {
  char line[512], form[16], lay[8];
  while (fgets(line, sizeof line, stdin)) {
    long long M, N, K, pa, pb, ldc, oa, ob, oc;
    int ksplit, lower, batch;
    if (line[0] == '#' || line[0] == '\n') continue;
    if (sscanf(line, "%15s %lld %lld %lld %7s %lld %lld %lld %lld %lld %lld %d %d %d", form, &M, &N, &K, lay, &pa, &pb, &ldc,
               &oa, &ob, &oc, &ksplit, &lower, &batch) != 14 || strlen(lay) != 2) {
      fprintf(stderr, "bad call line: %s", line);
      return 2;
    }
    const bool at = lay[0] == 't', bn = lay[1] == 'n';
    const int64_t sam = at ? 1 : pa, sak = at ? pa : 1, sbk = bn ? pb : 1, sbn = bn ? 1 : pb;
    const double *A = fake(0x10000000, oa), *B = fake(0x20000000, ob);
    double* C = fake(0x30000000, oc);
    ptd::g_launch_trace.on = true;
    ptd::g_launch_trace.count = 0;
    g_launches.clear();
    int rc, ns = -1;
    if (!strcmp(form, "plain") || !strcmp(form, "acc")) {
      rc = ptd::gemm_f64(A, sam, sak, B, sbk, sbn, C, ldc, M, N, K, 1.0, form[0] == 'a', ksplit, nullptr);
    } else if (!strcmp(form, "slabs")) {
      rc = ptd::gemm_f64_slabs(A, sam, sak, B, sbk, sbn, C, ldc, M * ldc, M, N, K, 1.0, ksplit, &ns, lower != 0, nullptr);
    } else if (!strcmp(form, "pair")) {
      rc = ptd::gemm_f64_pair(A, B, fake(0x40000000, ob), fake(0x50000000, oa), sam, sak, sbk, sbn, C, ldc, M, N, K, -1.0,
                              fake(0x60000000, oc), nullptr, batch, (M + K + 8) * ldc);
    } else {
      fprintf(stderr, "unknown form: %s\n", form);
      return 2;
    }
    line[strcspn(line, "\n")] = 0;
    printf("%s > %d", line, rc);
    if (ns >= 0) printf(" ns=%d", ns);
    for (int i = 0; i < ptd::g_launch_trace.count && i < 32; ++i) printf("%s %s", i ? ";" : "", ptd::g_launch_trace.what[i]);
    printf("%s\n", g_launches.c_str());
  }
  return 0;
}
