// Drives ptd::gemm_bf16 / ptd::gemm_f16 of a host-only compile of gemm_bf16.hip (see shim.h) over a lattice of calls
// with fake pointers and prints one line per call:
//   <inputs> > <rc> [label; label] [@<handle> <gx>,<gy>,<gz> <block> <scalar launch arguments>] ...
// Linked with NO HIP library: the runtime symbols the host objects reference are the no-ops below, so nothing here can
// reach a GPU.  `driver named` prints the named cases only (what the switch runs use), `driver` the lattice as well.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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
void ptd_probe_int(long long v) { g_launches += " " + std::to_string(v); }
void ptd_probe_real(double v) {
  char buf[32];
  snprintf(buf, sizeof buf, " %g", v);
  g_launches += buf;
}

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipErrorUnknown; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) { return hipErrorUnknown; }
hipError_t hipDeviceGetAttribute(int*, hipDeviceAttribute_t, int) { return hipErrorUnknown; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipErrorUnknown; }
hipError_t hipGetDevice(int*) { return hipErrorUnknown; }
const char* hipGetErrorString(hipError_t) { return "no runtime"; }
}

namespace {

struct Case {
  int64_t M, N, K;
  int ws = 0;                  // 0 none, 1 what gemm_bf16_workspace_bytes asks for, 2 one byte less, 3 base 4 bytes off,
                               // 4 a pointer with 0 bytes
  const char* lay = "nt";      // storage as in tests/test_gemm_routes_gpu.py: "nt" = A [M, K], B [N, K]
  int64_t pitch_a = 0, pitch_b = 0, ldc = 0;   // 0: row length + 8
  int off_a = 0, off_b = 0, off_c = 0;         // bytes added to the 16-byte aligned bases
  bool bias = false;
  double alpha = 1.0;
  int64_t kv = 0, nv = 0;
};

unsigned short* fake(uintptr_t base, int off) { return reinterpret_cast<unsigned short*>(base + 16 + off); }

void run(const Case& c, int el, bool c16) {
  const bool at = c.lay[0] == 't', bn = c.lay[1] == 'n';
  const int64_t pa = c.pitch_a ? c.pitch_a : (at ? c.M : c.K) + 8;
  const int64_t pb = c.pitch_b ? c.pitch_b : (bn ? c.N : c.K) + 8;
  const int64_t ldc = c.ldc ? c.ldc : c.N + 8;
  const int64_t sam = at ? 1 : pa, sak = at ? pa : 1, sbk = bn ? pb : 1, sbn = bn ? 1 : pb;
  size_t wsb = c.ws ? ptd::gemm_bf16_workspace_bytes(c.M, c.N, c.K) : 0;
  if (c.ws == 2 && wsb) --wsb;
  if (c.ws == 4) wsb = 0;
  void* ws = wsb || c.ws == 4 ? fake(0x40000000, c.ws == 3 ? 4 : 0) : nullptr;
  ptd::g_launch_trace.on = true;
  ptd::g_launch_trace.count = 0;
  g_launches.clear();
  const auto fn = el ? ptd::gemm_f16 : ptd::gemm_bf16;
  const int rc = fn(fake(0x10000000, c.off_a), sam, sak, fake(0x20000000, c.off_b), sbk, sbn, fake(0x30000000, c.off_c), ldc,
                    c.M, c.N, c.K, c16, c.alpha, c.bias ? fake(0x50000000, 0) : nullptr, ws, wsb, nullptr, c.kv, c.nv);
  printf("%s %lld %lld %lld %d", el ? "h" : "b", (long long)c.M, (long long)c.N, (long long)c.K, c16 ? 16 : 32);
  if (strcmp(c.lay, "nt")) printf(" %s", c.lay);
  if (c.pitch_a) printf(" pa=%lld", (long long)c.pitch_a);
  if (c.pitch_b) printf(" pb=%lld", (long long)c.pitch_b);
  if (c.ldc) printf(" ldc=%lld", (long long)c.ldc);
  if (c.off_a) printf(" A+%d", c.off_a);
  if (c.off_b) printf(" B+%d", c.off_b);
  if (c.off_c) printf(" C+%d", c.off_c);
  if (c.ws) printf(" ws%s=%zu", c.ws == 2 ? "-1" : c.ws == 3 ? "+4" : c.ws == 4 ? "ptr" : "", wsb);
  if (c.bias) printf(" bias");
  if (c.alpha != 1.0) printf(" al=%g", c.alpha);
  if (c.kv) printf(" kv=%lld", (long long)c.kv);
  if (c.nv) printf(" nv=%lld", (long long)c.nv);
  printf(" > %d", rc);
  for (int i = 0; i < ptd::g_launch_trace.count && i < 32; ++i) printf("%s %s", i ? ";" : "", ptd::g_launch_trace.what[i]);
  printf("%s\n", g_launches.c_str());
}

Case shape(int64_t M, int64_t N, int64_t K, int ws = 0) {
  Case c{};
  c.M = M; c.N = N; c.K = K; c.ws = ws;
  return c;
}

// the cases of tests/test_gemm_routes_gpu.py, the instance variants of each family, the error exits and the guards
std::vector<Case> named_cases() {
  std::vector<Case> v;
  auto add = [&](Case c) { v.push_back(c); return &v.back(); };
  // one per family, as the GPU route test has them
  add(shape(2048, 768, 512));                                   // 128 x 64 tiles
  add(shape(128, 128, 1024, 1));                                // split K, one tile
  add(shape(128, 128, 1024, 1))->ldc = 128 + 4;                 // ... 8 does not divide ldc
  add(shape(256, 64, 2048, 1));                                 // split K, N = 64
  add(shape(1536, 768, 3072, 1));                               // split K, 72 tiles
  add(shape(128, 128, 2048, 1));                                // split K, K / ks = 256
  add(shape(2048, 1024, 14336, 1));                             // split K of a long K ahead of the 128 x 64 tiles
  add(shape(2048, 1024, 14336));                                // ... and without a workspace
  add(shape(2048, 1024, 4096, 1));                              // 128 x 64 tiles ahead of the split below K = 8192
  for (int kc = 1; kc <= 4; ++kc) add(shape(2048, 256, 64 * kc));          // short K, 256-column panel (K = 256: interleaved)
  for (double al : {1.0, 0.5})
    for (int bias = 0; bias < 2; ++bias) {
      if (al == 1.0 && !bias) continue;
      Case* c = add(shape(2048, 256, 256));
      c->alpha = al; c->bias = bias;
    }
  add(shape(2112, 512, 192));
  for (int kc = 1; kc <= 4; ++kc) add(shape(1024, 128, 64 * kc));          // short K, 128-column panel
  add(shape(1088, 384, 192));
  for (int kc = 1; kc <= 8; ++kc) add(shape(1024, 320, 64 * kc));          // short K, A panel
  add(shape(1152, 576, 512));
  add(shape(3584, 4096, 384));                                  // 256 x 256, 224 tiles
  add(shape(4352, 4096, 384));                                  // 256 x 256, 272 tiles
  add(shape(12288, 512, 576));                                  // 128 x 256
  add(shape(8192, 768, 704));
  add(shape(128, 128, 256));                                    // LDS-DMA, 4 buffers
  add(shape(896, 896, 1088));
  add(shape(256, 384, 192));                                    // LDS-DMA, 2 buffers
  add(shape(2176, 2048, 576));
  for (const char* lay : {"nn", "nt", "tn", "tt"}) add(shape(130, 257, 33))->lay = lay;     // generic
  for (const char* lay : {"nn", "tn", "tt"}) {                  // every tile family wants the nn.Linear layout
    add(shape(3584, 4096, 384))->lay = lay;
    add(shape(896, 896, 1088))->lay = lay;
  }
  { Case* c = add(shape(129, 72, 33)); c->pitch_a = c->pitch_b = 40; }
  // partial N and partial K ranges
  add(shape(1024, 64, 512))->nv = 8;
  add(shape(1024, 256, 512))->nv = 200;
  add(shape(1024, 256, 192))->nv = 200;                         // K < 256: no LDS-DMA shape
  add(shape(1024, 192, 512))->nv = 100;                         // N neither 64 nor a multiple of 128
  add(shape(128, 64, 4096, 1))->nv = 56;                        // the split is tried before the partial-N branch
  add(shape(128, 64, 4096))->nv = 56;
  add(shape(2048, 768, 512))->nv = 700;                         // no 128 x 64 tiles with a partial range
  add(shape(2048, 256, 256))->kv = 200;
  add(shape(2048, 256, 192))->kv = 136;
  add(shape(1024, 128, 128))->kv = 72;
  add(shape(1024, 320, 256))->kv = 200;
  add(shape(2048, 256, 320))->kv = 312;                         // K > 256
  add(shape(1024, 320, 320))->kv = 312;
  add(shape(2048, 256, 256))->kv = 250;                         // 8 does not divide kvalid
  add(shape(2048, 256, 160))->kv = 152;                         // 64 does not divide K
  add(shape(128, 128, 256))->kv = 200;                          // no short-K shape
  add(shape(1024, 192, 256))->kv = 200;
  add(shape(2048, 768, 512))->kv = 504;                         // no 128 x 64 tiles with a partial range either
  add(shape(2048, 768, 512))->kv = 512;                         // ... nor with kvalid = K or nvalid = N: the branch asks for 0
  add(shape(2048, 768, 512))->nv = 768;
  add(shape(2048, 256, 256))->kv = 256;                         // kvalid = K and nvalid = N: the whole range
  add(shape(1024, 256, 512))->nv = 256;
  // guards: bases off by 2 bytes, pitches that are no multiple of 8 elements, ldc = N + 1
  const Case bases[] = {shape(2048, 768, 512), shape(128, 128, 1024, 1), shape(2048, 256, 64), shape(2048, 256, 256),
                        shape(1024, 128, 64), shape(1024, 320, 320), shape(3584, 4096, 384), shape(12288, 512, 576),
                        shape(896, 896, 1088), shape(2176, 2048, 576)};
  for (const Case& b : bases) {
    add(b)->off_a = 2;
    add(b)->off_b = 2;
    add(b)->off_c = 2;
    add(b)->pitch_a = b.K + 4;
    add(b)->pitch_b = b.K + 4;
    add(b)->ldc = b.N + 1;
    add(b)->ldc = b.N + 4;
  }
  // the workspace: none, one byte short, 4 bytes off
  for (const Case& b : {shape(128, 128, 1024), shape(256, 64, 2048), shape(1536, 768, 3072)}) {
    add(b);
    add(b)->ws = 2;
    add(b)->ws = 3;
  }
  // (an oddity that is kept: a long K with ANY workspace pointer declines the 128 x 64 tiles, usable or not)
  add(shape(2048, 1024, 14336))->ws = 2;
  add(shape(2048, 1024, 14336))->ws = 4;
  add(shape(2048, 1024, 4096))->ws = 4;
  // degenerate sizes
  add(shape(0, 128, 128));
  add(shape(128, 0, 128));
  add(shape(1, 128, 128));
  add(shape(128, 1, 128));
  add(shape(128, 128, 1));
  add(shape(128, 128, 0));
  // the 32-bit offset limits of the kernels that keep per-lane offsets
  for (const Case& b : {shape(2048, 256, 64), shape(2048, 256, 256)}) {
    add(b)->pitch_a = (1 << 24) - 8;
    add(b)->pitch_a = 1 << 24;
    add(b)->ldc = (1 << 23) - 8;
    add(b)->ldc = 1 << 23;
  }
  for (const Case& b : {shape(3584, 4096, 384), shape(12288, 512, 576)}) {
    add(b)->pitch_a = (1 << 22) - 8;
    add(b)->pitch_a = 1 << 22;
    add(b)->pitch_b = (1 << 22) - 8;
    add(b)->pitch_b = 1 << 22;
  }
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  const bool named_only = argc > 1 && !strcmp(argv[1], "named");
  for (const Case& c : named_cases())
    for (int el = 0; el < 2; ++el)
      for (int c16 = 1; c16 >= 0; --c16) run(c, el, c16);
  if (named_only) return 0;
  // the lattice: bf16, both outputs, with the workspace wherever one is asked for; partial ranges with 16-bit output
  const int64_t Ms[] = {128, 1024, 2048, 4352, 12288};
  const int64_t Ns[] = {64, 128, 256, 512, 768, 4096};
  const int64_t Ks[] = {64, 192, 256, 320, 384, 512, 576, 1024, 4096, 8192};
  for (int64_t M : Ms)
    for (int64_t N : Ns)
      for (int64_t K : Ks) {
        const bool has_ws = ptd::gemm_bf16_workspace_bytes(M, N, K) > 0;
        for (int c16 = 1; c16 >= 0; --c16) {
          run(shape(M, N, K), 0, c16);
          if (has_ws) run(shape(M, N, K, 1), 0, c16);
        }
        Case c = shape(M, N, K, has_ws);
        c.nv = N - 8;
        run(c, 0, true);
        if (K <= 256) {
          c = shape(M, N, K);
          c.kv = K - 8;
          run(c, 0, true);
        }
      }
  return 0;
}
