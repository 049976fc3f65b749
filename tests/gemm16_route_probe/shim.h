// Force-included (-include) into a HOST-ONLY compile of ptdeco_amd/csrc/gemm_bf16.hip or gemm_f64.hip: every launch becomes a
// call of a recorder, so the router can be driven on a machine without a GPU and without a HIP runtime.
// The recorder gets the kernel's handle (the test names the exact template instance from it), the grid, the block and
// the trailing launch arguments of arithmetic type.  Pointers are skipped, and so are structs: they have padding.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

void ptd_probe_launch(const void* kernel, dim3 grid, dim3 block);
void ptd_probe_int(long long v);
void ptd_probe_real(double v);

template <typename T>
inline void ptd_probe_arg(const T& v) {
  if constexpr (std::is_integral_v<T>) ptd_probe_int((long long)v);
  else if constexpr (std::is_floating_point_v<T>) ptd_probe_real((double)v);
}

template <typename... Ts>
inline void ptd_probe_record(const void* kernel, dim3 grid, dim3 block, const Ts&... args) {
  ptd_probe_launch(kernel, grid, block);
  (ptd_probe_arg(args), ...);
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, shmem, stream, ...) \
  ptd_probe_record(reinterpret_cast<const void*>(k), dim3(g), dim3(b), ##__VA_ARGS__)
#define hipGetLastError() hipSuccess
