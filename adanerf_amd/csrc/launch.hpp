// Shared by the two launching translation units: picking a kernel instantiation by a run-time value, sizing a persistent grid.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <type_traits>

#include "layout.hpp"
#include "params.hpp"

namespace adanerf {

// f(std::integral_constant<.., V>{}) for the V among Vs that equals v, else `none`.  The call site lists the admissible values, so
// exactly the kernels it names are instantiated: dispatch<64, 128, 256>(width, [&](auto w) { return launch(kernel<w()>); }, error)
template <auto... Vs, typename T, typename F, typename R>
R dispatch(T v, F&& f, R none) {
  (void)((v == static_cast<T>(Vs) ? (none = f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) || ...);
  return none;
}

// frequency bands (positions, directions) of the slot layout kEnc*: template arguments of the kernels
constexpr int enc_fp(int enc) { return enc == kEnc10_4 ? 10 : enc == kEnc2_2 ? 2 : kMaxBands; }
constexpr int enc_fd(int enc) { return enc == kEnc10_4 ? 4 : enc == kEnc2_2 ? 2 : kMaxBands; }

// Resident workgroups of each persistent kernel on one device, asked of the occupancy API once per kernel.
struct GridCache {
  int compute_units = 0;
  std::map<const void*, int> resident;
};

template <typename K>
hipError_t persistent_grid(GridCache& gc, K kernel, int threads, int* grid) {
  int& g = gc.resident[reinterpret_cast<const void*>(kernel)];
  if (!g) {
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0);
    if (e != hipSuccess) return e;
    g = std::max(per_cu, 1) * gc.compute_units;
  }
  *grid = g;
  return hipSuccess;
}

// `tiles` units of work on at most the resident workgroups (the kernel strides over its tiles); the caller asks hipGetLastError()
template <typename K, typename... Args>
hipError_t launch_persistent(GridCache& gc, K kernel, int tiles, int threads, hipStream_t stream, const Args&... args) {
  int grid = 0;
  const hipError_t e = persistent_grid(gc, kernel, threads, &grid);
  if (e == hipSuccess) hipLaunchKernelGGL(kernel, dim3(std::min(tiles, grid)), dim3(threads), 0, stream, args...);
  return e;
}

}  // namespace adanerf
