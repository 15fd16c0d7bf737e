// N9: hybrid rendering -- the rasterised colour behind a frame rendered under a depth limit (adanerf_set_depth_limit) let through with the
// transmittance the volume left: t = 1 - acc, !(t > 0) -> 0 (a NaN too), t > 1 -> 1; t == 0: out = rgb, the bits copied (a NaN in the
// behind image cannot leak); otherwise out_c = rgb_c + t * behind_c, a product, then a sum.  Every value is one rounded fp32 operation, so
// the kernel is exact against a numpy float32 restatement (tests/depth_limit_reference.py).  The 8-bit image follows
// adanerf_resolve_mean's byte contract (rgba8_of, k_accumulate.hip.hpp).  Bandwidth-bound: a thread per pixel, no LDS.
#pragma once
#include "k_common.hip.hpp"
#include "k_accumulate.hip.hpp"

namespace adanerf {

// rgb_out [n,3] may be rgb itself (a thread reads its three values before it writes them); either output may be null
__global__ __launch_bounds__(256) void blend_behind_kernel(const float* rgb, const float* __restrict__ acc, const float* __restrict__ behind, int n,
                                                           float* rgb_out, uchar4* __restrict__ rgba8_out) {
  const int r = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
  if (r >= n) return;
  const size_t o = 3 * static_cast<size_t>(r);
  float t = __fsub_rn(1.0f, acc[r]);
  if (!(t > 0.f)) t = 0.f;
  if (t > 1.f) t = 1.f;
  float c0 = rgb[o], c1 = rgb[o + 1], c2 = rgb[o + 2];
  if (t != 0.f) {
    c0 = __fadd_rn(c0, __fmul_rn(t, behind[o]));
    c1 = __fadd_rn(c1, __fmul_rn(t, behind[o + 1]));
    c2 = __fadd_rn(c2, __fmul_rn(t, behind[o + 2]));
  }
  if (rgb_out) {
    rgb_out[o] = c0;
    rgb_out[o + 1] = c1;
    rgb_out[o + 2] = c2;
  }
  if (rgba8_out) rgba8_out[r] = rgba8_of(c0, c1, c2);
}

}  // namespace adanerf
