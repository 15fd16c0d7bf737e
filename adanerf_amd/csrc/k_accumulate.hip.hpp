// N5: supersampling in time -- the running sum of several sub-pixel frames (adanerf_set_pixel_offset) and its mean.  The viewer has no
// counterpart: its ray table is fixed to pixel centres (src/util/raygeneration.py:10-26).  Every value is one rounded fp32 operation
// (a sum, or an IEEE division by the frame count), so the kernels are exact against a numpy float32 restatement
// (tests/antialias_reference.py).  The 8-bit image follows the viewer's output contract as the compositing kernels write it
// (k_composite.hip.hpp: (uchar)(clamp(v, 0, 1) * 255), A = 255), so the mean of one frame is that frame byte for byte.
// Bandwidth-bound and tiny beside a frame's two networks: grid-stride over the values, a thread per pixel in the resolve.  No LDS.
#pragma once
#include "k_common.hip.hpp"

namespace adanerf {

// the viewer's output contract for one pixel (adaptive_cuda_kernels.cu:846-851): a NaN becomes 0
__device__ __forceinline__ uchar4 rgba8_of(float r, float g, float b) {
  uchar4 px;
  px.x = static_cast<unsigned char>(fminf(fmaxf(r, 0.f), 1.f) * 255.0f);
  px.y = static_cast<unsigned char>(fminf(fmaxf(g, 0.f), 1.f) * 255.0f);
  px.z = static_cast<unsigned char>(fminf(fmaxf(b, 0.f), 1.f) * 255.0f);
  px.w = 255;
  return px;
}

// Each pair of kernels below is one body: Masked adds the test of a byte mask (mask_selects, k_common.hip.hpp: the test of
// adanerf_render_masked), and nothing of a pixel the mask does not select is read or written.

// sum[i] = rgb[i] (first) or sum[i] + rgb[i]; rgb may be sum itself.  Value i belongs to pixel i / 3.
template <bool Masked>
__device__ __forceinline__ void accumulate_value(int64_t i, const float* rgb, const uint8_t* __restrict__ mask, uint32_t values, float* sum, int first) {
  if (Masked && !mask_selects(mask[static_cast<uint32_t>(i) / 3u], values)) return;
  const float v = rgb[i];
  sum[i] = first ? v : __fadd_rn(sum[i], v);
}

// pixel r: m = sum / frames per channel -> rgb_out [n_rays,3] (may be sum itself: a thread reads its three values before it writes them)
// and rgba8_out [n_rays]; either may be null.  Every element of a pixel the mask does not select keeps its bytes in both outputs.
template <bool Masked>
__device__ __forceinline__ void resolve_mean_pixel(const float* sum, const uint8_t* __restrict__ mask, uint32_t values, int n_rays, float frames,
                                                   float* rgb_out, uchar4* __restrict__ rgba8_out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rays || (Masked && !mask_selects(mask[r], values))) return;
  const size_t o = 3 * static_cast<size_t>(r);
  const float m0 = __fdiv_rn(sum[o], frames), m1 = __fdiv_rn(sum[o + 1], frames), m2 = __fdiv_rn(sum[o + 2], frames);
  if (rgb_out) {
    rgb_out[o] = m0;
    rgb_out[o + 1] = m1;
    rgb_out[o + 2] = m2;
  }
  if (rgba8_out) rgba8_out[r] = rgba8_of(m0, m1, m2);
}

// A thread per value, i < n, masked or not, so the loads and stores of a wave stay contiguous where the mask selects a run of pixels.  The
// grid-stride loop is written out in both kernels: inside a device function its blockDim.x costs a load and a select that a kernel folds away.
__global__ __launch_bounds__(256) void accumulate_kernel(const float* rgb, float* sum, int n, int first) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;      // 64-bit: i + stride passes 2^31 at the largest n
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) accumulate_value<false>(i, rgb, nullptr, 0, sum, first);
}
__global__ __launch_bounds__(256) void resolve_mean_kernel(const float* sum, int n_rays, float frames, float* rgb_out, uchar4* __restrict__ rgba8_out) {
  resolve_mean_pixel<false>(sum, nullptr, 0, n_rays, frames, rgb_out, rgba8_out);
}
// N11 (adaptive supersampling): the two for the pixels the mask selects
__global__ __launch_bounds__(256) void accumulate_masked_kernel(const float* rgb, const uint8_t* __restrict__ mask, uint32_t values, float* sum, int n, int first) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) accumulate_value<true>(i, rgb, mask, values, sum, first);
}
__global__ __launch_bounds__(256) void resolve_mean_masked_kernel(const float* sum, const uint8_t* __restrict__ mask, uint32_t values, int n_rays, float frames,
                                                                  float* rgb_out, uchar4* __restrict__ rgba8_out) {
  resolve_mean_pixel<true>(sum, mask, values, n_rays, frames, rgb_out, rgba8_out);
}

}  // namespace adanerf
