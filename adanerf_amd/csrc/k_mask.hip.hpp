// N8: masked rendering (adanerf_render_masked) -- the two small kernels around the unchanged render path.
//   mask_bits_kernel     the caller's byte mask -> one bit per pixel, 32 pixels per word: the form refine_list_kernel (k_compact.hip.hpp)
//                        turns into an ascending list of ray ids and their count, every workgroup tallying what lies in front of it from
//                        the bit words in L2 (80 KB at 800 x 800) -- no workgroup waits on another, the order is that of the pixels
//   mask_scatter_kernel  the finished pixels of a listed batch (compact staging buffers, written by the compositing kernels exactly as
//                        they write a batch of a whole frame) -> the caller's images at the listed positions
// Between them the sampling kernel reads its ray ids from the list (SampleArgs::ray_list) and every later stage sees an ordinary batch.
#pragma once
#include "k_common.hip.hpp"

namespace adanerf {

// One thread per 16 pixels: a 16-byte load where the 16 bytes exist and are aligned (aligned16: the mask pointer is), single bytes for a
// partial last group and for a misaligned mask; the thread's 16 bits are half a word of `bits` (little-endian: pixel 32 w + b is bit b of
// word w).  Launched over 2 x n_words threads, so the bits behind the last pixel of the last word are written too, as zeros.
__global__ __launch_bounds__(256) void mask_bits_kernel(const uint8_t* __restrict__ mask, int n, uint32_t values, int aligned16, int n_halves,
                                                        uint16_t* __restrict__ bits) {
  const int t = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
  if (t >= n_halves) return;
  const int p0 = t * 16;
  uint32_t out = 0u;
  if (aligned16 && p0 + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(mask + p0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int b = 0; b < 4; ++b) out |= mask_selects((w[k] >> (8 * b)) & 0xFFu, values) << (4 * k + b);
  } else {
    for (int b = 0; b < 16 && p0 + b < n; ++b) out |= mask_selects(mask[p0 + b], values) << b;
  }
  bits[t] = static_cast<uint16_t>(out);
}

// The staging buffers of a listed batch and the images they belong in; every pair is optional (null destination: not written).
struct MaskScatter {
  const int32_t* list;      // [n] ray ids of the batch's rays, ascending
  const uint32_t* rgba8;    // [n] staged
  const float* rgb;         // [n,3]
  const float* depth;       // [n]
  const float* acc;         // [n]
  const float* disp;        // [n]
  uint32_t* o_rgba8;        // [rays_local] the caller's
  float* o_rgb;
  float* o_depth;
  float* o_acc;
  float* o_disp;
};

// one thread per listed ray; the bits move unchanged
__global__ __launch_bounds__(256) void mask_scatter_kernel(MaskScatter s, int n) {
  const int i = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const size_t r = static_cast<size_t>(s.list[i]);
  if (s.o_rgba8) s.o_rgba8[r] = s.rgba8[i];
  if (s.o_rgb) {
    const float x = s.rgb[3 * static_cast<size_t>(i)], y = s.rgb[3 * static_cast<size_t>(i) + 1], z = s.rgb[3 * static_cast<size_t>(i) + 2];
    s.o_rgb[3 * r] = x;
    s.o_rgb[3 * r + 1] = y;
    s.o_rgb[3 * r + 2] = z;
  }
  if (s.o_depth) s.o_depth[r] = s.depth[i];
  if (s.o_acc) s.o_acc[r] = s.acc[i];
  if (s.o_disp) s.o_disp[r] = s.disp[i];
}

}  // namespace adanerf
