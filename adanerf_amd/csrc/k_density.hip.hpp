// N10: foveated ray density (adanerf_foveate_density / adanerf_fill_density and their _phased forms, of which the unphased ones are
// phase (0, 0)) -- the two kernels either side of adanerf_render_masked.
//   density_mask_kernel  the byte mask of a gaze point and rings of strides 1 / 2 / 4 / 8 (density_rule.hpp, shared with the host mirror):
//                        0 = render this pixel, else the pixel's stride.  Four pixels and one 4-byte store per thread where the mask
//                        pointer is 4-byte aligned (a wave then writes 256 contiguous bytes, not 64), single bytes otherwise and at the end.
//   density_fill_kernel  every pixel whose byte is 2, 4 or 8 becomes the bilinear blend of the rendered corners of its stride's cell, in
//                        place, in up to four images.  One thread per pixel, consecutive lanes along a row: the lanes of one cell read the
//                        same corner addresses, so a wave in the stride-8 region asks for at most 9 + 9 distinct pixels, all within the 768
//                        bytes of its two corner rows (the rendered pixels are a fifth of the frame and stay in L2); the mask bytes and
//                        the stores are contiguous per wave.  A thread reads only pixels of byte 0 and writes only pixels of another
//                        byte: no thread reads what another writes, whatever the mask holds.  No LDS.
// Every blend step is one rounded fp32 operation (-ffp-contract=off and the _rn intrinsics: never fused), so the kernel is exact against
// a numpy float32 restatement (tests/density_reference.py).
#pragma once
#include "k_common.hip.hpp"
#include "k_accumulate.hip.hpp"
#include "density_rule.hpp"

namespace adanerf {

__global__ __launch_bounds__(256) void density_mask_kernel(DensityRule f, int w, int h, int aligned4, uint8_t* __restrict__ mask) {
  const int n = w * h;      // <= 2^28 (sides <= 16384): pixel indices are 32-bit, divided as unsigned
  const int p0 = 4 * (static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x));
  if (p0 >= n) return;
  int y = static_cast<int>(static_cast<uint32_t>(p0) / static_cast<uint32_t>(w)), x = p0 - y * w;
  const int cnt = n - p0 < 4 ? n - p0 : 4;
  uint32_t word = 0u;
  for (int k = 0; k < cnt; ++k) {
    word |= static_cast<uint32_t>(density_mask_byte(f, x, y, w, h)) << (8 * k);
    if (++x == w) {
      x = 0;
      ++y;
    }
  }
  if (aligned4 && cnt == 4) {
    *reinterpret_cast<uint32_t*>(mask + p0) = word;
  } else {
    for (int k = 0; k < cnt; ++k) mask[p0 + k] = static_cast<uint8_t>(word >> (8 * k));
  }
}

// the images adanerf_fill_density works on; all but rgb may be null
struct DensityFill {
  const uint8_t* mask;      // [h*w]
  float* rgb;               // [h*w,3]
  float* depth;             // [h*w]
  float* acc;               // [h*w]
  uchar4* rgba8;            // [h*w]
  int32_t* unfilled;        // the pixels left untouched because a corner of theirs was not rendered (zeroed before the launch)
};

// c00 + fx (c01 - c00), then the same between the two rows; an axis whose two taps are one pixel copies the value's bits
__device__ __forceinline__ float density_blend(float c00, float c01, float c10, float c11, float fx, float fy, bool two_x, bool two_y) {
  const float top = two_x ? __fadd_rn(c00, __fmul_rn(fx, __fsub_rn(c01, c00))) : c00;
  if (!two_y) return top;
  const float bot = two_x ? __fadd_rn(c10, __fmul_rn(fx, __fsub_rn(c11, c10))) : c10;
  return __fadd_rn(top, __fmul_rn(fy, __fsub_rn(bot, top)));
}

__global__ __launch_bounds__(256) void density_fill_kernel(DensityFill d, int w, int h, int phase_x, int phase_y) {
  const int n = w * h;      // <= 2^28 (sides <= 16384): 3 n values fit 32 bits too
  const int p = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  const int s = p < n ? d.mask[p] : 0;
  bool missing = false;
  if (s == 2 || s == 4 || s == 8) {
    const int y = static_cast<int>(static_cast<uint32_t>(p) / static_cast<uint32_t>(w)), x = p - y * w;
    const DensityAxis ax = density_cell_axis(x, phase_x, s, w), ay = density_cell_axis(y, phase_y, s, h);
    const bool two_x = ax.c1 != ax.c0, two_y = ay.c1 != ay.c0;
    missing = ax.none || ay.none;      // a frame narrower than the stride: no corner on that axis, nothing is read
    const int i00 = ay.c0 * w + ax.c0, i01 = ay.c0 * w + ax.c1, i10 = ay.c1 * w + ax.c0, i11 = ay.c1 * w + ax.c1;
    // the corners that are not distinct repeat one that is: their bytes are looked at twice, nothing more
    if (!missing) missing = (d.mask[i00] | d.mask[i01] | d.mask[i10] | d.mask[i11]) != 0;
    if (!missing) {
      const float inv_s = s == 2 ? 0.5f : (s == 4 ? 0.25f : 0.125f);      // m / s, exact: s is a power of two
      const float fx = static_cast<float>(ax.m) * inv_s, fy = static_cast<float>(ay.m) * inv_s;
      float out[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        out[ch] = density_blend(d.rgb[3 * i00 + ch], d.rgb[3 * i01 + ch], d.rgb[3 * i10 + ch], d.rgb[3 * i11 + ch], fx, fy, two_x, two_y);
      d.rgb[3 * p] = out[0];
      d.rgb[3 * p + 1] = out[1];
      d.rgb[3 * p + 2] = out[2];
      if (d.depth) d.depth[p] = density_blend(d.depth[i00], d.depth[i01], d.depth[i10], d.depth[i11], fx, fy, two_x, two_y);
      if (d.acc) d.acc[p] = density_blend(d.acc[i00], d.acc[i01], d.acc[i10], d.acc[i11], fx, fy, two_x, two_y);
      if (d.rgba8) d.rgba8[p] = rgba8_of(out[0], out[1], out[2]);
    }
  }
  const uint64_t lost = __ballot(missing);      // one atomic per wave that has any
  if (lost && lane_id() == __ffsll(static_cast<unsigned long long>(lost)) - 1) atomicAdd(d.unfilled, __popcll(lost));
}

}  // namespace adanerf
