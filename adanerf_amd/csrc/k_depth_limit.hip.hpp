// A4c: per-ray depth limits (adanerf_set_depth_limit): a ray stops at the depth a rasteriser reports for its pixel.  A second trim of the
// rows the selection left in selbin / selw, after the budget trim (k_budget.hip.hpp) and before expand_kernel: entry k of ray r, bin b, is
// dropped iff zc >= L_r, with z = ztab[b], P = o + d z (a product, then a sum: the first line of sample_position), q = P - pos,
// zc = -((R[2] q_0 + R[5] q_1) + R[8] q_2) -- every operation one rounded fp32 operation in this order (tests/depth_limit_reference.py).
// A NaN limit keeps the row, a NaN zc is kept, equality drops; no entry is kept as a fallback, so a row may become empty.  Survivors stay
// in ascending bin order with their selw untouched; counts[r] is replaced only when the row shrank; the segment totals expand_kernel
// reads are recomputed as at the tail of trim_rows_kernel -- integer sums in a fixed order, no atomics: the same inputs give the same bytes.
// Measured at N = 8: 11.3 us for 640 000 rays, trim_rows_kernel in the same trace 25.1 us (profiles/depth_limit_measured.md).
// Device code only (gfx950, wave64); part of kernels.hip.hpp.
#pragma once
#include "k_common.hip.hpp"

namespace adanerf {

// the pose in force (adanerf_set_camera): position and the third column of rot_c2w, the camera's -viewing axis
struct DepthPose {
  float pos[3];
  float r2, r5, r8;
};

// One thread per ray, any n_max <= 128: the row is walked with plain loads and survivors are written at pos <= k, in place (an entry never
// overwrites one that is still to be read).  2^seg_shift rays per entry of seg_total (32 or 64), as trim_rows_kernel.  rays: the [n,8]
// records the sampling kernel wrote for this batch.  Ray i of the batch reads limit[map_first + i], with a list limit[map_first + list[i]]
// (adanerf_render_masked: the batch is the listed rays, the map is indexed by frame position).
__global__ __launch_bounds__(256) void depth_limit_kernel(int32_t* __restrict__ counts, uint8_t* __restrict__ selbin, float* __restrict__ selw,
                                                          const float* __restrict__ rays, const float* __restrict__ limit,
                                                          const int32_t* __restrict__ list, int map_first, DepthPose pose,
                                                          const float* __restrict__ ztab, int n_rays, int n_max, int seg_shift,
                                                          int32_t* __restrict__ seg_total) {
  const int r = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
  const int c = r < n_rays ? min(counts[r], n_max) : 0;
  int kept = c;
  if (c > 0) {
    const float L = limit[map_first + (list ? list[r] : r)];
    if (L == L) {      // a NaN limit drops nothing
      const float4 o4 = reinterpret_cast<const float4*>(rays)[2 * static_cast<size_t>(r)];
      const float4 d4 = reinterpret_cast<const float4*>(rays)[2 * static_cast<size_t>(r) + 1];
      const size_t o = static_cast<size_t>(r) * n_max;
      int pos = 0;
      for (int k = 0; k < c; ++k) {
        const uint8_t b = selbin[o + k];
        const float z = ztab[b & 127];
        const float q0 = __fsub_rn(__fadd_rn(o4.x, __fmul_rn(d4.x, z)), pose.pos[0]);
        const float q1 = __fsub_rn(__fadd_rn(o4.y, __fmul_rn(d4.y, z)), pose.pos[1]);
        const float q2 = __fsub_rn(__fadd_rn(o4.z, __fmul_rn(d4.z, z)), pose.pos[2]);
        const float zc = -__fadd_rn(__fadd_rn(__fmul_rn(pose.r2, q0), __fmul_rn(pose.r5, q1)), __fmul_rn(pose.r8, q2));
        if (!(zc >= L)) {
          if (pos != k) {
            selbin[o + pos] = b;
            selw[o + pos] = selw[o + k];
          }
          ++pos;
        }
      }
      kept = pos;
      if (kept != c) counts[r] = kept;
    }
  }
  const int x = seg_shift == 5 ? wave_incl_sum_dpp_i32<32>(kept) : wave_incl_sum_dpp_i32<64>(kept);
  const int last = (1 << seg_shift) - 1;
  if ((static_cast<int>(threadIdx.x) & last) == last && (r & ~last) < n_rays) seg_total[r >> seg_shift] = x;
}

}  // namespace adanerf
