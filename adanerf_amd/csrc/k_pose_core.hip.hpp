// The arithmetic that carries a pixel to another camera pose, each expression written once: what the reprojection (k_reproject.hip.hpp)
// and the three temporal resolves (k_temporal.hip.hpp, k_upsample.hip.hpp, k_sparse_temporal.hip.hpp) have in common.  The numbers are
// the steps of the kernels' header comments and of the numpy restatements (tests/*_reference.py):
//   2  camera_depth                   a point's depth in a camera: row 2 of its c2w against P - pos
//   3  to_camera, image_coord, nearest_tap   q into a camera's space; onto its image; the pixel it falls in
//   5  bilinear_history               four bilinear taps of the history's colour, clamped at the border
//   6  temporal_min, temporal_max     the order of the 3 x 3 clamp
//   8  blend_toward                   history + a_eff x (current - history), one channel
//      count_in_block                 a block's count of flagged pixels: one atomicAdd
// Every floating-point operation is a single rounded fp32 operation in a fixed order (-ffp-contract=off and the _rn intrinsics): a change
// here changes every kernel above at once, and each is exact against its own restatement.
// What is NOT here, and why: a step moved here only where the kernels' gfx950 code stayed what it was (tools/isa_diff.py: identical, or
// other register numbers only; profiles/pose_core_isa_identity.md has the table and what was tried).  Values come back as return values
// where they can: a helper that fills a caller's array, or that reads the kernel's parameter struct where the kernel itself no longer
// does, changes when the optimiser splits those objects and with that the order of the loads, although never a result.  So step 2's
// surface (gen_ray, origin, near test, P), step 3's q and its inside test, step 4's depth range, the LDS staging, the clamp's loop and the
// output stores are still written in each kernel.
// Device code only (gfx950, wave64).
#pragma once
#include "k_accumulate.hip.hpp"      // rgba8_of, for the resolves that include this file
#include "k_common.hip.hpp"

namespace adanerf {

// ---- 2: the depth of P in the camera (pos, row-major c2w rot) --------------------------------------------------------------------------
__device__ __forceinline__ float camera_depth(const float (&pos)[3], const float (&rot)[9], const float (&P)[3]) {
  const float q0 = __fsub_rn(P[0], pos[0]), q1 = __fsub_rn(P[1], pos[1]), q2 = __fsub_rn(P[2], pos[2]);
  return -__fadd_rn(__fadd_rn(__fmul_rn(rot[2], q0), __fmul_rn(rot[5], q1)), __fmul_rn(rot[8], q2));
}

// ---- 3: the other camera ---------------------------------------------------------------------------------------------------------------
// v = q (a point less the camera's position, or a far pixel's direction) in the camera space of the row-major c2w rot: its transpose on q
__device__ __forceinline__ void to_camera(const float (&rot)[9], const float (&q)[3], float v[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = __fadd_rn(__fadd_rn(__fmul_rn(rot[k], q[0]), __fmul_rn(rot[3 + k], q[1])), __fmul_rn(rot[6 + k], q[2]));
}
// the image coordinate of camera-space x (v[0], or -v[1] down the rows) at depth zc > 0 on an axis of `size` pixels
__device__ __forceinline__ float image_coord(float focal, float x, float zc, float size) {
  return __fadd_rn(__fmul_rn(focal, x) / zc, __fmul_rn(0.5f, size));
}
// the pixel (u, vv) falls in; 0 <= u < w and 0 <= vv < h (the caller's inside test): floorf(u) <= u < w, so it is inside
__device__ __forceinline__ int nearest_tap(float u, float vv, int w) { return static_cast<int>(floorf(vv)) * w + static_cast<int>(floorf(u)); }

// ---- 5: hst = hist_rgb [H, W, 3] at (u, vv), bilinear between pixel centres, the taps clamped to the image ------------------------------
__device__ __forceinline__ void bilinear_history(const float* __restrict__ hist_rgb, int W, int H, float u, float vv, float hst[3]) {
  const float fx = __fsub_rn(u, 0.5f), fy = __fsub_rn(vv, 0.5f);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float wx = __fsub_rn(fx, x0f), wy = __fsub_rn(fy, y0f);
  const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);      // -1 .. W - 1
  const int xa = max(x0, 0), xb = min(x0 + 1, W - 1), ya = max(y0, 0), yb = min(y0 + 1, H - 1);
  const float* h00 = hist_rgb + 3 * (ya * W + xa);
  const float* h01 = hist_rgb + 3 * (ya * W + xb);
  const float* h10 = hist_rgb + 3 * (yb * W + xa);
  const float* h11 = hist_rgb + 3 * (yb * W + xb);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float top = __fadd_rn(h00[k], __fmul_rn(wx, __fsub_rn(h01[k], h00[k])));
    const float bot = __fadd_rn(h10[k], __fmul_rn(wx, __fsub_rn(h11[k], h10[k])));
    hst[k] = __fadd_rn(top, __fmul_rn(wy, __fsub_rn(bot, top)));
  }
}

// ---- 6: the order of the clamp ---------------------------------------------------------------------------------------------------------
// A NaN is skipped (both NaN: a NaN), otherwise the floats order as sign-magnitude integers, so -0 < +0.
// v_min_f32 / v_max_f32 do not promise the signed-zero order, hence integers.
__device__ __forceinline__ int32_t temporal_order_key(float f) {
  const int32_t b = __float_as_int(f);
  return b ^ ((b >> 31) & 0x7FFFFFFF);
}
__device__ __forceinline__ float temporal_min(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  return temporal_order_key(b) < temporal_order_key(a) ? b : a;
}
__device__ __forceinline__ float temporal_max(float a, float b) {
  if (a != a) return b;
  if (b != b) return a;
  return temporal_order_key(b) > temporal_order_key(a) ? b : a;
}

// ---- 8: one channel of the blend -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float blend_toward(float hst, float c, float a_eff) { return __fadd_rn(hst, __fmul_rn(a_eff, __fsub_rn(c, hst))); }

// ---- *counter += the threads of the block (256, and all of them call) whose flag is 1 ---------------------------------------------------
// a DPP sum per wave, four LDS slots, one atomicAdd per block that has any
__device__ __forceinline__ void count_in_block(int flag, int32_t* __restrict__ counter) {
  __shared__ int wave_count[4];
  const int tid = static_cast<int>(threadIdx.x);
  const int in_wave = wave_sum_dpp_i32(flag);
  if (lane_id() == 0) wave_count[tid >> 6] = in_wave;
  __syncthreads();
  if (tid == 0) {
    const int in_block = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
    if (in_block) atomicAdd(counter, in_block);
  }
}

}  // namespace adanerf
