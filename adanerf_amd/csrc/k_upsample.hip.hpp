// N7: temporal upsampling -- the frame is rendered at w x h with a sub-pixel offset and resolved into a history of s w x s h: s^2 times
// fewer rays per displayed frame, the full-resolution image rebuilt over the s^2 offsets of the grid.  The temporal resolve
// (k_temporal.hip.hpp) with two sizes and a neighbourhood depth test; the viewer has no counterpart (it blits the frame it rendered).
// Two launches:
//   upsample_depth_kernel   (pass A) render pixel i -> zp[i], its surface's camera depth at the PREVIOUS pose (+inf: far).  Only when the
//                           history's depth is tested.
//   upsample_resolve_kernel (pass B) output pixel J -> the render pixel i whose jittered sample lies nearest its centre -> the surface along
//                           J's own full-resolution ray at i's depth -> the previous camera -> the history's nearest tap (depth against
//                           the range of zp over i's 3 x 3 neighbourhood, count) and four bilinear taps -> clamp to the current colour's
//                           3 x 3 neighbourhood -> blend with the sample's weight k.  A gather: nothing depends on the order of arrival.
// Pass B works on 32 x 8 output tiles.  At s >= 2 a render pixel is read by up to 9 s^2 threads, so the tile's render-size footprint plus a
// one-pixel halo goes through LDS: rows of 3 consecutive colour floats per pixel (read at a stride of 3 floats, free of bank conflicts
// as 3 is odd; the s threads that share a render pixel read one address, a broadcast) and a plane of zp.  The footprint's first column
// and row are those of the tile's first pixel: step 1's expression is monotone in X (each of its operations is correctly rounded, hence
// monotone).  Across 31 further output pixels floor(cx) grows by at most ceil(31 / s) + 1 -- the + 1 is the rounding's: with cx just below
// 1 at the first pixel, cx + 31 can round up to 32 -- so the footprint is ceil(31 / s) + 4 columns and ceil(7 / s) + 4 rows with the halo.
// A pixel outside the image is staged as a NaN: the clamp's rule skips it, and zp (finite or +inf by definition) reads it as "no such pixel".
// Every floating-point operation is a single rounded fp32 operation in a fixed order (-ffp-contract=off): exact against
// tests/upsample_reference.py.  The expressions shared with the other stages that change pose are k_pose_core.hip.hpp's; pass A and
// step 5 keep their own text (profiles/pose_core_isa_identity.md).  Device code only (gfx950, wave64); part of stages.hip.
#pragma once
#include "k_temporal.hip.hpp"

namespace adanerf {

constexpr int kUpsampleMaxScale = 4;
constexpr int kUpsampleMaxCols = 31 + 4, kUpsampleMaxRows = 7 + 4;      // the footprint at s = 1, the largest
constexpr int kUpsampleMaxPixels = kUpsampleMaxCols * kUpsampleMaxRows;

struct UpsampleParams {
  RayGenParams g_lo;        // the context's ray generator, the offset (cur_dx, cur_dy) applied, pos / rot = the CURRENT pose
  RayGenParams g_hi;        // the generator of the s w x s h frame at pixel centres, the same pose
  float prev_pos[3];
  float prev_rot[9];        // row-major c2w of the history's pose
  float alpha, depth_tol, acc_min;
  float cur_dx, cur_dy;
  int32_t scale;
  int32_t origin_is_camera; // 1: depths count from the camera position (ADANERF_SAMPLER_COARSE_FINE), 0: from the view-cell sphere exit
  int32_t clamp;            // ADANERF_TEMPORAL_CLAMP
};

// step 1 along one axis: the render pixel whose jittered sample lies nearest the centre of output pixel X
__device__ __forceinline__ int upsample_nearest(int X, float fs, float d, int n) {
  const float c = __fsub_rn((static_cast<float>(X) + 0.5f) / fs, d);
  return min(max(static_cast<int>(floorf(c)), 0), n - 1);
}

__global__ __launch_bounds__(256) void upsample_depth_kernel(UpsampleParams p, const float* __restrict__ cur_depth, const float* __restrict__ cur_acc,
                                                             float* __restrict__ zp) {
  const int w = p.g_lo.w, n = w * p.g_lo.h;      // w * h < 2^25
  const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const int y = i / w, x = i - y * w;
  float nds[3], o[3];
  gen_ray(p.g_lo, x, y, nds, o);
  if (p.origin_is_camera) {
    o[0] = p.g_lo.pos[0];
    o[1] = p.g_lo.pos[1];
    o[2] = p.g_lo.pos[2];
  }
  const float a = cur_acc[i];
  const float t = cur_depth[i] / a;
  const bool near = a >= p.acc_min && fabsf(t) < INFINITY && t > 0.f;      // a NaN fails every comparison: far
  float z = INFINITY;
  if (near) {
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = __fsub_rn(__fadd_rn(o[k], __fmul_rn(nds[k], t)), p.prev_pos[k]);
    z = -__fadd_rn(__fadd_rn(__fmul_rn(p.prev_rot[2], q[0]), __fmul_rn(p.prev_rot[5], q[1])), __fmul_rn(p.prev_rot[8], q[2]));
    if (!(fabsf(z) < INFINITY)) z = INFINITY;
  }
  zp[i] = z;
}

__global__ __launch_bounds__(256) void upsample_resolve_kernel(UpsampleParams p, const float* __restrict__ cur_rgb, const float* __restrict__ cur_depth,
                                                               const float* __restrict__ cur_acc, const float* __restrict__ zp,
                                                               const float* __restrict__ hist_rgb, const float* __restrict__ hist_depth,
                                                               const uint8_t* __restrict__ hist_count, float* __restrict__ out_rgb,
                                                               float* __restrict__ out_depth, uint8_t* __restrict__ out_count,
                                                               uchar4* __restrict__ out_rgba8, uint8_t* __restrict__ out_mask,
                                                               int32_t* __restrict__ rejected) {
  __shared__ float tile[kUpsampleMaxPixels * 3];
  __shared__ float ztile[kUpsampleMaxPixels];
  const int w = p.g_lo.w, h = p.g_lo.h, W = p.g_hi.w, H = p.g_hi.h;      // W * H < 2^25: 3 * W * H fits an int
  const int s = p.scale;
  const float fs = static_cast<float>(s);
  const int tid = static_cast<int>(threadIdx.x);
  const int tx = tid & (kTemporalTileW - 1), ty = tid >> 5;
  const int X_first = static_cast<int>(blockIdx.x) * kTemporalTileW, Y_first = static_cast<int>(blockIdx.y) * kTemporalTileH;
  const int X = X_first + tx, Y = Y_first + ty;
  const bool in_image = X < W && Y < H;
  const int J = Y * W + X;
  const bool depth_test = hist_rgb && hist_depth;      // uniform over the launch

  // the footprint: block-uniform first column / row (the halo's), run-time extent
  const int cols = (30 + s) / s + 4, rows = (6 + s) / s + 4;      // ceil(31 / s) + 4, ceil(7 / s) + 4
  const int fx0 = upsample_nearest(X_first, fs, p.cur_dx, w) - 1, fy0 = upsample_nearest(Y_first, fs, p.cur_dy, h) - 1;
  const int row_floats = cols * 3;
  for (int e = tid; e < row_floats * rows; e += 256) {
    const int r = e / row_floats, c = e - r * row_floats;
    const int px = fx0 + c / 3, py = fy0 + r;
    float v = __int_as_float(0x7FC00000);      // no such pixel: skipped as a NaN is
    if (px >= 0 && px < w && py >= 0 && py < h) v = cur_rgb[(py * w + fx0) * 3 + c];
    tile[e] = v;
  }
  if (depth_test) {
    for (int e = tid; e < cols * rows; e += 256) {
      const int r = e / cols, c = e - r * cols;
      const int px = fx0 + c, py = fy0 + r;
      float v = __int_as_float(0x7FC00000);      // no such pixel
      if (px >= 0 && px < w && py >= 0 && py < h) v = zp[py * w + px];
      ztile[e] = v;
    }
  }
  __syncthreads();

  int is_rejected = 0;
  if (in_image) {
    // 1 sample
    const int ix = upsample_nearest(X, fs, p.cur_dx, w), iy = upsample_nearest(Y, fs, p.cur_dy, h);
    const int i = iy * w + ix;
    const float ex = __fsub_rn(__fmul_rn(__fadd_rn(static_cast<float>(ix) + 0.5f, p.cur_dx), fs), static_cast<float>(X) + 0.5f);
    const float ey = __fsub_rn(__fmul_rn(__fadd_rn(static_cast<float>(iy) + 0.5f, p.cur_dy), fs), static_cast<float>(Y) + 0.5f);
    const float kw = __fmul_rn(fmaxf(0.f, __fsub_rn(1.f, fabsf(ex))), fmaxf(0.f, __fsub_rn(1.f, fabsf(ey))));
    const int inside = (fabsf(ex) <= 0.5f && fabsf(ey) <= 0.5f) ? 1 : 0;
    // the pixel's place in the footprint: 1 .. cols - 2 by the bound in the header comment; the min keeps a wrong bound inside the tile
    const int lx = min(ix - fx0, cols - 2), ly = min(iy - fy0, rows - 2);
    const float* centre = tile + ly * row_floats + lx * 3;
    const float c0 = centre[0], c1 = centre[1], c2 = centre[2];
    // 2 surface and own depth
    float nds[3], o[3];
    gen_ray(p.g_hi, X, Y, nds, o);
    if (p.origin_is_camera) {
      o[0] = p.g_hi.pos[0];
      o[1] = p.g_hi.pos[1];
      o[2] = p.g_hi.pos[2];
    }
    const float a = cur_acc[i], dm = cur_depth[i];
    const float t = dm / a;
    const bool near = a >= p.acc_min && fabsf(t) < INFINITY && t > 0.f;
    float P[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) P[k] = __fadd_rn(o[k], __fmul_rn(nds[k], t));
    const float zc_cur = near ? camera_depth(p.g_hi.pos, p.g_hi.rot, P) : INFINITY;
    float r0 = c0, r1 = c1, r2 = c2;      // not live: the bits copied
    int count = inside;
    int mask = 0;
    if (hist_rgb) {
      // 3 previous camera
      float q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) q[k] = near ? __fsub_rn(P[k], p.prev_pos[k]) : nds[k];      // far: direction only
      float v[3];      // camera space of the history
      to_camera(p.prev_rot, q, v);
      const float zc = -v[2];
      if (zc > 0.f && zc < INFINITY) {
        const float focal = static_cast<float>(p.g_hi.focal), fw = static_cast<float>(W), fh = static_cast<float>(H);
        const float u = image_coord(focal, v[0], zc, fw);
        const float vv = image_coord(focal, -v[1], zc, fh);
        if (u >= 0.f && u < fw && vv >= 0.f && vv < fh) {      // floorf(u) <= u < W: every tap below is inside
          const int tap = nearest_tap(u, vv, W);
          bool accepted = true;
          // 4 disocclusion: the history's depth against the range of zp over i's 3 x 3 neighbourhood
          if (hist_depth) {
            const float hd = hist_depth[tap];
            float zmin = INFINITY, zmax = -INFINITY;
            bool any_far = false, any_finite = false;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
              for (int dx = -1; dx <= 1; ++dx) {
                const float z = ztile[(ly + dy) * cols + lx + dx];
                if (z == INFINITY) {
                  any_far = true;
                } else if (z == z) {      // a NaN: no such pixel
                  any_finite = true;
                  zmin = z < zmin ? z : zmin;
                  zmax = z > zmax ? z : zmax;
                }
              }
            }
            if (hd == INFINITY) {
              accepted = any_far;
            } else if (fabsf(hd) < INFINITY) {
              accepted = any_finite && __fsub_rn(zmin, __fmul_rn(p.depth_tol, zmin)) <= hd && hd <= __fadd_rn(zmax, __fmul_rn(p.depth_tol, zmax));
            } else {
              accepted = false;
            }
          }
          if (accepted) {
            // 5 history colour
            const float fx = __fsub_rn(u, 0.5f), fy = __fsub_rn(vv, 0.5f);
            const float x0f = floorf(fx), y0f = floorf(fy);
            const float wx = __fsub_rn(fx, x0f), wy = __fsub_rn(fy, y0f);
            const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);      // -1 .. W - 1
            const int xa = max(x0, 0), xb = min(x0 + 1, W - 1), ya = max(y0, 0), yb = min(y0 + 1, H - 1);
            const float* h00 = hist_rgb + 3 * (ya * W + xa);
            const float* h01 = hist_rgb + 3 * (ya * W + xb);
            const float* h10 = hist_rgb + 3 * (yb * W + xa);
            const float* h11 = hist_rgb + 3 * (yb * W + xb);
            float hst[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const float top = __fadd_rn(h00[k], __fmul_rn(wx, __fsub_rn(h01[k], h00[k])));
              const float bot = __fadd_rn(h10[k], __fmul_rn(wx, __fsub_rn(h11[k], h10[k])));
              hst[k] = __fadd_rn(top, __fmul_rn(wy, __fsub_rn(bot, top)));
            }
            // 6 clamp
            if (p.clamp) {
              const float qnan = __int_as_float(0x7FC00000);
              float lo[3] = {qnan, qnan, qnan}, hi[3] = {qnan, qnan, qnan};
#pragma unroll
              for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                  const float* nb = tile + (ly + dy) * row_floats + (lx + dx) * 3;
#pragma unroll
                  for (int k = 0; k < 3; ++k) {
                    lo[k] = temporal_min(lo[k], nb[k]);
                    hi[k] = temporal_max(hi[k], nb[k]);
                  }
                }
              }
#pragma unroll
              for (int k = 0; k < 3; ++k) hst[k] = temporal_min(temporal_max(hst[k], lo[k]), hi[k]);
            }
            // 7 count
            bool live = true;
            float a_eff = __fmul_rn(kw, p.alpha);
            mask = 1;
            if (hist_count) {
              const int hc = hist_count[tap];
              live = hc >= 1;
              if (live) {
                count = min(hc + inside, 255);
                a_eff = __fmul_rn(kw, fmaxf(p.alpha, 1.0f / static_cast<float>(count)));
              } else {
                mask = 2;      // a placeholder replaced
              }
            } else {
              count = 1;
            }
            // 8 blend
            if (live) {
              r0 = hst[0];
              r1 = hst[1];
              r2 = hst[2];
              if (kw > 0.f) {
                r0 = blend_toward(hst[0], c0, a_eff);
                r1 = blend_toward(hst[1], c1, a_eff);
                r2 = blend_toward(hst[2], c2, a_eff);
              }
            }
          }
        }
      }
    }
    out_rgb[3 * J] = r0;
    out_rgb[3 * J + 1] = r1;
    out_rgb[3 * J + 2] = r2;
    if (out_depth) out_depth[J] = zc_cur;
    if (out_count) out_count[J] = static_cast<uint8_t>(count);
    if (out_rgba8) out_rgba8[J] = rgba8_of(r0, r1, r2);
    if (out_mask) out_mask[J] = static_cast<uint8_t>(mask);
    is_rejected = mask == 0 ? 1 : 0;
  }
  count_in_block(is_rejected, rejected);
}

}  // namespace adanerf
