// N6: temporal anti-aliasing -- a history image carried to the pose of the moment by the new frame's own depth, tested for disocclusion,
// clamped to what the new frame's 3 x 3 neighbourhood can justify and blended with the new (jittered) frame.  The stage a real-time viewer
// runs every frame between its render and its present step; the viewer has none: it shows the frame it rendered
// (adanerf_real_time_viewer/src/neuralrenderer.cpp:146-182 -> src/interoprenderbuffer.cpp:87).
// One launch, a thread per destination pixel, 32 x 8 pixel tiles:
//   temporal_resolve_kernel   destination pixel j -> its point at the current pose (ray origin + direction x depth / acc) -> the previous
//                             camera -> the history's nearest tap (depth test, count) and four bilinear taps (colour) -> min / max of the
//                             current colour over the 3 x 3 neighbourhood -> blend.  A gather: nothing depends on the order of arrival.
// The current colour's tile plus a one-pixel halo goes through LDS: rows of (32 + 2) x 3 consecutive floats, read with
// consecutive lanes on consecutive floats, so a current pixel comes from HBM about once instead of nine times; the threads then read
// at a stride of 3 floats, which is free of bank conflicts (3 is odd).  A pixel outside the image is staged as a NaN: the clamp's own
// rule skips NaNs, so the border needs no second case.  The history taps depend on the data and stay plain global loads.
// Every floating-point operation is a single rounded fp32 operation in a fixed order (the library is built with -ffp-contract=off), so
// the stage is exact against a numpy float32 restatement (tests/temporal_reference.py).  The rejected pixels are counted in integers.
// The expressions this stage shares with the others that change pose -- a point's camera depth, the rotation into a camera, image
// coordinates and tap, the history's bilinear taps, the clamp's order, the blend, the block's count -- are k_pose_core.hip.hpp's.
// Device code only (gfx950, wave64); part of stages.hip.
#pragma once
#include "k_pose_core.hip.hpp"

namespace adanerf {

constexpr int kTemporalTileW = 32, kTemporalTileH = 8;                      // 256 threads: a wave is two rows of 32 pixels
constexpr int kTemporalRowFloats = (kTemporalTileW + 2) * 3;                // a staged row: the tile and its halo, 3 channels
constexpr int kTemporalTileFloats = kTemporalRowFloats * (kTemporalTileH + 2);

struct TemporalParams {
  RayGenParams g;           // the context's ray generator with pos / rot = the CURRENT pose, pixel centres
  float prev_pos[3];
  float prev_rot[9];        // row-major c2w of the history's pose
  float alpha, depth_tol, acc_min;
  int32_t origin_is_camera; // 1: depths count from the camera position (ADANERF_SAMPLER_COARSE_FINE), 0: from the view-cell sphere exit
  int32_t clamp;            // ADANERF_TEMPORAL_CLAMP
};

__global__ __launch_bounds__(256) void temporal_resolve_kernel(TemporalParams p, const float* __restrict__ cur_rgb, const float* __restrict__ cur_depth,
                                                               const float* __restrict__ cur_acc, const float* __restrict__ hist_rgb,
                                                               const float* __restrict__ hist_depth, const uint8_t* __restrict__ hist_count,
                                                               float* __restrict__ out_rgb, float* __restrict__ out_depth,
                                                               uint8_t* __restrict__ out_count, uchar4* __restrict__ out_rgba8,
                                                               uint8_t* __restrict__ out_mask, int32_t* __restrict__ rejected) {
  __shared__ float tile[kTemporalTileFloats];
  const int w = p.g.w, h = p.g.h;      // w * h < 2^25 (frame_geometry): 3 * w * h fits an int
  const int tid = static_cast<int>(threadIdx.x);
  const int tx = tid & (kTemporalTileW - 1), ty = tid >> 5;
  const int x_first = static_cast<int>(blockIdx.x) * kTemporalTileW, y_first = static_cast<int>(blockIdx.y) * kTemporalTileH;
  const int x = x_first + tx, y = y_first + ty;
  const bool inside = x < w && y < h;
  const int j = y * w + x;

  if (p.clamp) {      // uniform over the launch
    for (int i = tid; i < kTemporalTileFloats; i += 256) {
      const int r = i / kTemporalRowFloats, c = i - r * kTemporalRowFloats;
      const int px = x_first - 1 + c / 3, py = y_first - 1 + r;
      float v = __int_as_float(0x7FC00000);      // no such pixel: skipped as a NaN is
      if (px >= 0 && px < w && py >= 0 && py < h) v = cur_rgb[(py * w + x_first - 1) * 3 + c];
      tile[i] = v;
    }
    __syncthreads();
  }

  int is_rejected = 0;
  if (inside) {
    float nds[3], o[3];
    gen_ray(p.g, x, y, nds, o);
    if (p.origin_is_camera) {
      o[0] = p.g.pos[0];
      o[1] = p.g.pos[1];
      o[2] = p.g.pos[2];
    }
    const float a = cur_acc[j], dm = cur_depth[j];
    const float t = dm / a;
    const bool near = a >= p.acc_min && fabsf(t) < INFINITY && t > 0.f;      // a NaN fails every comparison: far
    float P[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) P[k] = __fadd_rn(o[k], __fmul_rn(nds[k], t));
    const float zc_cur = near ? camera_depth(p.g.pos, p.g.rot, P) : INFINITY;
    const float c0 = cur_rgb[3 * j], c1 = cur_rgb[3 * j + 1], c2 = cur_rgb[3 * j + 2];
    float r0 = c0, r1 = c1, r2 = c2;      // a rejected pixel: the bits copied
    int count = 1;
    bool accepted = false;
    if (hist_rgb) {
      float q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) q[k] = near ? __fsub_rn(P[k], p.prev_pos[k]) : nds[k];      // far: direction only
      float v[3];      // camera space of the history
      to_camera(p.prev_rot, q, v);
      const float zc = -v[2];
      if (zc > 0.f && zc < INFINITY) {
        const float focal = static_cast<float>(p.g.focal), fw = static_cast<float>(w), fh = static_cast<float>(h);
        const float u = image_coord(focal, v[0], zc, fw);
        const float vv = image_coord(focal, -v[1], zc, fh);
        if (u >= 0.f && u < fw && vv >= 0.f && vv < fh) {      // floorf(u) <= u < w: every tap below is inside
          const int tap = nearest_tap(u, vv, w);
          accepted = true;
          if (hist_depth) {
            const float hd = hist_depth[tap];
            accepted = near ? (fabsf(hd) < INFINITY && fabsf(__fsub_rn(zc, hd)) <= __fmul_rn(p.depth_tol, zc)) : hd == INFINITY;
          }
          if (accepted) {
            float hst[3];
            bilinear_history(hist_rgb, w, h, u, vv, hst);
            if (p.clamp) {
              const float qnan = __int_as_float(0x7FC00000);
              float lo[3] = {qnan, qnan, qnan}, hi[3] = {qnan, qnan, qnan};
#pragma unroll
              for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                  const float* s = tile + (ty + 1 + dy) * kTemporalRowFloats + (tx + 1 + dx) * 3;
#pragma unroll
                  for (int k = 0; k < 3; ++k) {
                    lo[k] = temporal_min(lo[k], s[k]);
                    hi[k] = temporal_max(hi[k], s[k]);
                  }
                }
              }
#pragma unroll
              for (int k = 0; k < 3; ++k) hst[k] = temporal_min(temporal_max(hst[k], lo[k]), hi[k]);
            }
            float a_eff = p.alpha;
            if (hist_count) {
              count = min(static_cast<int>(hist_count[tap]) + 1, 255);
              a_eff = fmaxf(p.alpha, 1.0f / static_cast<float>(count));
            }
            r0 = blend_toward(hst[0], c0, a_eff);
            r1 = blend_toward(hst[1], c1, a_eff);
            r2 = blend_toward(hst[2], c2, a_eff);
          }
        }
      }
    }
    out_rgb[3 * j] = r0;
    out_rgb[3 * j + 1] = r1;
    out_rgb[3 * j + 2] = r2;
    if (out_depth) out_depth[j] = zc_cur;
    if (out_count) out_count[j] = static_cast<uint8_t>(count);
    if (out_rgba8) out_rgba8[j] = rgba8_of(r0, r1, r2);
    if (out_mask) out_mask[j] = accepted ? 1 : 0;
    is_rejected = accepted ? 0 : 1;
  }
  count_in_block(is_rejected, rejected);
}

}  // namespace adanerf
