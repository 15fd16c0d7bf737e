// N13: gather reprojection -- adanerf_reproject's job done from the destination's side: a rendered fp32 frame, its depth_map and acc_map
// and the pose it was rendered at, warped to another pose with only the SOURCE frame's depth.  Each destination pixel searches its own
// ray for the source surface by a fixed-point iteration (guess a depth on the ray, look where that point lies in the source frame, take
// the surface found there as the next guess), so a pixel is a hole only where the source frame has nothing, never because no splat
// happened to land on it.
// Two launches, no LDS staging:
//   gather_surface_kernel   a thread per source pixel, coalesced: its surface point S and its depth zs in the source camera as one
//                           float4 (S.xyz, zs) in context-owned scratch, zs = +inf for a pixel without a surface.  This takes the
//                           float64 gen_ray of a source pixel out of the iteration and makes every data-dependent tap of the iteration
//                           one aligned 16-byte load.
//   gather_warp_kernel      a thread per destination pixel, 32 x 8 pixel tiles: the destination ray, `iterations` dependent taps of
//                           the surface table (the same count in every lane: a lane that has died keeps its last tap and goes on
//                           loading it, so the wave stays converged), one more for the consistency test, four bilinear taps of the
//                           colour.  All of them plain global loads: they depend on the data, and the re-reads hit L2.
// Every floating-point operation is a single rounded fp32 operation in a fixed order (the library is built with -ffp-contract=off), so
// the stage is exact against a numpy float32 restatement (tests/reproject_gather_reference.py); a gather, so nothing depends on the
// order of arrival.  The holes are counted in integers.  The camera depth, the rotation into the source camera, the image coordinates,
// the nearest tap, the bilinear colour taps and the block's count are k_pose_core.hip.hpp's.
// Device code only (gfx950, wave64); part of stages.hip.
#pragma once
#include "k_pose_core.hip.hpp"

namespace adanerf {

constexpr int kGatherTileW = 32, kGatherTileH = 8;      // 256 threads: a wave is two rows of 32 pixels
constexpr int kGatherMaxIterations = 8;

struct GatherSurfaceParams {
  RayGenParams g;           // the context's ray generator with pos / rot = the SOURCE pose, pixel centres
  float acc_min;
  int32_t origin_is_camera; // 1: depths count from the camera position (ADANERF_SAMPLER_COARSE_FINE), 0: from the view-cell sphere exit
};

struct GatherWarpParams {
  RayGenParams g;           // the same generator with pos / rot = the DESTINATION pose, pixel centres
  float src_pos[3];
  float src_rot[9];         // row-major c2w of the source
  float depth_tol;
  int32_t iterations;       // 1 .. kGatherMaxIterations
  int32_t guess;            // ADANERF_GATHER_GUESS
  uint32_t hole_rgba8;
};

__global__ __launch_bounds__(256) void gather_surface_kernel(GatherSurfaceParams p, const float* __restrict__ depth, const float* __restrict__ acc,
                                                             float4* __restrict__ surface) {
  const int w = p.g.w, h = p.g.h;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;      // w * h < 2^25 (frame_geometry)
  if (i >= w * h) return;
  const int row = i / w, col = i - row * w;
  float nds[3], o[3];
  gen_ray(p.g, col, row, nds, o);
  if (p.origin_is_camera) {
    o[0] = p.g.pos[0];
    o[1] = p.g.pos[1];
    o[2] = p.g.pos[2];
  }
  const float a = acc[i], dm = depth[i];
  const float t = dm / a;
  const bool near = a >= p.acc_min && fabsf(t) < INFINITY && t > 0.f;      // a NaN fails every comparison: far
  float S[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) S[k] = __fadd_rn(o[k], __fmul_rn(nds[k], t));
  const float zs = near ? camera_depth(p.g.pos, p.g.rot, S) : INFINITY;
  surface[i] = make_float4(S[0], S[1], S[2], zs);
}

__global__ __launch_bounds__(256) void gather_warp_kernel(GatherWarpParams p, const float4* __restrict__ surface, const float* __restrict__ src_rgb,
                                                          float* __restrict__ dst_rgb, uchar4* __restrict__ dst_rgba8, float* __restrict__ dst_depth,
                                                          uint8_t* __restrict__ dst_mask, int32_t* __restrict__ holes) {
  const int w = p.g.w, h = p.g.h;      // w * h < 2^25 (frame_geometry): 3 * w * h fits an int
  const int tid = static_cast<int>(threadIdx.x);
  const int x = static_cast<int>(blockIdx.x) * kGatherTileW + (tid & (kGatherTileW - 1));
  const int y = static_cast<int>(blockIdx.y) * kGatherTileH + (tid >> 5);
  const bool inside = x < w && y < h;
  const int j = y * w + x;

  int is_hole = 0;
  if (inside) {
    float d[3], exit_point[3];
    gen_ray(p.g, x, y, d, exit_point);      // only the direction is used
    const float focal = static_cast<float>(p.g.focal), fw = static_cast<float>(w), fh = static_cast<float>(h);
    int tap = j;
    bool alive = true, est_near = false;
    float u = 0.5f, vv = 0.5f, zc = 0.f;      // of the last step the pixel lived through; (0.5, 0.5) keeps a dead pixel's colour taps inside
    float P[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < p.iterations; ++k) {      // uniform over the launch
      const float4 s4 = surface[tap];
      const bool near = s4.w != INFINITY;
      const float s = __fadd_rn(__fadd_rn(__fmul_rn(__fsub_rn(s4.x, p.g.pos[0]), d[0]), __fmul_rn(__fsub_rn(s4.y, p.g.pos[1]), d[1])),
                                __fmul_rn(__fsub_rn(s4.z, p.g.pos[2]), d[2]));
      bool ok = !near || (fabsf(s) < INFINITY && s > 0.f);
      float Pk[3], q[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Pk[c] = __fadd_rn(p.g.pos[c], __fmul_rn(d[c], s));
        q[c] = near ? __fsub_rn(Pk[c], p.src_pos[c]) : d[c];      // far: direction only
      }
      float v[3];      // camera space of the source
      to_camera(p.src_rot, q, v);
      const float z = -v[2];
      const float uk = image_coord(focal, v[0], z, fw);
      const float vk = image_coord(focal, -v[1], z, fh);
      ok = ok && z > 0.f && z < INFINITY && uk >= 0.f && uk < fw && vk >= 0.f && vk < fh;      // floorf(uk) <= uk < w: the tap is inside
      alive = alive && ok;
      if (alive) {      // a dead pixel keeps what it had
        tap = nearest_tap(uk, vk, w);
        u = uk;
        vv = vk;
        zc = z;
        P[0] = Pk[0];
        P[1] = Pk[1];
        P[2] = Pk[2];
        est_near = near;
      }
    }
    const float zt = surface[tap].w;
    const bool tap_near = zt != INFINITY;
    const bool consistent = est_near ? (tap_near && fabsf(__fsub_rn(zc, zt)) <= __fmul_rn(p.depth_tol, zc)) : !tap_near;
    float col[3];
    bilinear_history(src_rgb, w, h, u, vv, col);
    const float zd = est_near ? camera_depth(p.g.pos, p.g.rot, P) : INFINITY;
    const int mask = alive ? (consistent ? 1 : (p.guess ? 2 : 0)) : 0;
    const float r0 = mask ? col[0] : 0.f, r1 = mask ? col[1] : 0.f, r2 = mask ? col[2] : 0.f;
    dst_rgb[3 * j] = r0;
    dst_rgb[3 * j + 1] = r1;
    dst_rgb[3 * j + 2] = r2;
    if (dst_rgba8) {
      uchar4 px = rgba8_of(r0, r1, r2);
      if (!mask) px = make_uchar4(p.hole_rgba8 & 0xFF, (p.hole_rgba8 >> 8) & 0xFF, (p.hole_rgba8 >> 16) & 0xFF, p.hole_rgba8 >> 24);
      dst_rgba8[j] = px;
    }
    if (dst_depth) dst_depth[j] = mask ? zd : 0.f;
    if (dst_mask) dst_mask[j] = static_cast<uint8_t>(mask);
    is_hole = mask == 0;
  }
  count_in_block(is_hole, holes);
}

}  // namespace adanerf
