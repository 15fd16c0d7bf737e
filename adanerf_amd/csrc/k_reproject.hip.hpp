// N4: depth reprojection (timewarp) -- a rendered frame, its depth_map and acc_map (adanerf_set_aux_outputs) and the pose it was rendered
// at, warped to another pose.  The stage a head-tracked or 120 Hz host puts in front of its present step (the viewer has none: it shows
// the frame it rendered, adanerf_real_time_viewer/src/neuralrenderer.cpp:146-182 -> src/interoprenderbuffer.cpp:87).
// Three launches, a thread per pixel each, no LDS staging:
//   reproject_clear_kernel    z-buffer to all ones, hole count to 0
//   reproject_splat_kernel    source pixel i -> its point (ray origin + direction x depth / acc) -> the destination camera -> one 64-bit
//                             atomicMin of (float bits of the camera depth << 32 | i) on the pixel it lands in.  Positive floats order as
//                             their bits and the source index breaks ties, so the winner does not depend on the order of arrival.
//   reproject_resolve_kernel  destination pixel j: the winner's colour / depth; a hole takes the FARTHEST of its 8 neighbours' splat keys
//                             (never a filled result: no dependence on order); holes left over are counted in integers.
// Every floating-point operation is a single rounded fp32 operation in a fixed order (the library is built with -ffp-contract=off), so
// the stage is exact against a numpy float32 restatement (tests/reproject_reference.py).  The source reads are coalesced, the scatter is
// what it is: one 8-byte atomic per source pixel, 5.1 MB of them for an 800 x 800 frame.
// The rotation into the destination camera, the image coordinates and the block's count are k_pose_core.hip.hpp's.  The splat of one source
// pixel is reproject_splat_pixel, which adanerf_reproject_pair's splat (k_reproject_pair.hip.hpp) calls per source as well.
// Device code only (gfx950, wave64); part of stages.hip.
#pragma once
#include "k_pose_core.hip.hpp"

namespace adanerf {

constexpr unsigned long long kReprojectEmpty = ~0ull;
constexpr uint32_t kReprojectFarBits = 0x7F800000u;      // +inf: a pixel without a surface lies behind every pixel with one

struct ReprojectParams {
  RayGenParams g;           // the context's ray generator with pos / rot = the SOURCE pose
  float dst_pos[3];
  float dst_rot[9];         // row-major c2w of the destination
  float acc_min;
  int32_t origin_is_camera; // 1: depths count from the camera position (ADANERF_SAMPLER_COARSE_FINE), 0: from the view-cell sphere exit
};

__global__ __launch_bounds__(256) void reproject_clear_kernel(unsigned long long* __restrict__ zbuf, int n, int32_t* __restrict__ holes) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) *holes = 0;
  if (j < n) zbuf[j] = kReprojectEmpty;
}

// the splat of source pixel i (the caller's i < w * h) into zbuf: adanerf_reproject's, and per source adanerf_reproject_pair's
__device__ __forceinline__ void reproject_splat_pixel(const ReprojectParams& p, int i, const float* __restrict__ depth, const float* __restrict__ acc,
                                                      unsigned long long* __restrict__ zbuf) {
  const int w = p.g.w, h = p.g.h;
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
  float q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = near ? __fsub_rn(__fadd_rn(o[k], __fmul_rn(nds[k], t)), p.dst_pos[k]) : nds[k];      // far: direction only
  float v[3];      // camera space of the destination
  to_camera(p.dst_rot, q, v);
  const float zc = -v[2];
  if (!(zc > 0.f && zc < INFINITY)) return;
  const float focal = static_cast<float>(p.g.focal), fw = static_cast<float>(w), fh = static_cast<float>(h);
  const float u = image_coord(focal, v[0], zc, fw);
  const float vv = image_coord(focal, -v[1], zc, fh);
  if (!(u >= 0.f && u < fw && vv >= 0.f && vv < fh)) return;      // floorf(u) <= u < w: the pixel is inside
  const int X = static_cast<int>(floorf(u)), Y = static_cast<int>(floorf(vv));
  const unsigned long long key =
      (static_cast<unsigned long long>(near ? __float_as_uint(zc) : kReprojectFarBits) << 32) | static_cast<unsigned long long>(static_cast<uint32_t>(i));
  atomicMin(zbuf + (Y * w + X), key);
}

__global__ __launch_bounds__(256) void reproject_splat_kernel(ReprojectParams p, const float* __restrict__ depth, const float* __restrict__ acc,
                                                              unsigned long long* __restrict__ zbuf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;      // w * h < 2^25 (frame_geometry)
  if (i >= p.g.w * p.g.h) return;
  reproject_splat_pixel(p, i, depth, acc, zbuf);
}

// fill != 0: a hole takes the largest key among its 8 neighbours' splats.  holes: += the pixels left with mask 0, one atomicAdd per block.
__global__ __launch_bounds__(256) void reproject_resolve_kernel(const unsigned long long* __restrict__ zbuf, const uint32_t* __restrict__ src, int w,
                                                                int h, int fill, uint32_t hole_rgba8, uint32_t* __restrict__ dst,
                                                                float* __restrict__ dst_depth, uint8_t* __restrict__ dst_mask,
                                                                int32_t* __restrict__ holes) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool inside = j < w * h;
  int is_hole = 0;
  if (inside) {
    unsigned long long key = zbuf[j];
    int mask = 1;
    if (key == kReprojectEmpty) {
      mask = 0;
      if (fill) {
        const int y = j / w, x = j - y * w;
        unsigned long long best = 0;      // no key is 0: zc > 0 has bits > 0
        for (int dy = -1; dy <= 1; ++dy) {
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx, yy = y + dy;
            if ((dx | dy) == 0 || xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
            const unsigned long long k = zbuf[yy * w + xx];
            if (k != kReprojectEmpty && k > best) best = k;
          }
        }
        if (best != 0) {
          key = best;
          mask = 2;
        }
      }
    }
    dst[j] = mask ? src[static_cast<uint32_t>(key)] : hole_rgba8;
    if (dst_depth) dst_depth[j] = mask ? __uint_as_float(static_cast<uint32_t>(key >> 32)) : 0.f;
    if (dst_mask) dst_mask[j] = static_cast<uint8_t>(mask);
    is_hole = mask == 0;
  }
  count_in_block(is_hole, holes);
}

}  // namespace adanerf
