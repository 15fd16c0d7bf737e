// N14: two-source reprojection (bidirectional frame interpolation) -- two rendered fp32 frames A and B, each with its depth_map, acc_map
// and pose, warped to a pose between them.  A disocclusion is a region ONE frame never saw; a frame behind and a frame ahead uncover
// each other's, so a pixel is a hole only where neither source has data.  For a host that knows the next rendered frame: one that
// replays a script, evaluates a pose list, or shows its frames K calls late.
// Three launches, a thread per pixel each, no LDS staging:
//   reproject_clear_kernel         (k_reproject.hip.hpp) over BOTH z-buffers, Z_A at [0, n) and Z_B at [n, 2n), and the hole count
//   reproject_pair_splat_kernel    grid.y = 2: row s of the grid splats source s into Z_s with reproject_splat_pixel, the body of
//                                  adanerf_reproject's splat, so each Z_s is bit for bit what adanerf_reproject builds for that source;
//                                  the two scatters run side by side instead of one behind the other
//   reproject_pair_resolve_kernel  destination pixel j, k_s = Z_s[j], z_s the float in the high word (+inf: a far winner), i_s the low word:
//                                  both winners   agree iff both far, or both near and |zA - zB| <= depth_tol * min(zA, zB)
//                                                 agree: c = cA + weight_b * (cB - cA) per channel, depth the same expression on zA, zB
//                                                 (+inf when both are far), mask 1, source 3.  Otherwise the smaller high word wins (the
//                                                 nearer surface occludes the other; a near winner beats a far one): its colour and depth,
//                                                 mask 1, source 1 (A) or 2 (B)
//                                  one winner     its colour and depth, mask 1, source 1 or 2
//                                  none, fill     the LARGEST key among the 8 neighbours' winners in both z-buffers (never a filled result:
//                                                 no dependence on order); B's is taken iff it is larger than A's, so A wins on equal
//                                                 keys; mask 2, source 1 or 2
//                                  otherwise      fp32 (0, 0, 0), hole_rgba8, depth 0, mask 0, source 0; counted in integers
// Every floating-point operation is a single rounded fp32 operation in a fixed order (the library is built with -ffp-contract=off; the
// blend is blend_toward: a subtraction, a multiplication, an addition), no floating-point atomics, so the stage is exact against a numpy
// float32 restatement (tests/reproject_pair_reference.py).  The resolve's reads of the z-buffers are coalesced, its colour reads follow
// the winners (neighbouring destination pixels mostly have neighbouring winners).
// Device code only (gfx950, wave64); part of stages.hip.
#pragma once
#include "k_reproject.hip.hpp"

namespace adanerf {

struct PairSplatParams {
  ReprojectParams s[2];      // source A, source B: g with that source's pose, the same destination
  const float* depth[2];
  const float* acc[2];
};

struct PairResolveParams {
  const float* rgb[2];       // fp32 colour [n,3] of A and of B
  int32_t w, h, fill;
  float weight_b, depth_tol;
  uint32_t hole_rgba8;
};

// zbuf: Z_A at [0, n), Z_B at [n, 2n)
__global__ __launch_bounds__(256) void reproject_pair_splat_kernel(PairSplatParams P, unsigned long long* __restrict__ zbuf) {
  const int s = static_cast<int>(blockIdx.y);      // uniform over the block
  const ReprojectParams& p = P.s[s];
  const int n = p.g.w * p.g.h;                     // < 2^25 (frame_geometry)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  reproject_splat_pixel(p, i, P.depth[s], P.acc[s], zbuf + static_cast<size_t>(s) * n);
}

// the largest key among the 8 neighbours of (x, y) in one z-buffer, 0 for none (no key is 0: zc > 0 has bits > 0)
__device__ __forceinline__ unsigned long long reproject_farthest_neighbour(const unsigned long long* __restrict__ zbuf, int x, int y, int w, int h) {
  unsigned long long best = 0;
  for (int dy = -1; dy <= 1; ++dy) {
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = x + dx, yy = y + dy;
      if ((dx | dy) == 0 || xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
      const unsigned long long k = zbuf[yy * w + xx];
      if (k != kReprojectEmpty && k > best) best = k;
    }
  }
  return best;
}

__global__ __launch_bounds__(256) void reproject_pair_resolve_kernel(PairResolveParams p, const unsigned long long* __restrict__ zbuf,
                                                                     float* __restrict__ dst_rgb, uchar4* __restrict__ dst_rgba8,
                                                                     float* __restrict__ dst_depth, uint8_t* __restrict__ dst_mask,
                                                                     uint8_t* __restrict__ dst_source, int32_t* __restrict__ holes) {
  const int w = p.w, h = p.h, n = w * h;      // 3 * n fits an int
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool inside = j < n;
  int is_hole = 0;
  if (inside) {
    const unsigned long long* zA = zbuf;
    const unsigned long long* zB = zbuf + n;
    unsigned long long kA = zA[j], kB = zB[j];
    const bool hasA = kA != kReprojectEmpty, hasB = kB != kReprojectEmpty;
    int mask = 1, source = 0;
    if (!hasA && !hasB) {
      mask = 0;
      if (p.fill) {
        const int y = j / w, x = j - y * w;
        kA = reproject_farthest_neighbour(zA, x, y, w, h);
        kB = reproject_farthest_neighbour(zB, x, y, w, h);
        if ((kA | kB) != 0) {
          mask = 2;
          source = kB > kA ? 2 : 1;      // on equal keys A
        }
      }
    } else if (hasA && hasB) {
      const uint32_t bA = static_cast<uint32_t>(kA >> 32), bB = static_cast<uint32_t>(kB >> 32);
      const bool farA = bA == kReprojectFarBits, farB = bB == kReprojectFarBits;
      const float zA_ = __uint_as_float(bA), zB_ = __uint_as_float(bB);
      const bool agree = (farA && farB) || (!farA && !farB && fabsf(__fsub_rn(zA_, zB_)) <= __fmul_rn(p.depth_tol, fminf(zA_, zB_)));
      source = agree ? 3 : (bB < bA ? 2 : 1);
    } else {
      source = hasA ? 1 : 2;
    }
    float c[3] = {0.f, 0.f, 0.f}, z = 0.f;
    if (source == 3) {
      const float* ca = p.rgb[0] + 3 * static_cast<int>(static_cast<uint32_t>(kA));
      const float* cb = p.rgb[1] + 3 * static_cast<int>(static_cast<uint32_t>(kB));
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = blend_toward(ca[k], cb[k], p.weight_b);
      const uint32_t bA = static_cast<uint32_t>(kA >> 32);
      z = bA == kReprojectFarBits ? INFINITY : blend_toward(__uint_as_float(bA), __uint_as_float(static_cast<uint32_t>(kB >> 32)), p.weight_b);
    } else if (source != 0) {
      const unsigned long long key = source == 1 ? kA : kB;
      const float* cs = p.rgb[source - 1] + 3 * static_cast<int>(static_cast<uint32_t>(key));
      c[0] = cs[0];
      c[1] = cs[1];
      c[2] = cs[2];
      z = __uint_as_float(static_cast<uint32_t>(key >> 32));
    }
    dst_rgb[3 * j] = c[0];
    dst_rgb[3 * j + 1] = c[1];
    dst_rgb[3 * j + 2] = c[2];
    if (dst_rgba8) {
      uchar4 px = rgba8_of(c[0], c[1], c[2]);
      if (!mask) px = make_uchar4(p.hole_rgba8 & 0xFF, (p.hole_rgba8 >> 8) & 0xFF, (p.hole_rgba8 >> 16) & 0xFF, p.hole_rgba8 >> 24);
      dst_rgba8[j] = px;
    }
    if (dst_depth) dst_depth[j] = z;
    if (dst_mask) dst_mask[j] = static_cast<uint8_t>(mask);
    if (dst_source) dst_source[j] = static_cast<uint8_t>(source);
    is_hole = mask == 0;
  }
  count_in_block(is_hole, holes);
}

}  // namespace adanerf
