// N12: the temporal resolve of a foveated frame (adanerf_temporal_resolve_sparse) -- the temporal resolve (k_temporal.hip.hpp) told which
// pixels of the frame were rendered (mask byte 0) and which adanerf_fill_density_phased only reconstructed (byte 2, 4 or 8, the stride).
// A rendered pixel refreshes the history as there; a reconstructed pixel keeps the history it has and shows the fill only where it has
// none, so a lattice that moves through its 64 phases converges on the full render while the camera rests.
// Two launches:
//   upsample_depth_kernel   (pass A, k_upsample.hip.hpp's, with the context's generator at pixel centres as its g_lo) pixel i -> zp[i],
//                           its surface's camera depth at the PREVIOUS pose (+inf: far).  Only when the history's depth is tested.
//   sparse_resolve_kernel   (pass B) pixel j -> its surface -> the previous camera -> the history's nearest tap (depth against the range of
//                           zp over the 3 x 3 neighbourhood of a rendered pixel, over the used corners of a reconstructed one; count)
//                           and four bilinear taps -> a rendered pixel: clamp to the current colour's 3 x 3 neighbourhood, blend;
//                           a reconstructed pixel: the history unclamped.  A gather: nothing depends on the order of arrival.
// Pass B works on 32 x 8 tiles, a thread per pixel, consecutive lanes along a row.  The 3 x 3 neighbourhoods of the current colour and
// of zp are nine plain global loads each, bounds-checked (a pixel outside the image is skipped, which is what the clamp's rule does with
// a NaN): the tile-plus-halo staging through LDS that temporal_resolve_kernel and upsample_resolve_kernel use was built and measured
// here, and lost -- 31.8 us against 29.8 us at 800 x 800 and 64.7 us against 60.0 us at 1920 x 1080 for pass B without the depth test,
// alternated twice in one session (profiles/foveated_temporal_measured.md): the neighbours of a row-major tile are the same cache
// lines the next row of lanes reads anyway, and the staging adds a barrier.  The corners' zp and the history taps are plain global loads
// too: the lanes of one cell share the corner addresses, so a wave in the stride-8 region asks for at most 9 + 9 distinct ones.
// The rejected pixels are counted in integers: a __ballot per wave, the four counts summed through LDS, one atomicAdd per block that
// has any, as the two sibling kernels count.  One atomicAdd per wave was measured first: with a third of the pixels rejected its 10 000
// (32 400) adds on one address made the call 0.133 ms (0.362 ms) where this form takes 0.059 ms (0.125 ms).
// Every floating-point operation is a single rounded fp32 operation in a fixed order (-ffp-contract=off and the _rn intrinsics), so the
// stage is exact against a numpy float32 restatement (tests/sparse_temporal_reference.py).
// The expressions shared with the other stages that change pose are k_pose_core.hip.hpp's.
// Device code only (gfx950, wave64); part of stages.hip.
#pragma once
#include "k_upsample.hip.hpp"

namespace adanerf {

// zmin / zmax / any_far of step 4 over one more value of zp; a NaN is "no such pixel"
__device__ __forceinline__ void sparse_z_take(float z, float& zmin, float& zmax, bool& any_far, bool& any_finite) {
  if (z == INFINITY) {
    any_far = true;
  } else if (z == z) {
    any_finite = true;
    zmin = z < zmin ? z : zmin;
    zmax = z > zmax ? z : zmax;
  }
}

__global__ __launch_bounds__(256) void sparse_resolve_kernel(TemporalParams p, int phase_x, int phase_y, const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ cur_rgb, const float* __restrict__ cur_depth,
                                                             const float* __restrict__ cur_acc, const float* __restrict__ zp,
                                                             const float* __restrict__ hist_rgb, const float* __restrict__ hist_depth,
                                                             const uint8_t* __restrict__ hist_count, float* __restrict__ out_rgb,
                                                             float* __restrict__ out_depth, uint8_t* __restrict__ out_count,
                                                             uchar4* __restrict__ out_rgba8, uint8_t* __restrict__ out_mask,
                                                             int32_t* __restrict__ rejected) {
  const int w = p.g.w, h = p.g.h;      // w * h < 2^25 (frame_geometry): 3 * w * h fits an int
  const int tid = static_cast<int>(threadIdx.x);
  const int tx = tid & (kTemporalTileW - 1), ty = tid >> 5;
  const int x_first = static_cast<int>(blockIdx.x) * kTemporalTileW, y_first = static_cast<int>(blockIdx.y) * kTemporalTileH;
  const int x = x_first + tx, y = y_first + ty;
  const bool inside = x < w && y < h;
  const int j = y * w + x;
  bool is_rejected = false;
  if (inside) {
    const int s = mask[j];
    const bool rendered = s == 0, rebuilt = s == 2 || s == 4 || s == 8;
    // 1, 2 surface and own depth
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
    float r0 = c0, r1 = c1, r2 = c2;      // not live: the bits copied
    int count = rendered ? 1 : 0;
    int verdict = 0;
    if (hist_rgb && (rendered || rebuilt)) {
      // 3 previous camera
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
          bool accepted = true;
          // 4 disocclusion: the history's depth against the range of zp over the 3 x 3 neighbourhood or the cell's used corners
          if (hist_depth) {
            const float hd = hist_depth[tap];
            float zmin = INFINITY, zmax = -INFINITY;
            bool any_far = false, any_finite = false;
            if (rendered) {
#pragma unroll
              for (int dy = 0; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx <= 2; ++dx) {
                  const int qx = x - 1 + dx, qy = y - 1 + dy;
                  if (qx >= 0 && qx < w && qy >= 0 && qy < h) sparse_z_take(zp[qy * w + qx], zmin, zmax, any_far, any_finite);
                }
              }
            } else {
              const DensityAxis ax = density_cell_axis(x, phase_x, s, w), ay = density_cell_axis(y, phase_y, s, h);
              if (!ax.none && !ay.none) {      // the corners that are not distinct repeat one that is
                sparse_z_take(zp[ay.c0 * w + ax.c0], zmin, zmax, any_far, any_finite);
                sparse_z_take(zp[ay.c0 * w + ax.c1], zmin, zmax, any_far, any_finite);
                sparse_z_take(zp[ay.c1 * w + ax.c0], zmin, zmax, any_far, any_finite);
                sparse_z_take(zp[ay.c1 * w + ax.c1], zmin, zmax, any_far, any_finite);
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
            // 7 count
            const int hc = hist_count[tap];
            const bool live = hc >= 1;
            verdict = live ? 1 : 2;
            if (live) {
              // 5 history colour
              float hst[3];
              bilinear_history(hist_rgb, w, h, u, vv, hst);
              if (rendered) {
                // 6 clamp: a reconstructed pixel's own colour is an interpolation and no evidence against its history
                if (p.clamp) {
                  const float qnan = __int_as_float(0x7FC00000);
                  float lo[3] = {qnan, qnan, qnan}, hi[3] = {qnan, qnan, qnan};
#pragma unroll
                  for (int dy = 0; dy <= 2; ++dy) {
#pragma unroll
                    for (int dx = 0; dx <= 2; ++dx) {
                      const int qx = x - 1 + dx, qy = y - 1 + dy;
                      if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;      // no such pixel
                      const float* nb = cur_rgb + 3 * (qy * w + qx);
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
                // 8 blend
                count = min(hc + 1, 255);
                const float a_eff = fmaxf(p.alpha, 1.0f / static_cast<float>(count));
                r0 = blend_toward(hst[0], c0, a_eff);
                r1 = blend_toward(hst[1], c1, a_eff);
                r2 = blend_toward(hst[2], c2, a_eff);
              } else {
                count = hc;
                r0 = hst[0];
                r1 = hst[1];
                r2 = hst[2];
              }
            }
          }
        }
      }
    }
    out_rgb[3 * j] = r0;
    out_rgb[3 * j + 1] = r1;
    out_rgb[3 * j + 2] = r2;
    if (out_depth) out_depth[j] = zc_cur;
    out_count[j] = static_cast<uint8_t>(count);
    if (out_rgba8) out_rgba8[j] = rgba8_of(r0, r1, r2);
    if (out_mask) out_mask[j] = static_cast<uint8_t>(verdict);
    is_rejected = verdict == 0;
  }
  __shared__ int wave_rejected[4];
  const uint64_t lost = __ballot(is_rejected);
  if (lane_id() == 0) wave_rejected[tid >> 6] = __popcll(lost);
  __syncthreads();
  if (tid == 0) {      // one atomic per block that has any
    const int in_block = (wave_rejected[0] + wave_rejected[1]) + (wave_rejected[2] + wave_rejected[3]);
    if (in_block) atomicAdd(rejected, in_block);
  }
}

}  // namespace adanerf
