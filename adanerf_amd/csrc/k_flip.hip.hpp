// N1: FLIP (Andersson et al., HPG 2020) between two images as the reference's image evaluation computes it
// (src/evaluate.py:120-145 over src/util/flip_loss.py:61-105).  Device code only (gfx950, wave64); part of kernels.hip.hpp.
//
// One fused kernel per 32 x 32 output tile: the tile plus halo of both images goes to LDS in YCxCz (coordinates clamped on load --
// the reference's replicate pad; a pointwise transform commutes with it), the colour pipeline (three contrast-sensitivity filters,
// L*a*b*, Hunt, HyAB, redistribution) and the feature pipeline (edge / point detectors on the luminance, in x and transposed) are
// evaluated from LDS as direct 2-D convolutions, the error map is written, and the workgroup leaves one partial sum (fp64, LDS tree
// in a fixed order).  flip_mean_kernel adds the partial sums in a fixed order: no floating-point atomics, so the mean is reproducible
// bit for bit.  Filter tables and radii arrive at run time (they depend on pixels per degree); the host builds them in fp64 as the
// reference does (flip_tables.cpp).  Every clamp and maximum keeps a NaN, as torch.clamp / torch.max do (fminf / fmaxf
// would drop it); lane exchanges: none.
#pragma once
#include "k_common.hip.hpp"

namespace adanerf {

constexpr int kFlipTile = 32;          // output tile edge; 256 threads, thread (tx, ty) owns pixels (tx, ty + 8 k), k = 0..3
constexpr int kFlipThreads = 256;

__device__ __forceinline__ float flip_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }      // NaN stays NaN

__device__ __forceinline__ float flip_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

__device__ __forceinline__ float flip_srgb_to_linear(float c) {
  c = flip_clamp01(c);
  return c > 0.04045f ? powf((c + 0.055f) / 1.055f, 2.4f) : c / 12.92f;
}

__device__ __forceinline__ void flip_mat3(const float* m, float a, float b, float c, float& x, float& y, float& z) {
  x = m[0] * a + m[1] * b + m[2] * c;
  y = m[3] * a + m[4] * b + m[5] * c;
  z = m[6] * a + m[7] * b + m[8] * c;
}

// color_space_transform(., 'srgb2ycxcz')
__device__ __forceinline__ void flip_srgb_to_ycxcz(const FlipParams& p, float r, float g, float b, float& y, float& cx, float& cz) {
  float X, Y, Z;
  flip_mat3(p.rgb2xyz, flip_srgb_to_linear(r), flip_srgb_to_linear(g), flip_srgb_to_linear(b), X, Y, Z);
  X = X / p.illum[0];
  Y = Y / p.illum[1];
  Z = Z / p.illum[2];
  y = 116.0f * Y - 16.0f;
  cx = 500.0f * (X - Y);
  cz = 200.0f * (Y - Z);
}

__device__ __forceinline__ float flip_lab_f(const FlipParams& p, float t) {
  return t > 0.00885f ? powf(t, 1.0f / 3.0f) : t / p.lab_div + p.lab_add;
}

// filtered YCxCz -> clamped linear RGB (spatial_filter's tail) -> L*a*b* -> hunt_adjustment
__device__ __forceinline__ void flip_ycxcz_to_hunt_lab(const FlipParams& p, float y, float cx, float cz, float& L, float& a, float& b) {
  const float fy = (y + 16.0f) / 116.0f;
  const float fx = fy + cx / 500.0f;
  const float fz = fy - cz / 200.0f;
  float r, g, bl;
  flip_mat3(p.xyz2rgb, fx * p.illum[0], fy * p.illum[1], fz * p.illum[2], r, g, bl);
  float X, Y, Z;
  flip_mat3(p.rgb2xyz, flip_clamp01(r), flip_clamp01(g), flip_clamp01(bl), X, Y, Z);
  X = flip_lab_f(p, X / p.illum[0]);
  Y = flip_lab_f(p, Y / p.illum[1]);
  Z = flip_lab_f(p, Z / p.illum[2]);
  L = 116.0f * Y - 16.0f;
  const float h = 0.01f * L;
  a = h * (500.0f * (X - Y));
  b = h * (200.0f * (Y - Z));
}

__global__ __launch_bounds__(kFlipThreads) void flip_kernel(FlipParams p) {
  extern __shared__ __attribute__((aligned(16))) char flip_lds[];
  float* s = reinterpret_cast<float*>(flip_lds);      // [test Y, Cx, Cz, ref Y, Cx, Cz][S][S]
  const int t = threadIdx.x;
  const int S = kFlipTile + 2 * p.halo;
  const int plane = S * S;
  const int tile_y = static_cast<int>(blockIdx.x) / p.tiles_x;
  const int x0 = (static_cast<int>(blockIdx.x) - tile_y * p.tiles_x) * kFlipTile, y0 = tile_y * kFlipTile;

  for (int i = t; i < plane; i += kFlipThreads) {
    const int ly = i / S, lx = i - ly * S;
    const int gx = min(max(x0 + lx - p.halo, 0), p.width - 1), gy = min(max(y0 + ly - p.halo, 0), p.height - 1);
    const size_t g = (static_cast<size_t>(gy) * p.width + gx) * 3;
    flip_srgb_to_ycxcz(p, p.test[g], p.test[g + 1], p.test[g + 2], s[i], s[plane + i], s[2 * plane + i]);
    flip_srgb_to_ycxcz(p, p.ref[g], p.ref[g + 1], p.ref[g + 2], s[3 * plane + i], s[4 * plane + i], s[5 * plane + i]);
  }
  __syncthreads();

  const int tx = t & 31, ty = t >> 5;
  float dc[4];
  {   // colour pipeline
    const int n = 2 * p.rc + 1, o0 = (p.halo - p.rc) * (S + 1);
    const float* wa = p.tab;
    const float* wrg = wa + n * n;
    const float* wby = wrg + n * n;
    float acc[4][6];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[k][c] = 0.0f;
    for (int dy = 0; dy < n; ++dy)
      for (int dx = 0; dx < n; ++dx) {
        const float a = wa[dy * n + dx], rg = wrg[dy * n + dx], by = wby[dy * n + dx];      // uniform: scalar loads
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int o = o0 + (ty + 8 * k + dy) * S + tx + dx;
          acc[k][0] += a * s[o];
          acc[k][1] += rg * s[plane + o];
          acc[k][2] += by * s[2 * plane + o];
          acc[k][3] += a * s[3 * plane + o];
          acc[k][4] += rg * s[4 * plane + o];
          acc[k][5] += by * s[5 * plane + o];
        }
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float Lt, at, bt, Lr, ar, br;
      flip_ycxcz_to_hunt_lab(p, acc[k][0], acc[k][1], acc[k][2], Lt, at, bt);
      flip_ycxcz_to_hunt_lab(p, acc[k][3], acc[k][4], acc[k][5], Lr, ar, br);
      const float da = at - ar, db = bt - br;
      const float e = powf(fabsf(Lt - Lr) + sqrtf(da * da + db * db), 0.7f);      // HyAB ^ qc
      dc[k] = e < p.pccmax ? p.lo_scale * e : p.pt + ((e - p.pccmax) / p.hi_div) * p.one_minus_pt;
    }
  }
  __syncthreads();

  // feature pipeline: the luminance planes become (Y + 16) / 116 in place
  for (int i = t; i < plane; i += kFlipThreads) {
    s[i] = (s[i] + 16.0f) / 116.0f;
    s[3 * plane + i] = (s[3 * plane + i] + 16.0f) / 116.0f;
  }
  __syncthreads();

  float out[4];
  {
    const int nc = 2 * p.rc + 1, n = 2 * p.rf + 1, o0 = (p.halo - p.rf) * (S + 1);
    const float* we = p.tab + 3 * nc * nc;
    const float* wp = we + n * n;
    float acc[4][8];      // test / ref x edge / point x (x, y)
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[k][c] = 0.0f;
    for (int dy = 0; dy < n; ++dy)
      for (int dx = 0; dx < n; ++dx) {
        const float ex = we[dy * n + dx], ey = we[dx * n + dy], px = wp[dy * n + dx], py = wp[dx * n + dy];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int o = o0 + (ty + 8 * k + dy) * S + tx + dx;
          const float vt = s[o], vr = s[3 * plane + o];
          acc[k][0] += ex * vt;
          acc[k][1] += ey * vt;
          acc[k][2] += px * vt;
          acc[k][3] += py * vt;
          acc[k][4] += ex * vr;
          acc[k][5] += ey * vr;
          acc[k][6] += px * vr;
          acc[k][7] += py * vr;
        }
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float et = sqrtf(acc[k][0] * acc[k][0] + acc[k][1] * acc[k][1]), pt = sqrtf(acc[k][2] * acc[k][2] + acc[k][3] * acc[k][3]);
      const float er = sqrtf(acc[k][4] * acc[k][4] + acc[k][5] * acc[k][5]), pr = sqrtf(acc[k][6] * acc[k][6] + acc[k][7] * acc[k][7]);
      const float df = flip_clamp01(sqrtf(p.inv_sqrt2 * flip_max(fabsf(et - er), fabsf(pt - pr))));      // ^ qf = 0.5
      out[k] = powf(dc[k], 1.0f - df);      // IEEE pow: 0^0 = 1
    }
  }

  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int gx = x0 + tx, gy = y0 + ty + 8 * k;
    if (gx < p.width && gy < p.height) {
      if (p.map) p.map[static_cast<size_t>(gy) * p.width + gx] = out[k];
      sum += static_cast<double>(out[k]);
    }
  }
  __syncthreads();      // the image planes are dead: the tree below reuses their LDS
  double* red = reinterpret_cast<double*>(flip_lds);
  red[t] = sum;
  __syncthreads();
  for (int w = kFlipThreads / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) p.partial[blockIdx.x] = red[0];
}

// mean = (sum of the per-tile sums, in a fixed order) / pixels
__global__ __launch_bounds__(kFlipThreads) void flip_mean_kernel(const double* __restrict__ partial, int n, double pixels, float* __restrict__ mean) {
  __shared__ double red[kFlipThreads];
  const int t = threadIdx.x;
  double sum = 0.0;
  for (int i = t; i < n; i += kFlipThreads) sum += partial[i];
  red[t] = sum;
  __syncthreads();
  for (int w = kFlipThreads / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) *mean = static_cast<float>(red[0] / pixels);
}

}  // namespace adanerf
