// N3: the frame at the window's size -- the headless counterpart of the viewer's blit from its render buffer to the window
// (adanerf_real_time_viewer/src/interoprenderbuffer.cpp:87: linear filtering if the window is wider than the frame, nearest otherwise,
// y flipped for GL's origin).  GL leaves the rounding of a linear blit to the implementation; here it is defined in integers, so the
// kernel is exact against a restatement (tests/present_reference.py).  Per axis, destination pixel x of d from a source of s pixels,
// D = 2 d:  n = (2 x + 1) s - d,  i0 = floor(n / D),  f = n - i0 D;  taps clamp(i0), clamp(i0 + 1) with weights D - f, f (pixel
// centres: equal sizes give the identity).  Per channel v = the four weighted taps (<= 255 D E < 2^38, E = 2 dst_h),
// out = floor((2 v + D E) / (2 D E)).  Nearest: i = min(floor((2 x + 1) s / D), s - 1).
// Bandwidth- and launch-bound: a thread per four adjacent destination pixels of one row, one 16-byte store where the group is whole;
// the pixels in front of a row's first 16-byte boundary and the ragged row end go out as 4-byte stores.  No LDS, no floating point.
#pragma once
#include "k_common.hip.hpp"

namespace adanerf {

constexpr int kPresentMaxSide = 16384;      // (2 x + 1) s < 2^29 and 2 D E <= 2^31: the 32-bit pieces below cannot overflow

// one axis of the linear filter: the two clamped taps and the weight f of the second (the first has D - f)
__device__ inline void present_taps(int x, int s, int d, int* t0, int* t1, uint32_t* f) {
  const int D = 2 * d, n = (2 * x + 1) * s - d;      // n > -D: floor(n / D) is -1 for every negative n
  const int i0 = n < 0 ? -1 : static_cast<int>(static_cast<uint32_t>(n) / static_cast<uint32_t>(D));
  *f = static_cast<uint32_t>(n - i0 * D);
  *t0 = max(i0, 0);
  *t1 = min(i0 + 1, s - 1);
}

__device__ inline int present_nearest(int x, int s, int d) {
  return min(static_cast<int>(static_cast<uint32_t>((2 * x + 1) * s) / static_cast<uint32_t>(2 * d)), s - 1);
}

// den = 2 D E, magic = floor((2^64 - 1) / den): the high half of num x magic is floor(num / den) or one less for num < 2^41
__device__ inline uint32_t present_channel(uint32_t c00, uint32_t c01, uint32_t c10, uint32_t c11, uint32_t wx0, uint32_t wx1, uint32_t wy0,
                                           uint32_t wy1, uint64_t den, uint64_t magic) {
  const uint64_t v = static_cast<uint64_t>(wy0) * (wx0 * c00 + wx1 * c01) + static_cast<uint64_t>(wy1) * (wx0 * c10 + wx1 * c11);
  const uint64_t num = 2 * v + (den >> 1);
  uint32_t q = static_cast<uint32_t>(__umul64hi(num, magic));
  if (num - q * den >= den) ++q;
  return q;
}

// src [src_h][src_w], dst [dst_h][dst_w], both row-major uchar4 at 4-byte-aligned addresses.  dst_px_phase = (address of dst / 4) & 3.
// Thread (row y, group g): g = 0 owns the `lead` pixels in front of the row's first 16-byte boundary, g >= 1 the four from
// lead + 4 (g - 1) on.  flip: row y of the result is written to row dst_h - 1 - y.
__global__ __launch_bounds__(256) void present_kernel(const uchar4* __restrict__ src, uchar4* __restrict__ dst, int src_w, int src_h, int dst_w,
                                                      int dst_h, int linear, int flip, uint32_t dst_px_phase, uint64_t den, uint64_t magic) {
  const int groups = 1 + (dst_w + 3) / 4;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;      // groups * dst_h <= 4097 * 16384 < 2^31
  const int y = t / groups, g = t - y * groups;
  if (y >= dst_h) return;
  const size_t row = static_cast<size_t>(flip ? dst_h - 1 - y : y) * dst_w;
  const int lead = static_cast<int>((4u - ((dst_px_phase + static_cast<uint32_t>(row)) & 3u)) & 3u);
  const int x0 = g == 0 ? 0 : lead + 4 * (g - 1);
  const int x1 = min(g == 0 ? lead : x0 + 4, dst_w);
  if (x0 >= x1) return;
  uchar4 px[4];
  if (linear) {
    int ya, yb;
    uint32_t fy;
    present_taps(y, src_h, dst_h, &ya, &yb, &fy);
    const uchar4* r0 = src + static_cast<size_t>(ya) * src_w;
    const uchar4* r1 = src + static_cast<size_t>(yb) * src_w;
    const uint32_t wy0 = 2u * dst_h - fy, wy1 = fy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x0 + k >= x1) break;
      int xa, xb;
      uint32_t fx;
      present_taps(x0 + k, src_w, dst_w, &xa, &xb, &fx);
      const uint32_t wx0 = 2u * dst_w - fx, wx1 = fx;
      const uchar4 p00 = r0[xa], p01 = r0[xb], p10 = r1[xa], p11 = r1[xb];
      px[k].x = static_cast<unsigned char>(present_channel(p00.x, p01.x, p10.x, p11.x, wx0, wx1, wy0, wy1, den, magic));
      px[k].y = static_cast<unsigned char>(present_channel(p00.y, p01.y, p10.y, p11.y, wx0, wx1, wy0, wy1, den, magic));
      px[k].z = static_cast<unsigned char>(present_channel(p00.z, p01.z, p10.z, p11.z, wx0, wx1, wy0, wy1, den, magic));
      px[k].w = static_cast<unsigned char>(present_channel(p00.w, p01.w, p10.w, p11.w, wx0, wx1, wy0, wy1, den, magic));
    }
  } else {
    const uchar4* r = src + static_cast<size_t>(present_nearest(y, src_h, dst_h)) * src_w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x0 + k >= x1) break;
      px[k] = r[present_nearest(x0 + k, src_w, dst_w)];
    }
  }
  uchar4* out = dst + row + x0;
  if (g != 0 && x1 - x0 == 4) {      // a whole group: (dst_px_phase + row + x0) & 3 == 0 by the choice of lead
    u32x4 q;
    q.x = static_cast<uint32_t>(px[0].x) | static_cast<uint32_t>(px[0].y) << 8 | static_cast<uint32_t>(px[0].z) << 16 | static_cast<uint32_t>(px[0].w) << 24;
    q.y = static_cast<uint32_t>(px[1].x) | static_cast<uint32_t>(px[1].y) << 8 | static_cast<uint32_t>(px[1].z) << 16 | static_cast<uint32_t>(px[1].w) << 24;
    q.z = static_cast<uint32_t>(px[2].x) | static_cast<uint32_t>(px[2].y) << 8 | static_cast<uint32_t>(px[2].z) << 16 | static_cast<uint32_t>(px[2].w) << 24;
    q.w = static_cast<uint32_t>(px[3].x) | static_cast<uint32_t>(px[3].y) << 8 | static_cast<uint32_t>(px[3].z) << 16 | static_cast<uint32_t>(px[3].w) << 24;
    *reinterpret_cast<u32x4*>(out) = q;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < x1) out[k] = px[k];
  }
}

// ADANERF_PRESENT_AREA: the exact area (box) filter for any pair of sizes, per axis in units of 1 / dst of a source pixel.  Destination
// pixel x covers [x s, (x + 1) s), source pixel i covers [i d, (i + 1) d); the weight is the overlap, the contributing i run from
// floor(x s / d) to floor(((x + 1) s - 1) / d) and their weights sum to s.  Per channel V = sum_j sum_i wy wx v <= 255 S, S = src_w src_h
// <= 2^28, out = floor((2 V + S) / (2 S)): half up.  den = 2 S and magic as in present_channel (2 V + S < 2^38).  The host admits
// src <= 8 dst per axis: at most 9 taps.  A thread per destination pixel, one 4-byte store each, consecutive threads consecutive pixels.
__global__ __launch_bounds__(256) void present_area_kernel(const uchar4* __restrict__ src, uchar4* __restrict__ dst, int src_w, int src_h,
                                                           int dst_w, int dst_h, int flip, uint64_t den, uint64_t magic) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;      // dst_w * dst_h <= 2^28
  const int y = t / dst_w, x = t - y * dst_w;
  if (y >= dst_h) return;
  const int xa = x * src_w, xb = xa + src_w, ya = y * src_h, yb = ya + src_h;      // < 2^28 + 2^14
  const int i0 = xa / dst_w, i1 = (xb - 1) / dst_w, j0 = ya / dst_h, j1 = (yb - 1) / dst_h;
  uint64_t v[4] = {0, 0, 0, 0};
  for (int j = j0; j <= j1; ++j) {
    const uint32_t wy = static_cast<uint32_t>(min((j + 1) * dst_h, yb) - max(j * dst_h, ya));
    const uchar4* row = src + static_cast<size_t>(j) * src_w;
    uint32_t r[4] = {0, 0, 0, 0};      // sum_i wx v <= 255 src_w < 2^22
    for (int i = i0; i <= i1; ++i) {
      const uint32_t wx = static_cast<uint32_t>(min((i + 1) * dst_w, xb) - max(i * dst_w, xa));
      const uchar4 p = row[i];
      r[0] += wx * p.x;
      r[1] += wx * p.y;
      r[2] += wx * p.z;
      r[3] += wx * p.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += static_cast<uint64_t>(wy) * r[k];
  }
  unsigned char o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t num = 2 * v[k] + (den >> 1);
    uint32_t q = static_cast<uint32_t>(__umul64hi(num, magic));
    if (num - q * den >= den) ++q;
    o[k] = static_cast<unsigned char>(q);
  }
  dst[static_cast<size_t>(flip ? dst_h - 1 - y : y) * dst_w + x] = make_uchar4(o[0], o[1], o[2], o[3]);
}

}  // namespace adanerf
