// N10: the foveated ray density rule (adanerf_foveate_density / adanerf_host_density_mask), in integers.  Plain C++ with no HIP include: the
// mask kernel (k_density.hip.hpp) and the host mirror (model_setup.cpp) compile this one text, so the two cannot drift.
//   ring      adanerf_foveate's: q = (2 x + 1 - gx2)^2 + (2 y + 1 - gy2)^2 against (2 radius_k)^2, the first ring that contains the pixel
//             gives its stride s(x, y), the entry behind the last ring outside them all
//   rendered  pixel (x, y) iff for some level L of 1, 2, 4, 8: the pixel lies on the lattice of L -- ((x - phase_x) & (L - 1)) == 0 and the
//             same in y; at phase (0, 0): L divides x and y -- and the pixel of the box of L - 1 pixels around it (clipped to the frame)
//             whose centre lies nearest the gaze has a stride <= L.  Strides never decrease outward, so that pixel carries the smallest
//             stride of the box: a lattice point of level L is rendered as soon as any pixel that may use it as a corner (within L - 1
//             of it per axis) has stride L or finer, also when the point itself sits in a coarser ring.
//   byte      0 for a rendered pixel, else the pixel's own stride (2, 4 or 8: a pixel of stride 1 passes at L = 1)
//   cell      a pixel of byte s takes, per axis, the lattice points either side of it: m = (x - phase_x) & (s - 1), x0 = x - m, x1 = x0 + s
//             (density_cell_axis).  m <= s - 1 and x1 - x = s - m <= s - 1 where m != 0, so a corner lies within s - 1 of every pixel that
//             uses it, whatever the phase: the pixel is in the corner's box, its stride is s, and the corner is rendered at level s.  The
//             phase moves the lattice and nothing else; a corner outside the frame is not used (one tap, or none on a frame narrower than s).
//   phase     phase_x, phase_y in 0..7, the same for every level (level L sees them mod L); density_phase gives the phase of frame k
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADN_DENSITY_FN __host__ __device__ inline
#else
#define ADN_DENSITY_FN inline
#endif

namespace adanerf {

constexpr int kDensityMaxRings = 8;      // adanerf_foveate's limit (kFoveaMaxRings)

// Filled by density_rule_fill; the slots behind the rings in use contain nothing (r2x4 = 2^64 - 1) and carry the outside stride, so the
// walk below has constant bounds.  |gx2|, |gy2| <= 2^31 and x, y < 2^25: q < 2^64 (FoveaParams, k_budget.hip.hpp).
struct DensityRule {
  int64_t gx2, gy2;
  uint64_t r2x4[kDensityMaxRings];
  uint8_t stride[kDensityMaxRings + 1];
  int32_t phase_x, phase_y;      // 0..7
};

// Checks the arguments as the header states them and fills `out`; returns what is wrong, or nullptr.
inline const char* density_rule_fill(float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride, DensityRule* out,
                                     int32_t phase_x = 0, int32_t phase_y = 0) {
  if (!std::isfinite(gaze_x) || !std::isfinite(gaze_y)) return "the gaze must be finite";
  if (n_rings < 0 || n_rings > kDensityMaxRings) return "n_rings must be in 0..8";
  if ((n_rings > 0 && !radius_px) || !stride) return "NULL array";
  if (phase_x < 0 || phase_x > 7 || phase_y < 0 || phase_y > 7) return "phase_x and phase_y must be in 0..7";
  DensityRule f{};
  f.phase_x = phase_x;
  f.phase_y = phase_y;
  for (int k = 0; k < n_rings; ++k) {
    if (radius_px[k] < 0 || (k > 0 && radius_px[k] <= radius_px[k - 1])) return "radii must be >= 0 and strictly ascending";
    const uint64_t d = 2ull * static_cast<uint64_t>(radius_px[k]);
    f.r2x4[k] = d * d;
  }
  for (int k = 0; k <= n_rings; ++k) {
    const int32_t s = stride[k];
    if (s != 1 && s != 2 && s != 4 && s != 8) return "every stride must be 1, 2, 4 or 8";
    if (k > 0 && s < stride[k - 1]) return "strides must not decrease outward";
    f.stride[k] = static_cast<uint8_t>(s);
  }
  for (int k = n_rings; k < kDensityMaxRings; ++k) {
    f.r2x4[k] = ~0ull;
    f.stride[k + 1] = f.stride[n_rings];
  }
  // twice the gaze, to the nearest integer (ties to even), clamped as adanerf_foveate clamps it
  const auto half_px = [](float g) { return static_cast<int64_t>(std::lrintf(std::fmin(std::fmax(2.0f * g, -2147483648.0f), 2147483648.0f))); };
  f.gx2 = half_px(gaze_x);
  f.gy2 = half_px(gaze_y);
  *out = f;
  return nullptr;
}

// s(x, y)
ADN_DENSITY_FN int density_stride(const DensityRule& f, int x, int y) {
  const int64_t dx = 2 * static_cast<int64_t>(x) + 1 - f.gx2, dy = 2 * static_cast<int64_t>(y) + 1 - f.gy2;
  const uint64_t q = static_cast<uint64_t>(dx * dx) + static_cast<uint64_t>(dy * dy);
  int s = f.stride[0];
  for (int j = 0; j < kDensityMaxRings; ++j)      // radii ascend: the rings that do not contain the pixel come first
    if (q > f.r2x4[j]) s = f.stride[j + 1];
  return s;
}

// The integer c of [lo, hi] that minimises |2 c + 1 - g2|, the lower c on a tie: without the interval it is floor((g2 - 1) / 2) (g2 odd: the
// centre on the gaze; g2 even: the lower of the two centres half a pixel from it), and the distance grows to either side of that.
ADN_DENSITY_FN int density_nearest(int64_t g2, int lo, int hi) {
  const int64_t c = (g2 - 1) >> 1;
  return c < lo ? lo : (c > hi ? hi : static_cast<int>(c));
}

// the mask byte of pixel (x, y) of a w x h frame
ADN_DENSITY_FN uint8_t density_mask_byte(const DensityRule& f, int x, int y, int w, int h) {
  const int own = density_stride(f, x, y);
  if (own == 1) return 0;      // L = 1: the box is the pixel
  const int lx = x - f.phase_x, ly = y - f.phase_y;      // may be negative: the low bits of two's complement are the residue
  for (int L = 2; L <= 8; L *= 2) {
    if ((lx | ly) & (L - 1)) break;      // off the lattice of L, and so of every larger level
    const int x_lo = x - L + 1 > 0 ? x - L + 1 : 0, x_hi = x + L - 1 < w - 1 ? x + L - 1 : w - 1;
    const int y_lo = y - L + 1 > 0 ? y - L + 1 : 0, y_hi = y + L - 1 < h - 1 ? y + L - 1 : h - 1;
    if (density_stride(f, density_nearest(f.gx2, x_lo, x_hi), density_nearest(f.gy2, y_lo, y_hi)) <= L) return 0;
  }
  return static_cast<uint8_t>(own);
}

// One axis of the cell of a pixel with byte s at coordinate c of an axis of n pixels: the lattice points either side of it that lie in
// the frame.  c1 == c0: one tap (the pixel is on the lattice, or one side is outside); none: neither side exists.
struct DensityAxis {
  int c0, c1;
  int m;      // (c - phase) & (s - 1): the weight of c1 is m / s
  bool none;
};
ADN_DENSITY_FN DensityAxis density_cell_axis(int c, int phase, int s, int n) {
  DensityAxis a;
  a.m = (c - phase) & (s - 1);
  const int lo = c - a.m, hi = lo + s;
  const bool has_lo = lo >= 0, has_hi = hi < n;
  a.none = a.m != 0 && !has_lo && !has_hi;
  a.c0 = (a.m == 0 || has_lo) ? lo : hi;
  a.c1 = (a.m != 0 && has_lo && has_hi) ? hi : a.c0;
  return a;
}

// Frame k's phase: k mod 64 in base 4, digit i placing bit i.  k mod L^2 fixes (phase_x mod L, phase_y mod L) one to one, so any L^2
// consecutive frames put every residue pair mod L on the lattice exactly once, for L = 2, 4 and 8 at the same time.
inline void density_phase(int32_t k, int32_t* phase_x, int32_t* phase_y) {
  const uint32_t kk = static_cast<uint32_t>(k) & 63u;      // k mod 64, also for a negative k
  int32_t px = 0, py = 0;
  for (int i = 0; i < 3; ++i) {
    const uint32_t d = (kk >> (2 * i)) & 3u;
    px |= static_cast<int32_t>((d == 1 || d == 2) ? 1 : 0) << i;      // bx = {0, 1, 1, 0}
    py |= static_cast<int32_t>((d == 1 || d == 3) ? 1 : 0) << i;      // by = {0, 1, 0, 1}
  }
  *phase_x = px;
  *phase_y = py;
}

}  // namespace adanerf
