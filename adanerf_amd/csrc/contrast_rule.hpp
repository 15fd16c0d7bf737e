// N11: the contrast rule of adaptive supersampling (adanerf_contrast_mask / adanerf_host_contrast_mask).  Plain C++ with no HIP include: the
// mask kernel (k_contrast.hip.hpp) and the host mirror (model_setup.cpp) compile this one text, so the two cannot drift.
//   display value  v(p, ch) = fminf(fmaxf(rgb[3 p + ch], 0), 1): the clamp of rgba8_of (k_accumulate.hip.hpp), so a NaN is 0 and an infinity
//                  is 0 or 1; a -0 may stay -0, which no difference below tells from +0
//   contrast       c(p, q) = max over ch of |v(p, ch) - v(q, ch)|, each difference one rounded fp32 subtraction
//   flagged        p iff some q among its up to 8 neighbours inside the image has c(p, q) > threshold: strict, in fp32.  The relation is
//                  symmetric (|a - b| and |b - a| are the same float), so both sides of an edge are flagged; a 1 x 1 image flags nothing
//   byte           0 for a flagged pixel (render more), 1 for every other: adanerf_render_masked(values = 1) selects the flagged ones
// The rule takes the pixels through three loaders of DISPLAY values -- load(ch, x, y), called for pixels inside the image only -- so the
// kernel hands it its LDS tile of values clamped once and the host hands it the image with the clamp applied on the way.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADN_CONTRAST_FN __host__ __device__ inline
#else
#define ADN_CONTRAST_FN inline
#endif

namespace adanerf {

constexpr int kContrastMaxSide = 16384;      // adanerf_present's limit (kPresentMaxSide)

// v of one stored value
ADN_CONTRAST_FN float contrast_display(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// what is wrong with the arguments that do not depend on a device, or nullptr
inline const char* contrast_rule_check(int32_t width, int32_t height, float threshold) {
  if (width < 1 || width > kContrastMaxSide || height < 1 || height > kContrastMaxSide) return "width and height must be in 1..16384";
  if (!std::isfinite(threshold) || threshold < 0.f || threshold > 1.f) return "the threshold must be finite and lie in [0, 1]";
  return nullptr;
}

// the mask byte of pixel (x, y) of a w x h image; r, g, b: float(int x, int y), the display value of one channel
template <class LoadR, class LoadG, class LoadB>
ADN_CONTRAST_FN uint8_t contrast_mask_byte(int x, int y, int w, int h, float threshold, LoadR r, LoadG g, LoadB b) {
  const float pr = r(x, y), pg = g(x, y), pb = b(x, y);
  bool flagged = false;
  for (int dy = -1; dy <= 1; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= h) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= w || (dx == 0 && dy == 0)) continue;
      const float c = fmaxf(fmaxf(fabsf(pr - r(qx, qy)), fabsf(pg - g(qx, qy))), fabsf(pb - b(qx, qy)));
      flagged = flagged || c > threshold;
    }
  }
  return flagged ? 0 : 1;
}

}  // namespace adanerf
