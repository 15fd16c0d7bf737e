#include "flip_tables.hpp"

#include <algorithm>
#include <cmath>

namespace adanerf {

// generate_spatial_filter (flip_loss.py:112-154): a1 sqrt(pi / b1) exp(-pi^2 z / b1) + a2 sqrt(pi / b2) exp(-pi^2 z / b2), normalised by its own sum
static void flip_spatial_filter(double ppd, int r, double a1, double b1, double a2, double b2, float* out) {
  const int n = 2 * r + 1;
  const double dx = 1.0 / ppd;
  std::vector<double> g(static_cast<size_t>(n) * n);
  double sum = 0.0;
  for (int y = -r; y <= r; ++y)
    for (int x = -r; x <= r; ++x) {
      const double z = (x * dx) * (x * dx) + (y * dx) * (y * dx);
      const double v = a1 * std::sqrt(kFlipPi / b1) * std::exp(-(kFlipPi * kFlipPi) * z / b1) + a2 * std::sqrt(kFlipPi / b2) * std::exp(-(kFlipPi * kFlipPi) * z / b2);
      g[static_cast<size_t>(y + r) * n + (x + r)] = v;
      sum += v;
    }
  for (size_t i = 0; i < g.size(); ++i) out[i] = static_cast<float>(g[i] / sum);
}

// feature_detection (flip_loss.py:213-240): first (edge) or second (point) x derivative of a Gaussian; the table goes to fp32, then the
// positive and the negative weights are normalised separately, in fp32
static void flip_feature_filter(double sd, int r, bool point, float* out) {
  const int n = 2 * r + 1;
  std::vector<double> g(static_cast<size_t>(n) * n);
  double neg = 0.0, pos = 0.0;
  for (int y = -r; y <= r; ++y)
    for (int x = -r; x <= r; ++x) {
      const double e = std::exp(-static_cast<double>(x * x + y * y) / (2 * sd * sd));
      const double v = point ? (static_cast<double>(x * x) / (sd * sd) - 1) * e : -static_cast<double>(x) * e;
      g[static_cast<size_t>(y + r) * n + (x + r)] = v;
      if (v < 0) neg -= v;
      if (v > 0) pos += v;
    }
  const float fneg = static_cast<float>(neg), fpos = static_cast<float>(pos);
  for (size_t i = 0; i < g.size(); ++i) {
    const float v = static_cast<float>(g[i]);
    out[i] = v < 0.0f ? v / fneg : v / fpos;
  }
}

// linear RGB -> hunt-adjusted L*a*b* in fp64 (the two primaries behind cmax, flip_loss.py:82-84)
static void flip_hunt_lab64(const double A[9], const double illum[3], const double rgb[3], double lab[3]) {
  double f[3];
  for (int i = 0; i < 3; ++i) {
    const double t = (A[3 * i] * rgb[0] + A[3 * i + 1] * rgb[1] + A[3 * i + 2] * rgb[2]) / illum[i];
    const double delta = 6.0 / 29.0;
    f[i] = t > 0.00885 ? std::pow(t, 1.0 / 3.0) : t / (3 * delta * delta) + 4.0 / 29.0;
  }
  lab[0] = 116 * f[1] - 16;
  lab[1] = 0.01 * lab[0] * (500 * (f[0] - f[1]));
  lab[2] = 0.01 * lab[0] * (200 * (f[1] - f[2]));
}

bool flip_tables(double ppd, std::vector<float>* tab, FlipParams* out) {
  const int rc = static_cast<int>(std::ceil(3 * std::sqrt(0.04 / (2 * kFlipPi * kFlipPi)) * ppd));      // the largest scale parameter is BY's 0.04
  const double sd = 0.5 * 0.082 * ppd;
  const int rf = static_cast<int>(std::ceil(3 * sd));
  if (rc < 1 || rf < 1 || rc > kFlipMaxRadius || rf > kFlipMaxRadius) return false;
  const size_t nc = static_cast<size_t>(2 * rc + 1) * (2 * rc + 1), nf = static_cast<size_t>(2 * rf + 1) * (2 * rf + 1);
  tab->assign(3 * nc + 2 * nf, 0.f);
  flip_spatial_filter(ppd, rc, 1, 0.0047, 0, 1e-5, tab->data());
  flip_spatial_filter(ppd, rc, 1, 0.0053, 0, 1e-5, tab->data() + nc);
  flip_spatial_filter(ppd, rc, 34.1, 0.04, 13.5, 0.025, tab->data() + 2 * nc);
  flip_feature_filter(sd, rf, false, tab->data() + 3 * nc);
  flip_feature_filter(sd, rf, true, tab->data() + 3 * nc + nf);

  *out = FlipParams{};
  FlipParams& p = *out;
  p.rc = rc;
  p.rf = rf;
  p.halo = std::max(rc, rf);
  // flip_loss.py:264-272 (D65); the reference holds the matrix in fp32 and inverts that
  const double frac[9] = {10135552.0 / 24577794, 8788810.0 / 24577794, 4435075.0 / 24577794, 2613072.0 / 12288897, 8788810.0 / 12288897,
                          887015.0 / 12288897,   1425312.0 / 73733382, 8788810.0 / 73733382, 70074185.0 / 73733382};
  double A[9], inv[9], illum[3];
  for (int i = 0; i < 9; ++i) A[i] = p.rgb2xyz[i] = static_cast<float>(frac[i]);
  const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
  inv[0] = (A[4] * A[8] - A[5] * A[7]) / det;
  inv[1] = (A[2] * A[7] - A[1] * A[8]) / det;
  inv[2] = (A[1] * A[5] - A[2] * A[4]) / det;
  inv[3] = (A[5] * A[6] - A[3] * A[8]) / det;
  inv[4] = (A[0] * A[8] - A[2] * A[6]) / det;
  inv[5] = (A[2] * A[3] - A[0] * A[5]) / det;
  inv[6] = (A[3] * A[7] - A[4] * A[6]) / det;
  inv[7] = (A[1] * A[6] - A[0] * A[7]) / det;
  inv[8] = (A[0] * A[4] - A[1] * A[3]) / det;
  for (int i = 0; i < 9; ++i) p.xyz2rgb[i] = static_cast<float>(inv[i]);
  for (int i = 0; i < 3; ++i) p.illum[i] = static_cast<float>(illum[i] = A[3 * i] + A[3 * i + 1] + A[3 * i + 2]);
  p.lab_div = static_cast<float>(3 * (6.0 / 29.0) * (6.0 / 29.0));
  p.lab_add = static_cast<float>(4.0 / 29.0);
  // cmax = HyAB(green, blue) ^ qc in fp64; redistribute_errors' scalars (pc = 0.4, pt = 0.95) go to fp32 as torch applies them
  const double green[3] = {0, 1, 0}, blue[3] = {0, 0, 1};
  double lg[3], lb[3];
  flip_hunt_lab64(A, illum, green, lg);
  flip_hunt_lab64(A, illum, blue, lb);
  const double cmax = std::pow(std::fabs(lg[0] - lb[0]) + std::sqrt((lg[1] - lb[1]) * (lg[1] - lb[1]) + (lg[2] - lb[2]) * (lg[2] - lb[2])), 0.7);
  const double pccmax = 0.4 * cmax;
  p.pccmax = static_cast<float>(pccmax);
  p.lo_scale = static_cast<float>(0.95 / pccmax);
  p.hi_div = static_cast<float>(cmax - pccmax);
  p.pt = static_cast<float>(0.95);
  p.one_minus_pt = static_cast<float>(1.0 - 0.95);
  p.inv_sqrt2 = static_cast<float>(1 / std::sqrt(2.0));
  return true;
}

}  // namespace adanerf
