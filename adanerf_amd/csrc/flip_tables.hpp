// Host-only: tables and constants of src/util/flip_loss.py for one pixels-per-degree value (adanerf_flip), built in fp64 and
// rounded to fp32 where the reference rounds (torch.Tensor(g)).
#pragma once
#include <vector>

#include "params.hpp"

namespace adanerf {

constexpr double kFlipPi = 3.14159265358979323846;
constexpr double kFlipDefaultPpd = 0.7 * (3840 / 0.7) * (kFlipPi / 180);      // flip_loss.py:55
constexpr double kFlipPpdMin = 10.0, kFlipPpdMax = 140.0;

// The filter table FlipParams::tab points at once uploaded (A, RG, BY, then edge, point) and every FlipParams field that depends on
// ppd alone (radii, colour constants); the image fields stay zero.  false: a filter radius outside 1..kFlipMaxRadius at this ppd.
bool flip_tables(double ppd, std::vector<float>* tab, FlipParams* p);

}  // namespace adanerf
