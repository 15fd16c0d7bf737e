// Host-only: the model-directory validator.  Parses config.ini / dataset_info.txt, checks them against what the library renders and
// derives every per-context constant (ray generation, normalisation, depth tables).  No device code, no HIP header.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/adanerf_hip.h"
#include "format.hpp"
#include "layout.hpp"
#include "pack.hpp"
#include "params.hpp"

namespace adanerf {

// message of the last failed call that had no context to keep it (adanerf_last_error(NULL))
extern thread_local std::string g_create_error;

struct ModelSetup {
  // What bounds the sample positions the bf16 shading path's scaled layers may see (pack.hpp kPosIdentityBound): kept so that adanerf_set_camera can
  // check a pose outside the view cell (a free-fly viewer) instead of letting the clamped conversion cut activations silently.
  struct PosBound {
    bool active = false;      // bf16 shading and not NDC
    int normalize = 0;
    double cmax = 0, zmax = 0, off = 0, M = 1, rad = 0;
    double center[3] = {0, 0, 0};
    // largest |encoded position| for a camera `dcam` away from the view-cell centre: the ray starts on (or, outside the cell, within dcam + rad of) the
    // cell's sphere and runs zmax further along a unit direction
    double at(double dcam) const {
      const double reach = std::max(2.0 * rad, 2.0 * dcam + rad);
      const double world = cmax + reach + zmax, local = reach + zmax + off;
      if (normalize == kNormMaxDepth) return world / M;
      if (normalize == kNormCentered) return local;
      if (normalize == kNormMaxDepthCentered) return local / M;
      if (normalize == kNormInverseSqrtDistCentered) return std::sqrt(local / M);
      if (normalize != kNormNone) return local;      // InverseDistCentered (<= |l|), LogCentered (<= |l| for max_depth >= e - 1 ... kept loose)
      return world;
    }
  };

  PosBound pos_bound;
  Config cfg;
  adanerf_info info{};
  RayGenParams rg{};
  ShadeParams sp{};
  int mult_mode = 1;
  int transform = 0;
  int fp0 = 10, fd0 = 4, fp1 = 10, fd1 = 4;
  int ray_samples = 0;
  std::vector<float> rsi_z;
  std::vector<float> ztab;       // depth table in force: bin centres, or the dense mode's t-values at threshold 0 (depth_table)
  int sel_n = 0;                 // N and threshold as stated by the config or the last caller who overrode them (coarse/fine: Nf): what
  float sel_thr = 0.f;           // "keep" means to select_samples
  int bins = 128;                 // multiDepthFeatures: depth cells of the adaptive sampler (src/nerf_raymarch_common.py:675-677, 726-727)
  DepthMap dm{};
  bool coarse_fine = false;
  int n_coarse = 0;
  std::vector<float> ztab_coarse;
  int normalize0 = 0;      // kNorm* of the coarse pass
};

// Parse + validate the model directory and derive every per-context constant.  No exception leaves it: whatever a damaged or hostile
// model directory makes the loader throw (std::bad_alloc, std::length_error) comes back as a status + message
// (tests/host_sanitize_fuzz.cpp runs the loader itself under ASan / UBSan on mutated directories).
int setup_model(const char* model_dir, const adanerf_options* opt, ModelSetup* ms, std::string* err);
int setup_model_unguarded(const char* model_dir, const adanerf_options* opt, ModelSetup* ms, std::string* err);

// Everything a context derives from (N, threshold) on the host, for adanerf_create and adanerf_set_selection alike: resolves the pair
// (num_samples <= 0 / threshold < 0 keep what is in force), validates it against the model and the batch size, and fills
// info.num_samples / .threshold / .dense, ztab and pos_bound.zmax.  On failure *ms is unchanged.  Needs every model-derived field
// of *ms (setup_model calls it last).
int select_samples(ModelSetup* ms, int32_t num_samples, float threshold, std::string* err);
// Everything a context derives from (width, height) on the host, for adanerf_create and adanerf_set_frame_size alike: validates the
// size against the shard geometry and batch size of *opt (and the N in force, if there is one yet) and fills info.width / .height /
// .rays_local / .rays_local_max / .batch_rays / .focal and the image half of rg (pixel pitch, start, focal, strips, NDC scales); the
// camera and the view cell in rg stay.  batch_rays comes from opt->batch_rays, the value the caller asked for, never from the clamped
// info.batch_rays.  On failure *ms is unchanged.  Needs ms->cfg.
int frame_geometry(ModelSetup* ms, const adanerf_options* opt, int w, int h, std::string* err);
// The ray-generator half of frame_geometry, pure: the image half of *rg (pixel pitch, start, focal, size, strips, NDC scales) for a
// w x h frame of a model with this field of view; the camera and the view cell in *rg stay.  Returns the focal length as fp32
// (adanerf_info.focal).  adanerf_temporal_upsample builds the generator of its output size with it, from the same expressions.
float ray_geometry(double fov, int w, int h, int strip_rows, int world, int rank, RayGenParams* rg);
// The ray generator with a sub-pixel offset in force (adanerf_set_pixel_offset): start_x + x_pp * (double)dx, start_y + y_pp * (double)dy,
// each a rounded float64 multiply followed by a rounded float64 add (never fused); a component equal to 0 leaves that start value's bits
// untouched.  The kernels' gen_ray keeps computing start + pp * col.
RayGenParams with_pixel_offset(const RayGenParams& g, float dx, float dy);
// world depth of each of the 128 bins: the sampler's cell centres, or (dense) the dense mode's uniform t-values
void depth_table(const ModelSetup& ms, bool dense, float* ztab128);

// slot layout of an encoding pair (kEnc*, params.hpp): any pair but 10-4 (both networks) and 2-2 (sampling network) is packed into
// the catch-all kMaxBands layout and runs on the run-time-shaped kernels
int enc_layout(int fp, int fd, bool sampling);
NetShape shape_of(int fp0, int fd0, int fp1, int fd1, int ray_samples, bool net0_is_sampling = true);
// ADANERF_PREC_* -> element type of the packing; kPrecSplit (adanerf_host_pack_weights only): the split-precision sampling net
constexpr int kPrecSplit = 3;
Elem elem_of(int prec);
// rows of the image owned by `rank` under round-robin strips
int rows_of_rank(int h, int strip_rows, int world, int rank);

}  // namespace adanerf
