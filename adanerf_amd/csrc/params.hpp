// Plain structs, enums and constants the host fills and the kernels read.  Host-safe: no HIP header, no vector types, so the
// pure-host translation units (model_setup.cpp, guard_record.cpp, flip_tables.cpp) share them with the kernel headers.
#pragma once
#include <stdint.h>

namespace adanerf {

// Everything ray generation needs (A1 + A2).  Doubles mirror the float64 numpy ray table of
// src/util/raygeneration.py:10-26.
struct RayGenParams {
  double start_x, x_pp, start_y, y_pp, focal;
  int32_t w, h;
  int32_t strip_rows, world, rank;     // round-robin strip sharding of image rows
  int32_t use_ndc;
  float rot[9];                        // row-major c2w
  float pos[3];
  float center[3];
  float rad2;                          // ||view_cell_size/2||^2
  float ndc_sw, ndc_sh;                // -1/(W/(2 focal)), -1/(H/(2 focal))
};

// rayMarchNormalization (src/nerf_raymarch_common.py:195-244)
enum { kNormNone = 0, kNormInverseSqrtDistCentered = 1, kNormCentered = 2, kNormMaxDepth = 3, kNormMaxDepthCentered = 4, kNormLogCentered = 5,
       kNormInverseDistCentered = 6 };

struct ShadeParams {
  float center[3];                     // view_cell_center, or rayMarchNormalizationCenter when the config sets three values
  float max_depth;
  float sqrt_max_depth;
  int32_t normalize;                   // kNorm*
  int32_t unit_dir;                    // 1: PE(dir/|dir|) (NDC), 0: PE(dir) as received
  float log_max_depth_p1;              // math.log(max_depth + 1): kNormLogCentered
  const float* ztab;                   // [128] world depth per bin
};

struct DepthMap {          // warped depth t in [0,1] -> world depth (src/util/depth_transformations.py:37-58)
  float d0, d1;
  int32_t log_transform;   // 1: (d1-d0+1)^t - 1 + d0, 0: t (d1-d0) + d0
};

// the sampler's transform of the raw oracle outputs (SelectOut::transform, k_select_pair.hip.hpp); src/nerf_raymarch_common.py:624-630 /
// 686-690: BCEWithLogitsLoss -> sigmoid, CrossEntropyLoss[Weighted] -> softmax over the bins
constexpr int kOracleRaw = 0, kOracleSigmoid = 1, kOracleSoftmax = 2;

constexpr int kMaxCoarse = 128;      // coarse samples per ray (their depths are a table, like the 128 bins)

// slot layout of the positional encodings a network was packed with: the specialised kernels exist for 10-4 (both networks) and
// 2-2 (sampling network); kEncMax is the catch-all kMaxBands-band layout of the run-time-shaped kernels (any posEncArgs)
enum { kEnc10_4 = 0, kEnc2_2 = 1, kEncMax = 2 };

struct GenericTopo {      // a network on the run-time-shaped kernels (k_generic_f32.hip.hpp, k_generic16.hip.hpp)
  int32_t depth;        // Linear layers of the trunk (sampling net: all layers)
  int32_t cat_mask;     // shading trunk: bit l set <=> layer l takes cat([pts, h]) (l - 1 in the reference's `skips`, src/models.py:226-228, 260-261); 0 none
  int32_t ray_samples;  // sampling net: raySampleInput
  uint32_t rsi_w_off;   // 16-byte offset of the raySampleInput fragments of layer 0, [a][s4][m][lane]
  const float* rsi_z;   // [ray_samples] world depth of every extra point
  float rsi_d1;         // upper end of the warped depth range
};

constexpr int kFlipMaxRadius = 19;     // colour radius at 140 pixels per degree: (32 + 38)^2 x 6 planes x 4 B = 117.6 KB of the CU's 160 KB

struct FlipParams {
  const float* test;     // [h*w,3] sRGB
  const float* ref;      // [h*w,3] sRGB
  float* map;            // [h*w] or null
  double* partial;       // [tiles] one sum per workgroup
  const float* tab;      // A, RG, BY [(2 rc + 1)^2] each, then edge, point [(2 rf + 1)^2] each (x direction; y is the transpose)
  int32_t width, height, tiles_x;
  int32_t rc, rf, halo;  // filter radii of the colour / feature pipeline; halo = max of the two
  float rgb2xyz[9];      // flip_loss.py:264-272, fp32 as torch.Tensor holds it
  float xyz2rgb[9];      // its inverse
  float illum[3];        // A (1,1,1)
  float lab_div, lab_add;          // 3 (6/29)^2, 4/29
  float pccmax, lo_scale, hi_div;  // redistribute_errors: pc cmax, pt / (pc cmax), cmax - pc cmax
  float pt, one_minus_pt;
  float inv_sqrt2;
};

}  // namespace adanerf
