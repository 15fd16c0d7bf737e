// See model_setup.hpp.  Also the three entry points of the C ABI that never touch a device.
#include "model_setup.hpp"
#include "contrast_rule.hpp"
#include "density_rule.hpp"

#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>

namespace adanerf {

thread_local std::string g_create_error;

int enc_layout(int fp, int fd, bool sampling) {
  if (fp == 10 && fd == 4) return kEnc10_4;
  if (sampling && fp == 2 && fd == 2) return kEnc2_2;
  return kEncMax;
}
NetShape shape_of(int fp0, int fd0, int fp1, int fd1, int ray_samples, bool net0_is_sampling) {
  NetShape sh{fp0, fd0, fp1, fd1, ray_samples};
  if (enc_layout(fp0, fd0, net0_is_sampling) == kEncMax) sh.lp0 = sh.ld0 = kMaxBands;
  if (enc_layout(fp1, fd1, false) == kEncMax) sh.lp1 = sh.ld1 = kMaxBands;
  return sh;
}

Elem elem_of(int prec) {
  return prec == ADANERF_PREC_BF16 ? Elem::BF16 : (prec == ADANERF_PREC_FP16 ? Elem::F16 : (prec == kPrecSplit ? Elem::F16_SPLIT : Elem::F32));
}

int rows_of_rank(int h, int strip_rows, int world, int rank) {
  int n_strips = (h + strip_rows - 1) / strip_rows;
  int rows = 0;
  for (int s = rank; s < n_strips; s += world) rows += std::min(strip_rows, h - s * strip_rows);
  return rows;
}

static bool contains(const std::string& s, const char* sub) { return s.find(sub) != std::string::npos; }

int setup_model(const char* model_dir, const adanerf_options* opt, ModelSetup* ms, std::string* err) {
  try {
    return setup_model_unguarded(model_dir, opt, ms, err);
  } catch (const std::exception& e) {
    *err = std::string("model directory: ") + e.what();
    return ADANERF_EIO;
  }
}
int setup_model_unguarded(const char* model_dir, const adanerf_options* opt, ModelSetup* ms, std::string* err) {
  auto bad = [&](int code, const std::string& msg) {
    *err = msg;
    return code;
  };
  if (opt->width <= 0 || opt->height <= 0) return bad(ADANERF_EINVAL, "width/height must be positive");
  if (!ms->cfg.load(model_dir, err)) return ADANERF_EIO;
  const Config& cf = ms->cfg;

  // ---- validate the configuration against the supported (north-star) path ----
  const bool coarse_fine = cf.inFeatures.size() == 2 && cf.inFeatures[0] == "RayMarchFromPoses" && cf.inFeatures[1] == "RayMarchFromCoarse";
  ms->coarse_fine = coarse_fine;
  if (!coarse_fine && (cf.inFeatures.size() != 2 || cf.inFeatures[0] != "SpherePosDir" || cf.inFeatures[1] != "RayMarchFromPoses"))
    return bad(ADANERF_EUNSUPPORTED, "inFeatures must be [SpherePosDir, RayMarchFromPoses] or [RayMarchFromPoses, RayMarchFromCoarse]");
  if (cf.posEnc.size() != 2 || cf.posEnc[0] != "nerf" || cf.posEnc[1] != "nerf" || cf.posEncArgs.size() != 2)
    return bad(ADANERF_EUNSUPPORTED, "posEnc must be [nerf, nerf] with two posEncArgs entries");
  const bool pdf_mode = !coarse_fine && cf.rayMarchSampler.size() == 2 && cf.rayMarchSampler[1] == "FromClassifiedDepth";
  if (coarse_fine) {
    // RayMarchFromPoses without an oracle in front draws its depths from rayMarchSampler[0] (src/features.py:431-436)
    if (cf.rayMarchSampler.empty() || cf.rayMarchSampler[0] != "LinearlySpacedZNearZFar")
      return bad(ADANERF_EUNSUPPORTED, "coarse/fine: rayMarchSampler[0] must be LinearlySpacedZNearZFar");
    if (cf.numRaymarchSamples.size() != 2) return bad(ADANERF_EIO, "coarse/fine: numRaymarchSamples must be [Nc, Nf]");
  } else if (cf.rayMarchSampler.size() != 2 || (!pdf_mode && !contains(cf.rayMarchSampler[1], "FromClassifiedDepthAdaptive")))
    return bad(ADANERF_EUNSUPPORTED, "rayMarchSampler[1] must be FromClassifiedDepthAdaptive[NoDepthRange] or FromClassifiedDepth");
  // The transform every sampler applies to the raw oracle outputs follows losses[0] (src/nerf_raymarch_common.py:624-630,
  // 686-690, 782-788).  A model directory without a losses key (the trimmed 19-key config.ini) is an AdaNeRF export
  // (NeRFWeightMultiplicationLoss: no transform) -- except under FromClassifiedDepth, where the viewer's samplePDF
  // (base_cuda_kernels.cu:296-372) and every DONeRF config apply the sigmoid.
  {
    const std::string l0 = cf.losses.empty() ? std::string(pdf_mode ? "BCEWithLogitsLoss" : "NeRFWeightMultiplicationLoss") : cf.losses[0];
    ms->transform = l0 == "BCEWithLogitsLoss" ? kOracleSigmoid : ((l0 == "CrossEntropyLoss" || l0 == "CrossEntropyLossWeighted") ? kOracleSoftmax : kOracleRaw);
  }
  // raySampleInput[0] = A > 0: A extra encoded points along the ray in the oracle net's input (src/features.py:876-888);
  // the shading net takes no such input on this path (RayMarchFromPoses ignores the key)
  ms->ray_samples = cf.raySampleInput.empty() ? 0 : cf.raySampleInput[0];
  if (ms->ray_samples < 0 || ms->ray_samples > 1024) return bad(ADANERF_EUNSUPPORTED, "raySampleInput[0] must be in 0..1024");
  if (cf.viewcellCenter.size() != 3 || cf.viewcellSize.size() != 3 || cf.depthRange.size() != 2 || cf.fov <= 0.0)
    return bad(ADANERF_EIO, "dataset_info.txt: view_cell_center/view_cell_size/depth_range/fov missing or malformed");
  if (cf.numRaymarchSamples.empty()) return bad(ADANERF_EIO, "config.ini: numRaymarchSamples missing");
  ms->fp0 = static_cast<int>(cf.posEncArgs[0][0]);
  ms->fd0 = static_cast<int>(cf.posEncArgs[0][1]);
  ms->fp1 = static_cast<int>(cf.posEncArgs[1][0]);
  ms->fd1 = static_cast<int>(cf.posEncArgs[1][1]);
  // any F_pos-F_dir the reference's "nerf" encoding accepts (src/util/feature_encoding.py:54-73; viewer config.cpp:142-146) up to
  // kMaxBands bands: 10-4 (both nets) and 2-2 (sampling net) run on the specialised kernels, every other pair on the
  // run-time-shaped fp32 kernels with the catch-all slot layout
  for (int f : {ms->fp0, ms->fd0, ms->fp1, ms->fd1})
    if (f < 0 || f > kMaxBands) return bad(ADANERF_EUNSUPPORTED, "posEncArgs: 0.." + std::to_string(kMaxBands) + " frequency bands are supported");
  const bool ndc = cf.useNDC;
  const bool no_range = !coarse_fine && contains(cf.rayMarchSampler[1], "NoDepthRange");
  if (!pdf_mode && !coarse_fine && ndc != no_range) return bad(ADANERF_EUNSUPPORTED, "useNDC requires the NoDepthRange sampler and vice versa");
  // every function nerf_get_normalization_function knows (src/nerf_raymarch_common.py:195-244); a config WITHOUT the key gets
  // normalization_max_depth (src/features.py:319-324)
  auto norm_code = [](const std::string& n) {
    return n == "None" ? kNormNone : n == "InverseSqrtDistCentered" ? kNormInverseSqrtDistCentered : n == "Centered" ? kNormCentered
         : n == "MaxDepth" ? kNormMaxDepth : n == "MaxDepthCentered" ? kNormMaxDepthCentered : n == "LogCentered" ? kNormLogCentered
         : n == "InverseDistCentered" ? kNormInverseDistCentered : -1;
  };
  const size_t norm_idx = 1;
  if (!cf.rayMarchNormalization.empty() && cf.rayMarchNormalization.size() <= norm_idx)
    return bad(ADANERF_EIO, "rayMarchNormalization needs one entry per network");
  const std::string norm = cf.rayMarchNormalization.empty() ? std::string("MaxDepth") : cf.rayMarchNormalization[norm_idx];
  if (norm_code(norm) < 0)
    return bad(ADANERF_EUNSUPPORTED, "rayMarchNormalization[1] = " + norm + ": None, Centered, MaxDepth, MaxDepthCentered, LogCentered, InverseDistCentered or InverseSqrtDistCentered");
  if (!cf.rayMarchNormalizationCenter.empty() && cf.rayMarchNormalizationCenter.size() != 3)
    return bad(ADANERF_EIO, "rayMarchNormalizationCenter must hold three values (or none)");
  if (cf.depthTransform != "log" && cf.depthTransform != "linear")
    return bad(ADANERF_EUNSUPPORTED, "depthTransform must be log or linear");
  if (coarse_fine) {
    const std::string norm0 = cf.rayMarchNormalization.empty() ? std::string("MaxDepth") : cf.rayMarchNormalization[0];
    if (norm_code(norm0) < 0) return bad(ADANERF_EUNSUPPORTED, "rayMarchNormalization[0] = " + norm0 + " is not a normalisation the reference knows");
    ms->normalize0 = norm_code(norm0);
  }
  if (cf.accumulationMult == "alpha") ms->mult_mode = 1;
  else if (cf.accumulationMult == "weights") ms->mult_mode = 2;
  else ms->mult_mode = 0;
  if (coarse_fine) ms->mult_mode = 0;
  if (!pdf_mode && !coarse_fine && !cf.losses.empty()) {
    // losses[0] drives two things on the adaptive path (src/nerf_raymarch_common.py:686-690, src/features.py:503):
    // the transform applied to the oracle outputs before the threshold test (sigmoid / softmax for the BCE / CE losses)
    // and whether the kept oracle values reach compositing at all (only under NeRFWeightMultiplicationLoss).
    if (cf.losses[0] != "NeRFWeightMultiplicationLoss") ms->mult_mode = 0;   // no oracle weights in compositing
  }

  if (coarse_fine) {
    // numRaymarchSamples = [Nc, Nf]; every ray carries Nc + Nf samples through model1 (select_samples)
    ms->n_coarse = cf.numRaymarchSamples[0];
    if (ms->n_coarse < 3 || ms->n_coarse > kMaxCoarse) return bad(ADANERF_EINVAL, "coarse/fine: numRaymarchSamples[0] must be in 3..128");
  }
  // multiDepthFeatures = [D0, D1]: D0 outputs of the sampling network, D1 depth cells of the sampler (cell_size = 1 / D1); the
  // reference needs them equal (it indexes cells by output position).  D < 128 runs on 128-wide rows padded with absent bins
  // (pack.cpp); only the adaptive sampler with a threshold takes it -- dense mode and the inverse-CDF sampler walk all 128 bins.
  ms->bins = cf.multiDepthFeatures.empty() ? kBins : cf.multiDepthFeatures.back();
  if (!cf.multiDepthFeatures.empty() && cf.multiDepthFeatures.front() != cf.multiDepthFeatures.back() && !coarse_fine)
    return bad(ADANERF_EUNSUPPORTED, "multiDepthFeatures entries differ: the sampler's cells are the sampling network's outputs");
  if (ms->bins < 1 || ms->bins > kBins) return bad(ADANERF_EUNSUPPORTED, "multiDepthFeatures must be in 1..128");
  if (opt->precision < 0 || opt->precision > 2) return bad(ADANERF_EINVAL, "precision must be ADANERF_PREC_{BF16,FP16,FP32}");
  if (opt->sampling_mode < 0 || opt->sampling_mode > 3) return bad(ADANERF_EINVAL, "sampling_mode must be ADANERF_SAMPLING_{SPLIT_FP16,FP32,FP16,GUARDED}");
  if (!(opt->guard_eps <= 1.0f)) return bad(ADANERF_EINVAL, "guard_eps must be <= 1 (<= 0 selects the default)");
  if (!(opt->guard_eps_pair <= 2.0f)) return bad(ADANERF_EINVAL, "guard_eps_pair must be <= 2 (<= 0 selects the default)");
  {
    const int ap = opt->guard_audit_period;
    if (ap > 32 || (ap > 0 && (ap & (ap - 1)) != 0)) return bad(ADANERF_EINVAL, "guard_audit_period must be a power of two <= 32 (0: default, < 0: off)");
  }

  // ---- info; everything that follows from (width, height): frame_geometry ----
  adanerf_info& I = ms->info;
  I.abi_version = ADANERF_ABI_VERSION;
  I.compute_units = 0;
  I.n_in0 = (ms->ray_samples * 3 + 3) * (2 * ms->fp0 + 1) + 3 + 6 * ms->fd0;     // src/features.py:738-740
  if (coarse_fine) I.n_in0 = 6 + 6 * (ms->fp0 + ms->fd0);                          // src/features.py:622
  I.n_in1 = 6 + 6 * (ms->fp1 + ms->fd1);
  I.use_ndc = ndc;
  I.sampler_mode = coarse_fine ? ADANERF_SAMPLER_COARSE_FINE : (pdf_mode ? ADANERF_SAMPLER_PDF : ADANERF_SAMPLER_ADAPTIVE);
  I.num_samples_coarse = ms->n_coarse;
  I.precision = opt->precision;
  I.fov = static_cast<float>(cf.fov);
  if (int rc = frame_geometry(ms, opt, opt->width, opt->height, err)) return rc;
  RayGenParams& g = ms->rg;
  g.use_ndc = ndc;
  double r2 = 0;
  for (int i = 0; i < 3; ++i) {
    g.center[i] = cf.viewcellCenter[i];
    I.view_cell_center[i] = cf.viewcellCenter[i];
    I.view_cell_size[i] = cf.viewcellSize[i];
    r2 += (static_cast<double>(cf.viewcellSize[i]) / 2.0) * (static_cast<double>(cf.viewcellSize[i]) / 2.0);
  }
  // radius = ||view_cell_size / 2||_2 (src/features.py:761); the reference squares the float64 norm
  const double rad = std::sqrt(r2);
  g.rad2 = static_cast<float>(rad * rad);
  I.view_cell_radius = static_cast<float>(rad);
  const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::memcpy(g.rot, ident, sizeof(ident));
  for (int i = 0; i < 3; ++i) g.pos[i] = g.center[i];
  I.depth_range[0] = cf.depthRange[0];
  I.depth_range[1] = cf.depthRange[1];
  I.max_depth = cf.max_depth;

  ShadeParams& sp = ms->sp;
  for (int i = 0; i < 3; ++i) sp.center[i] = cf.rayMarchNormalizationCenter.size() == 3 ? cf.rayMarchNormalizationCenter[i] : cf.viewcellCenter[i];
  sp.max_depth = cf.max_depth;
  sp.sqrt_max_depth = static_cast<float>(std::sqrt(static_cast<double>(cf.max_depth)));   // math.sqrt(max_depth)
  sp.log_max_depth_p1 = static_cast<float>(std::log(static_cast<double>(cf.max_depth) + 1.0));      // math.log(max_v + 1)
  sp.normalize = norm_code(norm);
  sp.unit_dir = ndc;
  sp.ztab = nullptr;

  ms->dm.d0 = cf.depthRange[0];
  ms->dm.d1 = cf.depthRange[1];
  ms->dm.log_transform = cf.depthTransform == "log";
  // world depths of the raySampleInput points: to_world(linspace(step/2, 1 - step/2, A)), always through the depth range
  for (int a = 0; a < ms->ray_samples; ++a) {
    const float step2 = static_cast<float>(0.5 / ms->ray_samples), end = static_cast<float>(1.0 - 0.5 / ms->ray_samples);
    // torch.linspace(start, end, A): start + a * (end - start) / (A - 1) in fp32 (symmetric form for the upper half)
    const int A = ms->ray_samples;
    const float inc = A > 1 ? (end - step2) / static_cast<float>(A - 1) : 0.f;
    const float t = (a < A / 2) ? step2 + inc * static_cast<float>(a) : end - inc * static_cast<float>(A - 1 - a);
    const float d0 = cf.depthRange[0], d1 = cf.depthRange[1];
    ms->rsi_z.push_back(ms->dm.log_transform ? powf(static_cast<float>(static_cast<double>(d1) - d0 + 1.0), t) - 1.0f + d0 : t * (d1 - d0) + d0);
  }
  const float d0 = cf.depthRange[0], d1 = cf.depthRange[1];
  // coarse/fine: LinearlySpacedZNearZFar.generate (src/nerf_raymarch_common.py:310-325): t = linspace(0,1,Nc+1)[:-1] + 0.5/Nc,
  // near (1-t) + far t with zNear[0] / zFar[0], then depth_transform.to_world over the depth range
  for (int k = 0; k < ms->n_coarse; ++k) {
    const int A = ms->n_coarse + 1;
    const float inc = 1.0f / static_cast<float>(A - 1);
    const float lin = (k < A / 2) ? inc * static_cast<float>(k) : 1.0f - inc * static_cast<float>(A - 1 - k);      // torch.linspace, fp32
    const float t = lin + static_cast<float>(0.5 / ms->n_coarse);
    const float zn = cf.zNear.empty() ? 0.001f : cf.zNear.front(), zf = cf.zFar.empty() ? 1.0f : cf.zFar.front();
    const float zw = zn * (1.0f - t) + zf * t;
    ms->ztab_coarse.push_back(cf.depthTransform == "log" ? powf(static_cast<float>(static_cast<double>(d1) - d0 + 1.0), zw) - 1.0f + d0
                                                         : zw * (d1 - d0) + d0);
  }
  // what bounds the sample positions of a bf16 shading net apart from the depth table in force (select_samples adds that and checks)
  {
    double cmax = 0.0, off = 0.0;
    for (int i = 0; i < 3; ++i) {
      cmax = std::max<double>(cmax, std::fabs(cf.viewcellCenter[i]));
      off = std::max<double>(off, std::fabs(static_cast<double>(sp.center[i]) - cf.viewcellCenter[i]));
    }
    ModelSetup::PosBound& pb = ms->pos_bound;
    pb.active = opt->precision == ADANERF_PREC_BF16 && !ndc;
    pb.normalize = sp.normalize;
    pb.cmax = cmax;
    pb.off = off;
    pb.M = std::max<double>(cf.max_depth, 1e-30);
    pb.rad = rad;
    for (int i = 0; i < 3; ++i) pb.center[i] = cf.viewcellCenter[i];
  }
  // ---- everything that follows from (N, threshold) ----
  ms->sel_n = cf.numRaymarchSamples.back();
  ms->sel_thr = cf.adaptiveSamplingThreshold;
  return select_samples(ms, opt->num_samples, opt->threshold, err);
}

int frame_geometry(ModelSetup* ms, const adanerf_options* opt, int w, int h, std::string* err) {
  auto bad = [&](int code, const std::string& msg) {
    *err = msg;
    return code;
  };
  if (w <= 0 || h <= 0) return bad(ADANERF_EINVAL, "width/height must be positive");
  const int world = opt->shard_world > 0 ? opt->shard_world : 1;
  const int rank = opt->shard_rank;
  if (rank < 0 || rank >= world) return bad(ADANERF_EINVAL, "shard_rank out of range");
  const int strip_rows = opt->strip_rows > 0 ? opt->strip_rows : 8;
  if (static_cast<int64_t>(w) * h >= (1ll << 25)) return bad(ADANERF_EINVAL, "width*height must be < 2^25");
  const int R = rows_of_rank(h, strip_rows, world, rank) * w;
  const int batch = (opt->batch_rays <= 0) ? std::max(R, 1) : std::min(opt->batch_rays, std::max(R, 1));
  // sample offsets, keys and totals are int32 on the device (select_samples checks the same product for a new N; 0: no N yet)
  if (static_cast<int64_t>(batch) * ms->info.num_samples > 0x7fffffffll)
    return bad(ADANERF_EINVAL, "batch_rays * num_samples exceeds 2^31 - 1; use a smaller batch (-bs)");
  // nothing above has touched *ms: a refused size leaves it as it was
  adanerf_info& I = ms->info;
  I.width = w;
  I.height = h;
  I.rays_local = R;
  I.rays_local_max = rows_of_rank(h, strip_rows, world, 0) * w;
  I.batch_rays = batch;
  I.focal = ray_geometry(ms->cfg.fov, w, h, strip_rows, world, rank, &ms->rg);
  return ADANERF_OK;
}

float ray_geometry(double fov, int w, int h, int strip_rows, int world, int rank, RayGenParams* rg) {
  // ray generation constants (A1: src/util/raygeneration.py:10-26, float64)
  const double focal = 0.5 * w / std::tan(0.5 * fov);   // src/datasets.py:182
  const double x_dist = std::tan(fov / 2) * focal;
  const double y_dist = x_dist * (static_cast<double>(h) / w);
  const double x_pp = x_dist / (w / 2.0), y_pp = y_dist / (h / 2.0);
  RayGenParams& g = *rg;
  g.start_x = -(x_dist - x_pp / 2);
  g.x_pp = x_pp;
  g.start_y = -(y_dist - y_pp / 2);
  g.y_pp = y_pp;
  g.focal = focal;
  g.w = w;
  g.h = h;
  g.strip_rows = strip_rows;
  g.world = world;
  g.rank = rank;
  g.ndc_sw = static_cast<float>(-1.0 / (w / (2.0 * focal)));
  g.ndc_sh = static_cast<float>(-1.0 / (h / (2.0 * focal)));
  return static_cast<float>(focal);
}

RayGenParams with_pixel_offset(const RayGenParams& g, float dx, float dy) {
  RayGenParams out = g;
  // the product goes through a volatile: two rounded operations on every compiler setting, never one fused multiply-add
  if (dx != 0.f) {
    volatile double m = g.x_pp * static_cast<double>(dx);
    out.start_x = g.start_x + m;
  }
  if (dy != 0.f) {
    volatile double m = g.y_pp * static_cast<double>(dy);
    out.start_y = g.start_y + m;
  }
  return out;
}

void depth_table(const ModelSetup& ms, bool dense, float* ztab128) {
  const Config& cf = ms.cfg;
  const float znear = cf.zNear.empty() ? 0.001f : cf.zNear.back();
  const float zfar = cf.zFar.empty() ? 1.0f : cf.zFar.back();
  const float d0 = cf.depthRange[0], d1 = cf.depthRange[1];
  for (int k = 0; k < kBins; ++k) {
    float t;
    if (dense) {
      // src/nerf_raymarch_common.py:708-720: t = linspace(0,1,N+1)[:-1] + .5/N; z = near(1-t) + far t
      float u = static_cast<float>(k) * (1.0f / kBins) + 0.5f / kBins;
      t = znear * (1.0f - u) + zfar * u;
    } else {
      t = (static_cast<float>(k) + 0.5f) * (1.0f / static_cast<float>(ms.bins));   // (k + .5) * cell_size, cell_size = 1 / multiDepthFeatures, :726-741
    }
    float z;
    if (ms.info.use_ndc) z = t;                                // ...NoDepthRange: :796-851
    else if (cf.depthTransform == "log")                       // util/depth_transformations.py:37-48
      z = powf(static_cast<float>(static_cast<double>(d1) - d0 + 1.0), t) - 1.0f + d0;
    else z = t * (d1 - d0) + d0;                               // :57-58
    ztab128[k] = z;
  }
}

int select_samples(ModelSetup* ms, int32_t num_samples, float threshold, std::string* err) {
  auto bad = [&](int code, const std::string& msg) {
    *err = msg;
    return code;
  };
  const Config& cf = ms->cfg;
  adanerf_info& I = ms->info;
  const bool coarse_fine = ms->coarse_fine, pdf_mode = I.sampler_mode == ADANERF_SAMPLER_PDF;
  const int n_req = num_samples > 0 ? num_samples : ms->sel_n;
  const float thr_req = threshold >= 0.f ? threshold : ms->sel_thr;
  int n_max = n_req;
  float thr = thr_req;
  if (pdf_mode || coarse_fine) thr = 1.0f;   // unused by the inverse-CDF samplers; any positive value keeps the bin-centre depth table
  if (coarse_fine) {
    // numRaymarchSamples = [Nc, Nf] (num_samples overrides Nf); every ray carries Nc + Nf samples through model1
    if (n_max < 1 || ms->n_coarse + n_max > 1024) return bad(ADANERF_EINVAL, "coarse/fine: numRaymarchSamples[1] must be >= 1 and Nc + Nf <= 1024");
    n_max += ms->n_coarse;
  }
  if (thr < 0.f) return bad(ADANERF_EUNSUPPORTED, "adaptiveSamplingThreshold < 0 is unsupported on the adaptive path (as in the reference)");
  if (ms->bins != kBins && (pdf_mode || coarse_fine || thr == 0.f))
    return bad(ADANERF_EUNSUPPORTED, "multiDepthFeatures != 128 is supported with the adaptive sampler and a threshold > 0 only");
  if (ms->bins != kBins && n_max > ms->bins) return bad(ADANERF_EINVAL, "numRaymarchSamples exceeds multiDepthFeatures");
  if (thr == 0.f && n_max != kBins) return bad(ADANERF_EUNSUPPORTED, "adaptiveSamplingThreshold == 0 (dense) requires numRaymarchSamples == 128");
  if (!coarse_fine && (n_max < 1 || n_max > kBins)) return bad(ADANERF_EINVAL, "numRaymarchSamples must be in 1..128");
  // sample offsets, keys and totals are int32 on the device
  if (static_cast<int64_t>(I.batch_rays) * n_max > 0x7fffffffll)
    return bad(ADANERF_EINVAL, "batch_rays * num_samples exceeds 2^31 - 1; use a smaller batch (-bs)");
  // ---- depth table: world depth of each of the 128 bins (A4/A5) ----
  std::vector<float> ztab(kBins);
  depth_table(*ms, thr == 0.f, ztab.data());
  // bf16 shading nets are packed scaled (pack.cpp scale_layer): every ReLU layer carries a power of two that keeps its activations <= 1 for
  // encoding inputs whose identity slots stay below kPosIdentityBound (positions) -- a scene whose sample positions can exceed it is refused here
  // rather than clamped silently.  Positions: camera inside the view cell, samples up to the far end of the depth range along a unit ray.
  ModelSetup::PosBound pb = ms->pos_bound;
  if (I.precision == ADANERF_PREC_BF16) {
    double zmax = std::max<double>(std::fabs(cf.depthRange[1]), std::fabs(cf.max_depth));
    for (float z : ztab) zmax = std::max<double>(zmax, std::fabs(z));
    for (float z : ms->ztab_coarse) zmax = std::max<double>(zmax, std::fabs(z));
    pb.zmax = zmax;
    double bound = pb.at(0.5 * pb.rad);      // a camera inside the view cell
    if (I.use_ndc) bound = 64.0;      // NDC cube [-1, 1]^3 for rays inside the frustum (positions o' + t d', t in [0, 1])
    if (!(bound <= kPosIdentityBound)) {
      char msg[256];
      std::snprintf(msg, sizeof(msg), "sample positions of this scene can reach %.3g after rayMarchNormalization: beyond the %.0f the bf16 shading path's "
                    "layer scaling assumes (pack.hpp kPosIdentityBound) -- use precision fp16 or fp32", bound, kPosIdentityBound);
      return bad(ADANERF_EUNSUPPORTED, msg);
    }
  }
  // nothing above has touched *ms: a refused pair leaves it as it was
  ms->sel_n = n_req;
  ms->sel_thr = thr_req;
  ms->pos_bound = pb;
  ms->ztab = std::move(ztab);
  I.num_samples = n_max;
  I.threshold = thr;
  I.dense = thr == 0.f;
  return ADANERF_OK;
}

}  // namespace adanerf

using namespace adanerf;

namespace {

constexpr int kPrecBf16Unscaled = 4;      // adanerf_host_pack_weights only: see there

int fail(int code, const std::string& msg) {
  g_create_error = msg;
  return code;
}

}  // namespace

extern "C" {

int adanerf_host_parse_model(const char* model_dir, const adanerf_options* opt, adanerf_info* info) {
  if (!model_dir || !opt || !info) return fail(ADANERF_EINVAL, "NULL argument");
  ModelSetup ms;
  std::string err;
  int rc = setup_model(model_dir, opt, &ms, &err);
  if (rc) return fail(rc, err);
  *info = ms.info;
  return ADANERF_OK;
}

int adanerf_host_subpixel_grid(int32_t s, int32_t k, float* dx, float* dy) {
  if (s < 1 || s > 8 || k < 0 || k >= s * s || !dx || !dy) return fail(ADANERF_EINVAL, "adanerf_host_subpixel_grid: s must be in 1..8, k in 0..s*s-1, outputs non-NULL");
  const int i = k % s, j = k / s;
  *dx = static_cast<float>((2.0 * i + 1.0 - s) / (2.0 * s));
  *dy = static_cast<float>((2.0 * j + 1.0 - s) / (2.0 * s));
  return ADANERF_OK;
}

int adanerf_host_sphere_zc(int32_t width, int32_t height, float focal, const float pos[3], const float rot_c2w[9], const float center[3], float radius,
                           float* zc_out) {
  if (!pos || !rot_c2w || !center || !zc_out) return fail(ADANERF_EINVAL, "adanerf_host_sphere_zc: NULL argument");
  if (width < 1 || width > 16384 || height < 1 || height > 16384) return fail(ADANERF_EINVAL, "adanerf_host_sphere_zc: width and height must be in 1..16384");
  bool finite = std::isfinite(focal) && std::isfinite(radius);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(pos[i]) && std::isfinite(center[i]);
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(rot_c2w[i]);
  if (!finite) return fail(ADANERF_EINVAL, "adanerf_host_sphere_zc: every value must be finite");
  if (!(radius > 0.f) || !(focal > 0.f)) return fail(ADANERF_EINVAL, "adanerf_host_sphere_zc: radius and focal must be > 0");
  // every intermediate goes through a volatile: one rounded float64 operation per step on every compiler setting, never a fused
  // multiply-add (with_pixel_offset); the order is the one the header states
  volatile double e[3], c[3], m0, m1, m2, s;
  for (int i = 0; i < 3; ++i) e[i] = static_cast<double>(center[i]) - static_cast<double>(pos[i]);
  for (int k = 0; k < 3; ++k) {      // c = R^T e
    m0 = static_cast<double>(rot_c2w[k]) * e[0];
    m1 = static_cast<double>(rot_c2w[3 + k]) * e[1];
    m2 = static_cast<double>(rot_c2w[6 + k]) * e[2];
    s = m0 + m1;
    c[k] = s + m2;
  }
  m0 = c[0] * c[0];
  m1 = c[1] * c[1];
  m2 = c[2] * c[2];
  s = m0 + m1;
  volatile double cc = s + m2;
  volatile double rr = static_cast<double>(radius) * static_cast<double>(radius);
  volatile double g = cc - rr;
  const double f = static_cast<double>(focal), hw = 0.5 * width, hh = 0.5 * height;
  const float inf = std::numeric_limits<float>::infinity();
  for (int y = 0; y < height; ++y) {
    volatile double ny = (y + 0.5) - hh;
    volatile double py = ny / f;
    const double vy = -py;
    for (int x = 0; x < width; ++x) {
      volatile double nx = (x + 0.5) - hw;
      volatile double vx = nx / f;
      m0 = vx * vx;
      m1 = vy * vy;
      s = m0 + m1;
      volatile double a = s + 1.0;
      m0 = vx * c[0];
      m1 = vy * c[1];
      s = m0 + m1;
      volatile double b = s - c[2];
      m0 = b * b;
      m1 = a * g;
      volatile double disc = m0 - m1;
      float out = inf;
      if (disc >= 0.0) {
        volatile double q = std::sqrt(disc);
        volatile double n0 = b - q, n1 = b + q;
        volatile double t0 = n0 / a, t1 = n1 / a;
        if (t0 > 0.0) out = static_cast<float>(t0);
        else if (t1 > 0.0) out = static_cast<float>(t1);
      }
      zc_out[static_cast<size_t>(y) * width + x] = out;
    }
  }
  return ADANERF_OK;
}

// adanerf_host_density_mask is phase (0, 0) of adanerf_host_density_mask_phased
static int host_density_mask_at(const std::string& who, int32_t width, int32_t height, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px,
                                const int32_t* stride, int32_t phase_x, int32_t phase_y, uint8_t* mask_out) {
  if (!mask_out) return fail(ADANERF_EINVAL, who + ": NULL mask");
  if (width < 1 || width > 16384 || height < 1 || height > 16384) return fail(ADANERF_EINVAL, who + ": width and height must be in 1..16384");
  DensityRule f;
  if (const char* why = density_rule_fill(gaze_x, gaze_y, n_rings, radius_px, stride, &f, phase_x, phase_y)) return fail(ADANERF_EINVAL, who + ": " + why);
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) mask_out[static_cast<size_t>(y) * width + x] = density_mask_byte(f, x, y, width, height);
  return ADANERF_OK;
}

int adanerf_host_density_mask(int32_t width, int32_t height, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride,
                              uint8_t* mask_out) {
  return host_density_mask_at("adanerf_host_density_mask", width, height, gaze_x, gaze_y, n_rings, radius_px, stride, 0, 0, mask_out);
}

int adanerf_host_density_mask_phased(int32_t width, int32_t height, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride,
                                     int32_t phase_x, int32_t phase_y, uint8_t* mask_out) {
  return host_density_mask_at("adanerf_host_density_mask_phased", width, height, gaze_x, gaze_y, n_rings, radius_px, stride, phase_x, phase_y, mask_out);
}

int adanerf_host_density_phase(int32_t k, int32_t* phase_x, int32_t* phase_y) {
  if (!phase_x || !phase_y) return fail(ADANERF_EINVAL, "adanerf_host_density_phase: NULL output");
  density_phase(k, phase_x, phase_y);
  return ADANERF_OK;
}

int adanerf_host_contrast_mask(const float* rgb, int32_t width, int32_t height, float threshold, uint8_t* mask, int32_t* n_flagged) {
  if (!rgb || !mask) return fail(ADANERF_EINVAL, "adanerf_host_contrast_mask: NULL image or mask");
  if (const char* why = contrast_rule_check(width, height, threshold)) return fail(ADANERF_EINVAL, std::string("adanerf_host_contrast_mask: ") + why);
  if (reinterpret_cast<uintptr_t>(rgb) & 3) return fail(ADANERF_EINVAL, "adanerf_host_contrast_mask: rgb must be 4-byte aligned");
  const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(rgb), b0 = reinterpret_cast<uintptr_t>(mask);
  if (a0 < b0 + n && b0 < a0 + n * 3 * sizeof(float)) return fail(ADANERF_EINVAL, "adanerf_host_contrast_mask: the mask overlaps the image");
  const auto plane = [&](int ch) {
    return [=](int x, int y) { return contrast_display(rgb[(static_cast<size_t>(y) * width + x) * 3 + ch]); };
  };
  int32_t count = 0;
  for (int y = 0; y < height; ++y)
    for (int x = 0; x < width; ++x) {
      const uint8_t m = contrast_mask_byte(x, y, width, height, threshold, plane(0), plane(1), plane(2));
      mask[static_cast<size_t>(y) * width + x] = m;
      count += m == 0;
    }
  if (n_flagged) *n_flagged = count;
  return ADANERF_OK;
}

int adanerf_host_pair_weight(const float dst_pos[3], const float a_pos[3], const float b_pos[3], float* weight_b) {
  if (!dst_pos || !a_pos || !b_pos || !weight_b) return fail(ADANERF_EINVAL, "adanerf_host_pair_weight: NULL argument");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(dst_pos[i]) || !std::isfinite(a_pos[i]) || !std::isfinite(b_pos[i])) return fail(ADANERF_EINVAL, "adanerf_host_pair_weight: every value must be finite");
  // every intermediate goes through a volatile, as in adanerf_host_sphere_zc: one rounded float64 operation per step, never fused
  volatile double d[2];
  for (int s = 0; s < 2; ++s) {
    const float* from = s ? b_pos : a_pos;
    volatile double e0 = static_cast<double>(dst_pos[0]) - static_cast<double>(from[0]);
    volatile double e1 = static_cast<double>(dst_pos[1]) - static_cast<double>(from[1]);
    volatile double e2 = static_cast<double>(dst_pos[2]) - static_cast<double>(from[2]);
    volatile double m0 = e0 * e0, m1 = e1 * e1, m2 = e2 * e2;
    volatile double sum = m0 + m1;
    volatile double sq = sum + m2;
    d[s] = std::sqrt(sq);
  }
  volatile double both = d[0] + d[1];
  *weight_b = both == 0.0 ? 0.5f : static_cast<float>(d[0] / both);
  return ADANERF_OK;
}

int adanerf_host_depth_table(const char* model_dir, const adanerf_options* opt, float* ztab128) {
  if (!model_dir || !opt || !ztab128) return fail(ADANERF_EINVAL, "NULL argument");
  ModelSetup ms;
  std::string err;
  int rc = setup_model(model_dir, opt, &ms, &err);
  if (rc) return fail(rc, err);
  std::memcpy(ztab128, ms.ztab.data(), kBins * sizeof(float));
  return ADANERF_OK;
}

int adanerf_host_pack_weights(const char* model_dir, int32_t net, int32_t precision, void* weights_out, size_t* weights_bytes,
                              float* bias_out, size_t* bias_floats, int32_t* layer_out, int32_t* n_layers) try {
  if (!model_dir || !weights_bytes || !bias_floats || !n_layers) return fail(ADANERF_EINVAL, "NULL argument");
  // kPrecBf16Unscaled (shading nets only): bf16 WITHOUT the scaled packing -- for the CPU test that replays both blobs; no kernel consumes it
  const bool unscaled_bf16 = precision == kPrecBf16Unscaled && net == 1;
  if (unscaled_bf16) precision = ADANERF_PREC_BF16;
  if (net < 0 || net > 1 || precision < 0 || precision > kPrecSplit || (precision == kPrecSplit && net != 0))
    return fail(ADANERF_EINVAL, "net/precision out of range");
  Config cfg;
  std::string err;
  if (!cfg.load(model_dir, &err)) return fail(ADANERF_EIO, err);
  if (cfg.posEncArgs.size() != 2) return fail(ADANERF_EIO, "posEncArgs missing");
  const bool cfm = cfg.inFeatures.size() == 2 && cfg.inFeatures[0] == "RayMarchFromPoses" && cfg.inFeatures[1] == "RayMarchFromCoarse";
  const NetShape sh = shape_of(static_cast<int>(cfg.posEncArgs[0][0]), static_cast<int>(cfg.posEncArgs[0][1]), static_cast<int>(cfg.posEncArgs[1][0]),
                               static_cast<int>(cfg.posEncArgs[1][1]), cfg.raySampleInput.empty() ? 0 : cfg.raySampleInput[0], !cfm);
  TensorMap tm;
  if (!read_onnx_initializers(join_path(model_dir, net == 0 ? "model0.onnx" : "model1.onnx"), &tm, &err)) return fail(ADANERF_EIO, err);
  PackedNet pn;
  // a coarse/fine directory holds two NeRF nets: model0.onnx packs like a shading net with the encoding posEncArgs[0]
  bool ok;
  if (net == 0 && cfm) {
    if (precision == kPrecSplit) return fail(ADANERF_EINVAL, "coarse/fine model: net 0 is a NeRF net (precision 0..2)");
    const NetShape shc = shape_of(sh.fp0, sh.fd0, sh.fp0, sh.fd0, 0, false);
    ok = pack_shading_net(tm, shc, elem_of(precision), &pn, &err);
  } else {
    ok = net == 0 ? pack_sampling_net(tm, sh, elem_of(precision), &pn, &err) : pack_shading_net(tm, sh, elem_of(precision), &pn, &err, !unscaled_bf16);
  }
  if (!ok) return fail(ADANERF_EIO, err);
  if (weights_out) {
    if (*weights_bytes < pn.weights.size()) return fail(ADANERF_EINVAL, "weights_out too small");
    std::memcpy(weights_out, pn.weights.data(), pn.weights.size());
  }
  if (bias_out) {
    if (*bias_floats < pn.bias.size()) return fail(ADANERF_EINVAL, "bias_out too small");
    std::memcpy(bias_out, pn.bias.data(), pn.bias.size() * sizeof(float));
  }
  const bool rsi = net == 0 && pn.topo.ray_samples > 0;     // one more record: the raySampleInput block of layer 0
  const bool scaled = pn.relu_scaled;                        // one more record: the output exponents of a scaled (bf16) shading net
  const int32_t n_rec = static_cast<int32_t>(pn.w_off.size()) + (rsi ? 1 : 0) + (scaled ? 1 : 0);
  if (layer_out) {
    if (*n_layers < n_rec) return fail(ADANERF_EINVAL, "layer_out too small");
    for (size_t i = 0; i < pn.w_off.size(); ++i) {
      layer_out[4 * i + 0] = static_cast<int32_t>(pn.w_off[i]);
      layer_out[4 * i + 1] = static_cast<int32_t>(pn.b_off[i]);
      layer_out[4 * i + 2] = pn.slots[i];
      layer_out[4 * i + 3] = pn.mtiles[i];
    }
    if (rsi) {
      const size_t i = pn.w_off.size();
      layer_out[4 * i + 0] = static_cast<int32_t>(pn.rsi_w_off);
      layer_out[4 * i + 1] = pn.topo.ray_samples;
      layer_out[4 * i + 2] = pe_slots(sh.lp0 ? sh.lp0 : sh.fp0);
      layer_out[4 * i + 3] = pn.mtiles[0];
    }
    if (scaled) {      // {alpha exponent, rgb exponent, 0, -1}: outputs of the packed network x 2^exponent = the network's own
      const size_t i = pn.w_off.size();
      layer_out[4 * i + 0] = pn.out_exp[0];
      layer_out[4 * i + 1] = pn.out_exp[1];
      layer_out[4 * i + 2] = 0;
      layer_out[4 * i + 3] = -1;
    }
  }
  *weights_bytes = pn.weights.size();
  *bias_floats = pn.bias.size();
  *n_layers = n_rec;
  return ADANERF_OK;
} catch (const std::exception& e) {
  return fail(ADANERF_EIO, std::string("adanerf_host_pack_weights: ") + e.what());
}

}  // extern "C"
