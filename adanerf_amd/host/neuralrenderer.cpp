#include "neuralrenderer.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

NeuralRenderer::~NeuralRenderer() {
  for (size_t i = 0; i < d_fovea_n.size(); ++i) {
    adanerf_ctx* c = i == 0 ? ctx : (i - 1 < peers.size() ? peers[i - 1] : nullptr);
    if (!c) continue;
    if (d_fovea_n[i]) adanerf_free(c, d_fovea_n[i]);
    if (d_fovea_thr[i]) adanerf_free(c, d_fovea_thr[i]);
  }
  for (size_t i = 0; i < peers.size(); ++i) {
    if (peers[i]) {
      if (i + 1 < d_payload.size() && d_payload[i + 1]) adanerf_free(peers[i], d_payload[i + 1]);
      adanerf_destroy(peers[i]);
    }
  }
  if (ctx) {
    if (d_gathered) adanerf_free(ctx, d_gathered);
    for (const FrameBuffer& b : frameBuffers())
      if (*b.p) adanerf_free(ctx, *b.p);
    if (d_window) adanerf_free(ctx, d_window);
    adanerf_destroy(ctx);
  }
}

int NeuralRenderer::batchesPerFrame() const {
  const long long rays = static_cast<long long>(info_.width) * info_.height, b = info_.batch_rays > 0 ? info_.batch_rays : rays;
  return static_cast<int>((rays + b - 1) / (b > 0 ? b : 1));
}

static adanerf_options options_of(const Settings& settings) {
  adanerf_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.width = static_cast<int32_t>(settings.width);
  opt.height = static_cast<int32_t>(settings.height);
  opt.batch_rays = settings.batch_request;      // the library clamps it to the frame (Settings::batch_size), again at every size
  opt.num_samples = settings.num_samples;
  opt.threshold = settings.threshold;
  opt.sampling_mode = (settings.sampling == "split" || settings.sampling == "auto") ? ADANERF_SAMPLING_SPLIT_FP16 : (settings.sampling == "fp32" ? ADANERF_SAMPLING_FP32
                      : (settings.sampling == "fp16" ? ADANERF_SAMPLING_FP16 : ADANERF_SAMPLING_GUARDED));
  opt.shard_world = 1;
  return opt;
}

bool NeuralRenderer::initHostOnly() {
  const adanerf_options opt = options_of(settings);
  if (adanerf_host_parse_model(settings.model_path.c_str(), &opt, &info_) != ADANERF_OK) {
    err = adanerf_last_error(nullptr);
    return false;
  }
  camera.setPosition(info_.view_cell_center);
  camera.setViewCell(info_.view_cell_size);
  render_oracle = settings.render_oracle;
  return true;
}

// --sampling auto: the default rule measured on the workload at hand -- a few frames of this model / frame size / threshold in the
// split mode (exact by construction) and in the guarded mode (the same frames while its measured band holds), camera at the view-cell centre;
// guarded only if it is at least 8 % faster here.  One context at a time, on GPU 0.
static std::string measure_sampling_mode(const adanerf_options& base, const Settings& settings, const Camera& camera) {
  double fps[2] = {0.0, 0.0};
  const int modes[2] = {ADANERF_SAMPLING_SPLIT_FP16, ADANERF_SAMPLING_GUARDED};
  for (int k = 0; k < 2; ++k) {
    adanerf_options opt = base;
    opt.sampling_mode = modes[k];
    adanerf_ctx* c = nullptr;
    if (adanerf_create(settings.model_path.c_str(), &opt, &c) != ADANERF_OK) break;      // no guarded mode for this model: split
    adanerf_info info;
    void* frame = nullptr;
    float rot[9];
    camera.getRotMatrix(rot);
    bool ok = adanerf_get_info(c, &info) == ADANERF_OK && adanerf_malloc(c, static_cast<size_t>(info.rays_local_max) * 4, &frame) == ADANERF_OK &&
              adanerf_set_camera(c, info.view_cell_center, rot) == ADANERF_OK;
    const int warm = 2, frames = 6;
    for (int i = 0; ok && i < warm; ++i) ok = adanerf_render(c, frame, nullptr, nullptr) == ADANERF_OK;
    ok = ok && adanerf_sync(c) == ADANERF_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; ok && i < frames; ++i) ok = adanerf_render(c, frame, nullptr, nullptr) == ADANERF_OK;
    ok = ok && adanerf_sync(c) == ADANERF_OK;
    if (ok) fps[k] = frames / std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (frame) adanerf_free(c, frame);
    adanerf_destroy(c);
    if (!ok) break;
  }
  const bool guarded = fps[0] > 0.0 && fps[1] >= 1.08 * fps[0];
  std::cout << "--sampling auto: split " << fps[0] << " frames/s, guarded " << fps[1] << " frames/s -> " << (guarded ? "guarded" : "split")
            << " (guarded only if >= 8 % faster on this workload)" << std::endl;
  return guarded ? "guarded" : "split";
}

bool NeuralRenderer::init() {
  std::cout << "Model Path: " << settings.model_path << std::endl;
  adanerf_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.width = static_cast<int32_t>(settings.width);
  opt.height = static_cast<int32_t>(settings.height);
  opt.batch_rays = settings.batch_request;      // the library clamps it to the frame (Settings::batch_size), again at every size
  opt.device_id = 0;
  opt.precision = settings.precision == "fp32" ? ADANERF_PREC_FP32 : (settings.precision == "fp16" ? ADANERF_PREC_FP16 : ADANERF_PREC_BF16);
  opt.num_samples = settings.num_samples;
  opt.threshold = settings.threshold;
  opt.shard_world = 1;
  opt.strip_rows = 8;
  opt.flags |= ADANERF_FLAG_GUARD_AUDIT_FILL;
  if (settings.sampling == "auto") settings.sampling = settings.precision == "fp32" ? std::string("split") : measure_sampling_mode(opt, settings, camera);
  opt.sampling_mode = settings.sampling == "split" ? ADANERF_SAMPLING_SPLIT_FP16 : (settings.sampling == "fp32" ? ADANERF_SAMPLING_FP32
                      : (settings.sampling == "fp16" ? ADANERF_SAMPLING_FP16 : ADANERF_SAMPLING_GUARDED));
  // --gpus N: rows are cut into strips, strip s belongs to (virtual) rank s % world; largest strip height <= 8 rows that
  // gives every rank the same number of strips.  --sub-shares P: every GPU hosts P virtual ranks (rank / P = its GPU), i.e. renders its
  // share of the frame as P concurrent sub-shares on P contexts / streams -- one sub-share's kernels take the CUs the other's tails
  // leave idle, the frame's latency does not grow (bench.py --sub-shares); default 2 on several GPUs when the rows split evenly
  auto even_split = [&](int ranks) {
    for (int sr = 8; sr >= 1; --sr)
      if (opt.height % sr == 0 && (opt.height / sr) % ranks == 0) return true;
    return false;
  };
  const int parts = settings.sub_shares > 0 ? settings.sub_shares : (settings.gpus > 1 && even_split(2 * settings.gpus) ? 2 : 1);
  const int world = settings.gpus * parts;
  if (world > 1 && settings.render_oracle) {
    err = "--oracle renders one context's rays; use it with --gpus 1";
    return false;
  }
  int strip_rows = 8;
  for (int sr = 8; sr >= 1; --sr)
    if (opt.height % sr == 0 && (opt.height / sr) % world == 0) {
      strip_rows = sr;
      break;
    }
  opt.shard_world = world;
  // the guarded selection's audit fills the last round of its refinement pass instead of adding one (adanerf_hip.h); as in renderer.py
  opt.flags |= ADANERF_FLAG_GUARD_AUDIT_FILL;
  opt.strip_rows = strip_rows;
  for (int rank = 0; rank < world; ++rank) {
    opt.shard_rank = rank;
    opt.device_id = settings.same_device ? 0 : rank / parts;
    adanerf_ctx* c = nullptr;
    if (adanerf_create(settings.model_path.c_str(), &opt, &c) != ADANERF_OK) {
      err = adanerf_last_error(nullptr);
      return false;
    }
    if (rank == 0) ctx = c;
    else peers.push_back(c);
  }
  adanerf_get_info(ctx, &info_);
  world_ = world;
  strip_rows_ = strip_rows;
  if (settings.supersample > 1 && (world > 1 || settings.render_oracle || settings.reproject > 1)) {
    err = world > 1 ? "--supersample accumulates whole frames of one context; use it with --gpus 1"
                    : (settings.render_oracle ? "--supersample averages rendered frames; not with --oracle"
                                              : "--supersample: the mean of jittered frames has no depth map to warp by; not with --reproject");
    return false;
  }
  if (settings.reproject > 1 && (world > 1 || info_.use_ndc)) {
    err = world > 1 ? "--reproject warps whole frames of one context; use it with --gpus 1" : "--reproject: the depth of a useNDC model is NDC depth";
    return false;
  }
  if (settings.interpolate > 1 && (world > 1 || info_.use_ndc)) {
    err = world > 1 ? "--interpolate warps whole frames of one context; use it with --gpus 1" : "--interpolate: the depth of a useNDC model is NDC depth";
    return false;
  }
  if (settings.taa_alpha > 0.f && (world > 1 || settings.render_oracle || info_.use_ndc)) {
    err = world > 1 ? "--taa resolves whole frames of one context; use it with --gpus 1"
                    : (settings.render_oracle ? "--taa blends rendered frames; not with --oracle" : "--taa: the depth of a useNDC model is NDC depth");
    return false;
  }
  if (settings.taau_scale > 0 && info_.use_ndc) {
    err = "--taau: the depth of a useNDC model is NDC depth";
    return false;
  }
  if (settings.fovea_temporal_alpha > 0.f && info_.use_ndc) {
    err = "--fovea-temporal: the depth of a useNDC model is NDC depth";
    return false;
  }
  if (!allocFrameBuffers()) return false;
  if (settings.write_window &&
      adanerf_malloc(ctx, static_cast<size_t>(settings.window_width) * settings.window_height * 4, &d_window) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  camera.setPosition(info_.view_cell_center);   // Camera::init: pos = view-cell centre (camera.cpp:49)
  camera.setViewCell(info_.view_cell_size);
  if (world > 1 && adanerf_set_profiling(ctx, 1) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  render_oracle = settings.render_oracle;
  if (settings.sample_cap > 0.f) setSampleCap(settings.sample_cap);      // installed before the first frame; the library validates it there
  return true;
}

// The host's frame-sized buffers on rank 0.  The modes that share a buffer agree on its size: d_rgb is the fp32 frame, d_depth / d_acc the aux
// maps at the render size in all of them.  --taa, --taau and --fovea-temporal are mutually exclusive (settings.cpp), so the history has one
// size: S w x S h under --taau, the render size under the other two.
std::vector<NeuralRenderer::FrameBuffer> NeuralRenderer::frameBuffers() {
  const size_t n = static_cast<size_t>(info_.width) * info_.height;
  const bool taa = settings.taa_alpha > 0.f, taau = settings.taau_scale > 0, density = !settings.density_stride.empty(),
             fovea_temporal = density && settings.fovea_temporal_alpha > 0.f, supersample = settings.supersample > 1,
             contrast = supersample && settings.supersample_contrast >= 0.f, occluder = !settings.occluders.empty(), reproject = settings.reproject > 1,
             gather = reproject && settings.reproject_gather, pair = settings.interpolate > 1;
  const size_t N = taau ? n * settings.taau_scale * settings.taau_scale : n, hist = taa || taau || fovea_temporal ? N : 0;
  const size_t aux = taa || taau || fovea_temporal || reproject ? n : 0;
  std::vector<FrameBuffer> table = {
      {&d_frame, n * 4, RESET_SOURCE},
      {&d_rgb, taa || taau || density || supersample || occluder ? n * 12 : 0, 0},
      {&d_depth, aux * 4, RESET_SOURCE | RESET_HISTORY},
      {&d_acc, (occluder ? n : aux) * 4, RESET_SOURCE | RESET_HISTORY | RESET_OCCLUDER},
      {&d_up, taau ? N * 4 : 0, 0},
      {&d_dmask, density ? n : 0, RESET_FOVEA},
      {&d_sum, supersample ? n * 12 : 0, 0},
      {&d_stage, contrast ? n * 12 : 0, 0},
      {&d_cmask, contrast ? n : 0, 0},
      {&d_limit, occluder ? n * 4 : 0, RESET_OCCLUDER},      // the library drops the limit when rays_local changes
      {&d_behind, occluder ? n * 12 : 0, RESET_OCCLUDER},
      {&d_warp, reproject || pair ? n * 4 : 0, 0},
      {&d_wmask, reproject || pair ? n * 4 : 0, 0},          // (the mask is a byte per pixel: a quarter of its allocation)
      {&d_src_rgb, gather ? n * 12 : 0, RESET_SOURCE},
      {&d_warp_rgb, gather || pair ? n * 12 : 0, 0},
  };
  for (Keyframe& k : ip_key) {      // --interpolate: the two keyframes
    table.push_back({&k.rgba, pair ? n * 4 : 0, RESET_SOURCE});
    table.push_back({&k.rgb, pair ? n * 12 : 0, RESET_SOURCE});
    table.push_back({&k.depth, pair ? n * 4 : 0, RESET_SOURCE});
    table.push_back({&k.acc, pair ? n * 4 : 0, RESET_SOURCE});
  }
  for (int side = 0; side < 2; ++side) {
    table.push_back({&history.set[side][0], hist * 12, RESET_HISTORY});
    table.push_back({&history.set[side][1], hist * 4, RESET_HISTORY});
    table.push_back({&history.set[side][2], hist, RESET_HISTORY});
  }
  return table;
}

bool NeuralRenderer::allocFrameBuffers() {
  int resets = 0;
  for (const FrameBuffer& b : frameBuffers()) {
    if (*b.p && adanerf_free(ctx, *b.p) != ADANERF_OK) return err = adanerf_last_error(ctx), false;
    *b.p = nullptr;
    if (b.bytes == 0) continue;
    if (adanerf_malloc(ctx, b.bytes, b.p) != ADANERF_OK) return err = adanerf_last_error(ctx), false;
    resets |= b.resets;
  }
  d_shown = d_frame;
  if (resets & RESET_SOURCE) have_source = false, ip_keys = 0;
  if (resets & RESET_HISTORY) history.reset();
  if (resets & RESET_OCCLUDER) occ_have = false;
  if (resets & RESET_FOVEA) fovea_pending = true;
  // the aux outputs belong to the frame size (the library drops them when rays_local changes): the depth and acc maps of the temporal and
  // reprojection stages, the acc map alone under --occluder
  float* const aux_depth = settings.occluders.empty() ? static_cast<float*>(d_depth) : nullptr;
  if (d_acc && adanerf_set_aux_outputs(ctx, aux_depth, static_cast<float*>(d_acc)) != ADANERF_OK) return err = adanerf_last_error(ctx), false;
  if (world_ > 1) {
    const size_t payload = static_cast<size_t>(info_.rays_local_max) * 4;
    if (d_gathered && adanerf_free(ctx, d_gathered) != ADANERF_OK) return err = adanerf_last_error(ctx), false;
    d_gathered = nullptr;
    if (adanerf_malloc(ctx, payload * world_, &d_gathered) != ADANERF_OK) {
      err = adanerf_last_error(ctx);
      return false;
    }
    d_payload.resize(world_, nullptr);
    d_payload[0] = d_gathered;     // rank 0 renders straight into its slot
    for (int rank = 1; rank < world_; ++rank) {
      if (d_payload[rank] && adanerf_free(peers[rank - 1], d_payload[rank]) != ADANERF_OK) return err = adanerf_last_error(peers[rank - 1]), false;
      d_payload[rank] = nullptr;
      if (adanerf_malloc(peers[rank - 1], payload, &d_payload[rank]) != ADANERF_OK) {
        err = adanerf_last_error(peers[rank - 1]);
        return false;
      }
    }
  }
  return true;
}

// script token "size": every context (--gpus / --sub-shares) gets the same frame size before this frame, the frame buffers follow;
// the window size stays.  Without a device (--dry-run) the model directory is parsed again at the new size: the same validation.
bool NeuralRenderer::applyFrameSize() {
  if (!size_pending) return true;
  size_pending = false;
  const int w = want_width, h = want_height;
  if (!ctx) {
    Settings at = settings;
    at.width = static_cast<unsigned>(w);
    at.height = static_cast<unsigned>(h);
    const adanerf_options opt = options_of(at);
    if (adanerf_host_parse_model(settings.model_path.c_str(), &opt, &info_) != ADANERF_OK) return err = adanerf_last_error(nullptr), false;
  } else {
    // a live context keeps its strip height: the rows of the new size must split into those strips over the shares as evenly as at start
    if (world_ > 1 && (h % strip_rows_ != 0 || (h / strip_rows_) % world_ != 0)) {
      err = "size " + std::to_string(w) + " x " + std::to_string(h) + ": " + std::to_string(h) + " rows do not split into strips of " +
            std::to_string(strip_rows_) + " rows over " + std::to_string(world_) + " shares";
      return false;
    }
    for (adanerf_ctx* c : contexts())
      if (adanerf_set_frame_size(c, w, h) != ADANERF_OK) return err = adanerf_last_error(c), false;
    adanerf_get_info(ctx, &info_);
    if (!allocFrameBuffers()) return false;
    fovea_pending = true;      // the maps belong to the old rays_local
  }
  settings.width = static_cast<unsigned>(info_.width);
  settings.height = static_cast<unsigned>(info_.height);
  settings.total_size = settings.width * settings.height;
  return true;
}

// --fovea: every context (--gpus / --sub-shares) fills the maps of its own local rays from the gaze and installs them; again after a
// "gaze" token and after a "size" token (the library drops the maps with the old rays_local).  Until a "gaze" token the gaze is the centre
// of the frame in force.
bool NeuralRenderer::applyFovea() {
  if (settings.fovea_n.empty() || !fovea_pending || !ctx) return true;
  fovea_pending = false;
  if (!gaze_set) {
    gaze_x = 0.5f * static_cast<float>(info_.width);
    gaze_y = 0.5f * static_cast<float>(info_.height);
  }
  const std::vector<adanerf_ctx*> all = contexts();
  d_fovea_n.resize(all.size(), nullptr);
  d_fovea_thr.resize(all.size(), nullptr);
  for (size_t i = 0; i < all.size(); ++i) {
    adanerf_ctx* c = all[i];
    adanerf_info in;
    bool ok = adanerf_get_info(c, &in) == ADANERF_OK && adanerf_set_budget_map(c, nullptr, nullptr) == ADANERF_OK;
    if (ok && d_fovea_n[i]) ok = adanerf_free(c, d_fovea_n[i]) == ADANERF_OK && adanerf_free(c, d_fovea_thr[i]) == ADANERF_OK;      // synchronises
    d_fovea_n[i] = d_fovea_thr[i] = nullptr;
    ok = ok && adanerf_malloc(c, static_cast<size_t>(in.rays_local), &d_fovea_n[i]) == ADANERF_OK &&
         adanerf_malloc(c, static_cast<size_t>(in.rays_local) * sizeof(float), &d_fovea_thr[i]) == ADANERF_OK &&
         adanerf_foveate(c, gaze_x, gaze_y, static_cast<int32_t>(settings.fovea_radius.size()), settings.fovea_radius.data(), settings.fovea_n.data(),
                         settings.fovea_thr.data(), static_cast<uint8_t*>(d_fovea_n[i]), static_cast<float*>(d_fovea_thr[i])) == ADANERF_OK &&
         adanerf_set_budget_map(c, static_cast<const uint8_t*>(d_fovea_n[i]), static_cast<const float*>(d_fovea_thr[i])) == ADANERF_OK;
    if (!ok) return err = adanerf_last_error(c), false;
  }
  return true;
}

// --fovea-density: the mask of the gaze and the size in force, filled on the device; again after a "gaze" token and after a "size" token
// (allocFrameBuffers makes the buffer for the new size).  Until a "gaze" token the gaze is the centre of the frame in force.
bool NeuralRenderer::applyFoveaDensity() {
  if (settings.density_stride.empty() || !fovea_pending || !ctx) return true;
  fovea_pending = false;
  if (!gaze_set) {
    gaze_x = 0.5f * static_cast<float>(info_.width);
    gaze_y = 0.5f * static_cast<float>(info_.height);
  }
  if (adanerf_foveate_density(ctx, gaze_x, gaze_y, static_cast<int32_t>(settings.density_radius.size()), settings.density_radius.data(),
                              settings.density_stride.data(), static_cast<uint8_t*>(d_dmask)) != ADANERF_OK)
    return err = adanerf_last_error(ctx), false;
  return true;
}

// --fovea-density: the lattice of the mask rendered into d_frame / d_rgb (adanerf_render_masked), the pixels in between rebuilt from it in
// both (adanerf_fill_density).  *st describes the rendered rays.
bool NeuralRenderer::renderFoveated(adanerf_stats* st) {
  int32_t m = 0;
  if (adanerf_render_masked(ctx, static_cast<const uint8_t*>(d_dmask), 1u, d_frame, static_cast<float*>(d_rgb), st, &m) != ADANERF_OK ||
      adanerf_fill_density(ctx, static_cast<const uint8_t*>(d_dmask), info_.width, info_.height, static_cast<float*>(d_rgb), nullptr, nullptr, d_frame, nullptr) != ADANERF_OK ||
      adanerf_sync(ctx) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  s_density_rendered += m;
  if (settings.log_camera) std::printf("foveated %d rendered %d of %u\n", sample_count, static_cast<int>(m), settings.total_size);
  return true;
}

// --fovea-density with --fovea-temporal: frame k takes the phase adanerf_host_density_phase(k); the mask of the gaze in force at that phase,
// its lattice rendered into d_rgb and the aux maps, the pixels in between rebuilt in all three (adanerf_fill_density_phased), then
// adanerf_temporal_resolve_sparse (clamp on) against the history, which the result replaces; d_frame gets the resolved frame.  The history's
// depth is tested only when the pose differs from the history's (as renderer.py).
bool NeuralRenderer::renderFoveatedTemporal(adanerf_stats* st, const float rot[9]) {
  int32_t m = 0, px = 0, py = 0, rejected = 0;
  adanerf_host_density_phase(ft_k, &px, &py);
  ft_k = (ft_k + 1) % 64;
  const uint8_t* mask = static_cast<const uint8_t*>(d_dmask);
  const History::Inputs h = history.inputs(camera.getPosition(), rot);
  if (adanerf_foveate_density_phased(ctx, gaze_x, gaze_y, static_cast<int32_t>(settings.density_radius.size()), settings.density_radius.data(),
                                     settings.density_stride.data(), px, py, static_cast<uint8_t*>(d_dmask)) != ADANERF_OK ||
      adanerf_render_masked(ctx, mask, 1u, nullptr, static_cast<float*>(d_rgb), st, &m) != ADANERF_OK ||
      adanerf_fill_density_phased(ctx, mask, info_.width, info_.height, px, py, static_cast<float*>(d_rgb), static_cast<float*>(d_depth), static_cast<float*>(d_acc),
                                  nullptr, nullptr) != ADANERF_OK ||
      adanerf_temporal_resolve_sparse(ctx, mask, px, py, static_cast<const float*>(d_rgb), static_cast<const float*>(d_depth), static_cast<const float*>(d_acc),
                                      camera.getPosition(), rot, h.rgb, h.depth, h.count, h.prev_pos, h.prev_rot, settings.fovea_temporal_alpha, 0.02f, 0.5f,
                                      ADANERF_TEMPORAL_CLAMP, h.out_rgb, h.out_depth, h.out_count, d_frame, nullptr, &rejected) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  history.commit(camera.getPosition(), rot);
  s_rejected += rejected;
  s_density_rendered += m;
  if (settings.log_camera)
    std::printf("foveated %d phase %d %d rendered %d of %u rejected %d\n", sample_count, static_cast<int>(px), static_cast<int>(py), static_cast<int>(m),
                settings.total_size, static_cast<int>(rejected));
  return true;
}

// a setting every context (--gpus / --sub-shares) gets before this frame.  It shows from this frame on: render it instead of warping the
// source frame, and --taa does not blend it with frames of the old setting.
template <class Set>
bool NeuralRenderer::applyToAll(Set set) {
  for (adanerf_ctx* c : contexts())
    if (set(c) != ADANERF_OK) return err = adanerf_last_error(c), false;
  have_source = false;
  ip_keys = 0;
  history.reset();
  return true;
}

bool NeuralRenderer::render() {
  float rot[9];
  camera.getRotMatrix(rot);
  if (!applyFrameSize()) return false;
  if (selection_pending) {      // script tokens "n" / "thr": every context (--gpus / --sub-shares) gets the same pair before this frame
    selection_pending = false;
    if (!applyToAll([&](adanerf_ctx* c) { return adanerf_set_selection(c, want_samples, want_threshold); })) return false;
    want_samples = 0;
    want_threshold = -1.f;
    adanerf_get_info(ctx, &info_);
  }
  if (cap_pending) {      // --sample-cap / script token "cap": every context (--gpus / --sub-shares) gets the same bound before this frame
    cap_pending = false;
    if (!applyToAll([&](adanerf_ctx* c) { return adanerf_set_sample_cap(c, want_cap); })) return false;
    cap_in_force = want_cap;
  }
  if (!applyFovea()) return false;
  if (!applyFoveaDensity()) return false;
  if (adanerf_set_camera(ctx, camera.getPosition(), rot) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  if (render_oracle) {   // imagegenerator.cpp:316-317: sampling network only, top-3 bins as RGB
    if (adanerf_render_oracle(ctx, d_frame) != ADANERF_OK || adanerf_sync(ctx) != ADANERF_OK) {
      err = adanerf_last_error(ctx);
      return false;
    }
    sample_count++;
    have_source = false;      // the debug view has no depth to warp
    ip_keys = 0;
    history.reset();          // nor is it a frame --taa may blend with
    d_shown = d_frame;
    return writeImageToFile();
  }
  if (settings.reproject > 1 && have_source && since_render + 1 < settings.reproject) return warp(rot);
  if (settings.interpolate > 1) return interpolate(rot);
  adanerf_stats st;
  std::memset(&st, 0, sizeof(st));
  if (!peers.empty()) {
    // every GPU renders its strips (launches are asynchronous: the GPUs run concurrently), each payload is copied to
    // the display GPU over xGMI behind its render, and rank 0 de-interleaves; one host sync at the end of the frame.
    // Rank 0 is enqueued first so that its stream does not wait for the peers before it starts.
    const size_t payload = static_cast<size_t>(info_.rays_local_max) * 4;
    if (adanerf_render(ctx, d_payload[0], nullptr, nullptr) != ADANERF_OK) {
      err = adanerf_last_error(ctx);
      return false;
    }
    for (size_t i = 0; i < peers.size(); ++i) {
      if (adanerf_set_camera(peers[i], camera.getPosition(), rot) != ADANERF_OK ||
          adanerf_render(peers[i], d_payload[i + 1], nullptr, nullptr) != ADANERF_OK ||
          adanerf_gather_to(ctx, static_cast<char*>(d_gathered) + (i + 1) * payload, peers[i], d_payload[i + 1], payload) != ADANERF_OK) {
        err = adanerf_last_error(peers[i]);
        return false;
      }
    }
    if (adanerf_assemble_strips(ctx, d_gathered, d_frame) != ADANERF_OK || adanerf_sync(ctx) != ADANERF_OK) {
      err = adanerf_last_error(ctx);
      return false;
    }
    sample_count++;
    if (sample_count % logging_interval == 0) {
      // rank 0's share, accumulated on its stream by the profiling API (no per-frame sync); samples scaled to the frame
      int32_t frames = 0;
      if (adanerf_collect_stats(ctx, &st, &frames) == ADANERF_OK && frames > 0) {
        const double f = frames, world = static_cast<double>(peers.size() + 1);
        std::cout << "Inference 1:" << st.ms_sample_mlp / f << ", 2:" << st.ms_shade_mlp / f << " | fc1: 0"
                  << ", fc2: " << st.ms_compact / f << ", rm: " << st.ms_composite / f
                  << ", avg samples ppx: " << st.total_samples * world / f / settings.total_size
                  << " (total: " << static_cast<long long>(st.total_samples * world / f) << ")"
                  << ", N: " << info_.num_samples << ", thr: " << info_.threshold << ", size: " << info_.width << "x" << info_.height
                  << ", frames: " << sample_count << ", gpus: " << peers.size() + 1 << " (stage times: GPU 0's share)" << std::endl;
      }
    }
    return writeImageToFile();
  }
  if (settings.taau_scale > 0) {
    if (!renderUpsampled(&st, rot)) return false;
  } else if (settings.taa_alpha > 0.f) {
    if (!renderTemporal(&st, rot)) return false;
  } else if (!settings.occluders.empty()) {
    if (!renderHybrid(&st, rot)) return false;
  } else if (!settings.density_stride.empty()) {
    if (settings.fovea_temporal_alpha > 0.f ? !renderFoveatedTemporal(&st, rot) : !renderFoveated(&st)) return false;
  } else if (settings.supersample > 1 ? !renderSupersampled(&st)
                                      : adanerf_render(ctx, d_frame, static_cast<float*>(settings.reproject_gather ? d_src_rgb : nullptr), &st) != ADANERF_OK) {
    if (settings.supersample <= 1) err = adanerf_last_error(ctx);
    return false;
  }
  if (st.guard_widened > guard_widened_seen) {      // the guarded selection's monitor saw its band violated and widened it (adanerf_hip.h)
    guard_widened_seen = st.guard_widened;
    adanerf_info now;
    if (adanerf_get_info(ctx, &now) == ADANERF_OK)
      std::cout << "guarded sampling: " << st.guard_violations << " re-evaluated rays exceeded a measured bound (largest output error " << st.guard_max_seen
                << ", largest pair error " << st.guard_pair_seen << "), audit: " << st.guard_audit_mismatch << " of " << st.guard_audited
                << " decided rays selected differently; bounds widened to " << now.guard_eps << " / " << now.guard_eps_pair
                << " for the following frames" << std::endl;
  }
  if (cap_in_force > 0.f) {      // the frame is finished (stats synchronise): what the cap did to its last render
    adanerf_cap_report rep;
    if (adanerf_sample_cap_report(ctx, &rep) != ADANERF_OK) {
      err = adanerf_last_error(ctx);
      return false;
    }
    if (rep.threshold_max > s_cap_thr) s_cap_thr = rep.threshold_max;
    s_cap_selected += rep.samples_selected;
    s_cap_kept += rep.samples_kept;
  }
  s_inference1 += st.ms_sample_mlp;
  s_inference2 += st.ms_shade_mlp;
  s_fc2 += st.ms_compact;
  s_rm += st.ms_composite;
  s_total += st.ms_total;
  s_num_total_samples += st.total_samples;
  sample_count++;
  s_rendered++;
  if (settings.reproject > 1) {
    std::memcpy(src_pos, camera.getPosition(), sizeof(src_pos));
    std::memcpy(src_rot, rot, sizeof(src_rot));
    have_source = true;
    since_render = 0;
  }
  d_shown = settings.taau_scale > 0 ? d_up : d_frame;
  logInterval();
  return writeImageToFile();
}

// One render with the rays through (dx, dy) of their pixels.  The offset goes back to (0, 0) whatever happened; err is the first failure's.
template <class Render>
bool NeuralRenderer::renderAtOffset(float dx, float dy, Render render) {
  const bool ok = adanerf_set_pixel_offset(ctx, dx, dy) == ADANERF_OK && render();
  if (!ok) err = adanerf_last_error(ctx);      // before the offset goes back: that call succeeds and would not touch the message anyway
  const bool back = adanerf_set_pixel_offset(ctx, 0.f, 0.f) == ADANERF_OK;
  if (ok && !back) err = adanerf_last_error(ctx);
  return ok && back;
}

// --supersample S: S x S renders of this frame's camera at the offsets of the regular sub-pixel grid, summed on the device; d_frame gets
// the mean under the viewer's output contract.
bool NeuralRenderer::renderSupersampled(adanerf_stats* st) {
  if (settings.supersample_contrast >= 0.f) return renderSupersampledAdaptive(st);
  const int S = settings.supersample, renders = S * S, n = info_.width * info_.height;
  for (int k = 0; k < renders; ++k) {
    float dx = 0.f, dy = 0.f;
    adanerf_stats sk;
    std::memset(&sk, 0, sizeof(sk));
    if (adanerf_host_subpixel_grid(S, k, &dx, &dy) != ADANERF_OK) return err = adanerf_last_error(ctx), false;
    if (!renderAtOffset(dx, dy, [&] {
          return adanerf_render(ctx, nullptr, static_cast<float*>(d_rgb), &sk) == ADANERF_OK &&
                 adanerf_accumulate(ctx, static_cast<const float*>(d_rgb), n, static_cast<float*>(d_sum), k == 0) == ADANERF_OK;
        }))
      return false;
    const int64_t samples = st->total_samples + sk.total_samples;
    const float ms[5] = {st->ms_total + sk.ms_total, st->ms_sample_mlp + sk.ms_sample_mlp, st->ms_compact + sk.ms_compact, st->ms_shade_mlp + sk.ms_shade_mlp,
                         st->ms_composite + sk.ms_composite};
    *st = sk;      // the counters "since create" of the last render
    st->total_samples = samples;
    st->ms_total = ms[0];
    st->ms_sample_mlp = ms[1];
    st->ms_compact = ms[2];
    st->ms_shade_mlp = ms[3];
    st->ms_composite = ms[4];
  }
  st->total_samples /= renders;      // per rendered frame, as the log's "avg samples ppx" counts
  if (adanerf_resolve_mean(ctx, static_cast<const float*>(d_sum), n, renders, d_frame, nullptr) != ADANERF_OK || adanerf_sync(ctx) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  return true;
}

// --supersample S --supersample-contrast T: the centre frame (offset (0, 0)) into d_frame / d_rgb, its contrast mask, and -- if any pixel is
// flagged -- the S x S renders of the grid for the flagged pixels alone, summed and averaged over the centre frame.  A flagged pixel carries
// the bytes of --supersample S, every other the bytes of a plain render.  No aux or disparity map is installed on this path (--supersample
// refuses every option that installs one), so there is none to switch off for the masked passes.  *st: the centre frame's record, the
// stage times summed over all passes.
bool NeuralRenderer::renderSupersampledAdaptive(adanerf_stats* st) {
  const int S = settings.supersample, renders = S * S, w = info_.width, h = info_.height, n = w * h;
  const uint8_t* mask = static_cast<const uint8_t*>(d_cmask);
  float *rgb = static_cast<float*>(d_rgb), *stage = static_cast<float*>(d_stage), *sum = static_cast<float*>(d_sum);
  int32_t flagged = 0;
  if (!renderAtOffset(0.f, 0.f, [&] {
        return adanerf_render(ctx, d_frame, rgb, st) == ADANERF_OK &&
               adanerf_contrast_mask(ctx, rgb, w, h, settings.supersample_contrast, static_cast<uint8_t*>(d_cmask), &flagged) == ADANERF_OK;
      }))
    return false;
  for (int k = 0; flagged > 0 && k < renders; ++k) {
    float dx = 0.f, dy = 0.f;
    int32_t m = 0;
    adanerf_stats sk;
    std::memset(&sk, 0, sizeof(sk));
    if (adanerf_host_subpixel_grid(S, k, &dx, &dy) != ADANERF_OK) return err = adanerf_last_error(ctx), false;
    if (!renderAtOffset(dx, dy, [&] {
          return adanerf_render_masked(ctx, mask, 1u, nullptr, stage, &sk, &m) == ADANERF_OK &&
                 adanerf_accumulate_masked(ctx, stage, mask, 1u, n, sum, k == 0) == ADANERF_OK;
        }))
      return false;
    st->ms_total += sk.ms_total;
    st->ms_sample_mlp += sk.ms_sample_mlp;
    st->ms_compact += sk.ms_compact;
    st->ms_shade_mlp += sk.ms_shade_mlp;
    st->ms_composite += sk.ms_composite;
  }
  if ((flagged > 0 && adanerf_resolve_mean_masked(ctx, sum, mask, 1u, n, renders, d_frame, rgb) != ADANERF_OK) || adanerf_sync(ctx) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  s_refined += flagged;
  if (settings.log_camera) std::printf("adaptive supersample %d refined %d of %u\n", sample_count, static_cast<int>(flagged), settings.total_size);
  return true;
}

// --occluder: the spheres' camera-space depth for every pixel (adanerf_host_sphere_zc, per-pixel minimum on the host; the nearest sphere's
// flat colour behind it) filled again when the camera or the frame size has changed, one render under that limit, and the colour behind
// let through with the transmittance left (adanerf_blend_behind) into d_frame.
bool NeuralRenderer::renderHybrid(adanerf_stats* st, const float rot[9]) {
  const int w = info_.width, h = info_.height;
  const size_t n = static_cast<size_t>(w) * h;
  if (!occ_have || std::memcmp(occ_pos, camera.getPosition(), sizeof(occ_pos)) != 0 || std::memcmp(occ_rot, rot, sizeof(occ_rot)) != 0) {
    std::vector<float> limit(n, INFINITY), behind(n * 3, 0.f), one(n);
    for (const Settings::Occluder& o : settings.occluders) {
      if (adanerf_host_sphere_zc(w, h, info_.focal, camera.getPosition(), rot, o.center, o.radius, one.data()) != ADANERF_OK) {
        err = adanerf_last_error(nullptr);
        return false;
      }
      for (size_t i = 0; i < n; ++i)
        if (one[i] < limit[i]) {      // the nearest sphere; the first given on a tie
          limit[i] = one[i];
          std::memcpy(&behind[3 * i], o.rgb, sizeof(o.rgb));
        }
    }
    // the copies synchronise: no frame in flight still reads the buffers
    if (adanerf_memcpy_h2d(ctx, d_limit, limit.data(), n * sizeof(float)) != ADANERF_OK ||
        adanerf_memcpy_h2d(ctx, d_behind, behind.data(), n * 3 * sizeof(float)) != ADANERF_OK ||
        adanerf_set_depth_limit(ctx, static_cast<const float*>(d_limit)) != ADANERF_OK) {
      err = adanerf_last_error(ctx);
      return false;
    }
    std::memcpy(occ_pos, camera.getPosition(), sizeof(occ_pos));
    std::memcpy(occ_rot, rot, sizeof(occ_rot));
    occ_have = true;
  }
  if (adanerf_render(ctx, nullptr, static_cast<float*>(d_rgb), st) != ADANERF_OK ||
      adanerf_blend_behind(ctx, static_cast<const float*>(d_rgb), static_cast<const float*>(d_acc), static_cast<const float*>(d_behind), static_cast<int32_t>(n),
                           nullptr, d_frame) != ADANERF_OK ||
      adanerf_sync(ctx) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  return true;
}

// --taa / --taau: one render of this frame's camera into d_rgb at the next offset (*dx, *dy) of the S x S sub-pixel cycle
bool NeuralRenderer::renderJittered(int S, adanerf_stats* st, float* dx, float* dy) {
  if (adanerf_host_subpixel_grid(S, taa_k % (S * S), dx, dy) != ADANERF_OK) return err = adanerf_last_error(ctx), false;
  if (!renderAtOffset(*dx, *dy, [&] { return adanerf_render(ctx, nullptr, static_cast<float*>(d_rgb), st) == ADANERF_OK; })) return false;
  taa_k = (taa_k + 1) % (S * S);
  return true;
}

// --taa: one jittered render, then adanerf_temporal_resolve against the history (clamp on), which the result replaces; d_frame gets the
// resolved frame under the viewer's output contract.  The history's depth is tested only when the pose differs from the history's.
bool NeuralRenderer::renderTemporal(adanerf_stats* st, const float rot[9]) {
  float dx = 0.f, dy = 0.f;
  if (!renderJittered(settings.taa_grid, st, &dx, &dy)) return false;
  const History::Inputs h = history.inputs(camera.getPosition(), rot);
  int32_t rejected = 0;
  if (adanerf_temporal_resolve(ctx, static_cast<const float*>(d_rgb), static_cast<const float*>(d_depth), static_cast<const float*>(d_acc), camera.getPosition(), rot,
                               h.rgb, h.depth, h.count, h.prev_pos, h.prev_rot, settings.taa_alpha, settings.taa_tol, 0.5f, ADANERF_TEMPORAL_CLAMP, h.out_rgb,
                               h.out_depth, h.out_count, d_frame, nullptr, &rejected) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  history.commit(camera.getPosition(), rot);
  s_rejected += rejected;
  return true;
}

// --taau S: one jittered render, then adanerf_temporal_upsample (clamp on) into the history of S w x S h, which the result replaces; d_up
// gets the upsampled frame under the viewer's output contract.  The history's depth is tested only when the pose differs from the history's.
bool NeuralRenderer::renderUpsampled(adanerf_stats* st, const float rot[9]) {
  const int S = settings.taau_scale;
  float dx = 0.f, dy = 0.f;
  if (!renderJittered(S, st, &dx, &dy)) return false;
  const History::Inputs h = history.inputs(camera.getPosition(), rot);
  int32_t rejected = 0;
  if (adanerf_temporal_upsample(ctx, S, static_cast<const float*>(d_rgb), static_cast<const float*>(d_depth), static_cast<const float*>(d_acc), dx, dy,
                                camera.getPosition(), rot, h.rgb, h.depth, h.count, h.prev_pos, h.prev_rot, settings.taau_alpha, settings.taau_tol, 0.5f,
                                ADANERF_TEMPORAL_CLAMP, h.out_rgb, h.out_depth, h.out_count, d_up, nullptr, &rejected) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  history.commit(camera.getPosition(), rot);
  s_rejected += rejected;
  return true;
}

// --reproject K: the last rendered frame at this frame's camera (adanerf_reproject, holes filled from their neighbours, the rest black;
// --reproject-warp gather: adanerf_reproject_gather, unverified pixels keep their gathered colour, the rest black)
bool NeuralRenderer::warp(const float rot[9]) {
  int32_t holes = 0;
  const int rc = settings.reproject_gather
                     ? adanerf_reproject_gather(ctx, static_cast<const float*>(d_src_rgb), static_cast<const float*>(d_depth), static_cast<const float*>(d_acc), src_pos,
                                                src_rot, camera.getPosition(), rot, 0.5f, settings.reproject_tol, settings.reproject_iterations, 0xFF000000u,
                                                ADANERF_GATHER_GUESS, static_cast<float*>(d_warp_rgb), d_warp, nullptr, static_cast<uint8_t*>(d_wmask), &holes)
                     : adanerf_reproject(ctx, d_frame, static_cast<const float*>(d_depth), static_cast<const float*>(d_acc), src_pos, src_rot, camera.getPosition(),
                                         rot, 0.5f, 0xFF000000u, ADANERF_REPROJECT_FILL, d_warp, nullptr, static_cast<uint8_t*>(d_wmask), &holes);
  if (rc != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  if (!settings.rerender.empty()) {
    // --rerender: the holes (mask 0; unsourced: the filled pixels, mask 2, too) at this frame's camera, which render() has set.  The aux maps
    // belong to the source frame and the next warp reads them: off for this call.
    int32_t m = 0;
    const bool ok = adanerf_set_aux_outputs(ctx, nullptr, nullptr) == ADANERF_OK &&
                    adanerf_render_masked(ctx, static_cast<const uint8_t*>(d_wmask), settings.rerender == "holes" ? 1u : 5u, d_warp, nullptr, nullptr, &m) == ADANERF_OK;
    if (!ok) err = adanerf_last_error(ctx);
    const bool back = adanerf_set_aux_outputs(ctx, static_cast<float*>(d_depth), static_cast<float*>(d_acc)) == ADANERF_OK;
    if (ok && !back) err = adanerf_last_error(ctx);
    if (!ok || !back) return false;
    s_rerendered += m;
    if (settings.log_camera) std::printf("warped %d holes %d rerendered %d\n", sample_count, static_cast<int>(holes), static_cast<int>(m));
  }
  since_render++;
  sample_count++;
  s_warped++;
  s_holes += holes;
  d_shown = d_warp;
  logInterval();
  return writeImageToFile();
}

// one render at this frame's camera into keyframe slot `into`, its depth_map and acc_map with it
bool NeuralRenderer::renderKeyframe(int into, adanerf_stats* st, const float rot[9]) {
  Keyframe& k = ip_key[into];
  if (adanerf_set_aux_outputs(ctx, static_cast<float*>(k.depth), static_cast<float*>(k.acc)) != ADANERF_OK ||
      adanerf_render(ctx, k.rgba, static_cast<float*>(k.rgb), st) != ADANERF_OK)
    return err = adanerf_last_error(ctx), false;
  std::memcpy(k.pos, camera.getPosition(), sizeof(k.pos));
  std::memcpy(k.rot, rot, sizeof(k.rot));
  return true;
}

// --interpolate K: the frames are shown K calls late.  On the calls with ip_call % K == 0 a keyframe is rendered at the camera of the moment:
// it becomes B, the one that was B becomes A and is shown.  On the K - 1 calls in between the frame is adanerf_reproject_pair(A, B) at the
// camera queued K calls earlier (fill on, the weight of adanerf_host_pair_weight).  Until two keyframes exist every call renders and shows
// its own frame.
bool NeuralRenderer::interpolate(const float rot[9]) {
  const int K = settings.interpolate;
  if (ip_keys == 0) ip_call = 0;
  if (static_cast<int>(ip_ring.size()) != K) ip_ring.assign(K, Pose());
  Pose& slot = ip_ring[ip_call % K];
  const Pose late = slot;      // the camera of K calls ago
  std::memcpy(slot.pos, camera.getPosition(), sizeof(slot.pos));
  std::memcpy(slot.rot, rot, sizeof(slot.rot));
  const bool key = ip_call % K == 0;
  if (key || ip_keys < 2) {
    adanerf_stats st;
    std::memset(&st, 0, sizeof(st));
    const int into = ip_keys == 0 ? 0 : 1 - ip_newer;      // the older keyframe's slot; before there are two, frames in between borrow it too
    if (!renderKeyframe(into, &st, rot)) return false;
    d_shown = ip_key[into].rgba;
    if (key) {
      ip_newer = into;
      ip_keys = std::min(ip_keys + 1, 2);
      if (ip_keys == 2) d_shown = ip_key[1 - ip_newer].rgba;      // A: the keyframe of K calls ago
    }
    s_inference1 += st.ms_sample_mlp;
    s_inference2 += st.ms_shade_mlp;
    s_fc2 += st.ms_compact;
    s_rm += st.ms_composite;
    s_total += st.ms_total;
    s_num_total_samples += st.total_samples;
    s_rendered++;
  } else {
    const Keyframe &A = ip_key[1 - ip_newer], &B = ip_key[ip_newer];
    float weight_b = 0.5f;
    int32_t holes = 0;
    if (adanerf_host_pair_weight(late.pos, A.pos, B.pos, &weight_b) != ADANERF_OK ||
        adanerf_reproject_pair(ctx, static_cast<const float*>(A.rgb), static_cast<const float*>(A.depth), static_cast<const float*>(A.acc), A.pos, A.rot,
                               static_cast<const float*>(B.rgb), static_cast<const float*>(B.depth), static_cast<const float*>(B.acc), B.pos, B.rot, late.pos,
                               late.rot, weight_b, 0.5f, 0.05f, 0xFF000000u, ADANERF_REPROJECT_FILL, static_cast<float*>(d_warp_rgb), d_warp, nullptr,
                               static_cast<uint8_t*>(d_wmask), nullptr, &holes) != ADANERF_OK)
      return err = adanerf_last_error(ctx), false;
    int32_t m = 0;
    if (!settings.rerender.empty()) {
      // --rerender: the holes (unsourced: the filled pixels too) at the camera of K calls ago; the aux maps belong to the keyframes: off for this call
      const bool ok = adanerf_set_camera(ctx, late.pos, late.rot) == ADANERF_OK && adanerf_set_aux_outputs(ctx, nullptr, nullptr) == ADANERF_OK &&
                      adanerf_render_masked(ctx, static_cast<const uint8_t*>(d_wmask), settings.rerender == "holes" ? 1u : 5u, d_warp, nullptr, nullptr, &m) == ADANERF_OK;
      if (!ok) return err = adanerf_last_error(ctx), false;
      s_rerendered += m;
    }
    if (settings.log_camera) std::printf("interpolated %d holes %d rerendered %d weight %g\n", sample_count, static_cast<int>(holes), static_cast<int>(m), weight_b);
    s_warped++;
    s_holes += holes;
    d_shown = d_warp;
  }
  ip_call++;
  sample_count++;
  logInterval();
  return writeImageToFile();
}

void NeuralRenderer::logInterval() {
  if (sample_count % logging_interval != 0) return;
  // same fields as the reference's log line; fc1 (ray/oracle features) is fused into "Inference 1".  --reproject K > 1: the averages are
  // over the rendered frames of the interval, and the line gains the holes per warped frame
  const int rendered = settings.reproject > 1 || settings.interpolate > 1 ? std::max(s_rendered, 1) : logging_interval;
  std::cout << "Inference 1:" << s_inference1 / rendered << ", 2:" << s_inference2 / rendered << " | fc1: 0"
            << ", fc2: " << s_fc2 / rendered << ", rm: " << s_rm / rendered
            << ", avg samples ppx: " << s_num_total_samples / static_cast<double>(rendered) / settings.total_size
            << " (total: " << s_num_total_samples / rendered << ")"
            << ", N: " << info_.num_samples << ", thr: " << info_.threshold << ", size: " << info_.width << "x" << info_.height
            << ", frames: " << sample_count << ", frame ms: " << s_total / rendered;
  if (settings.supersample > 1) std::cout << ", renders per frame: " << settings.supersample * settings.supersample;
  if (settings.supersample_contrast >= 0.f) std::cout << ", refined fraction: " << s_refined / static_cast<double>(logging_interval) / settings.total_size;
  if (settings.taa_alpha > 0.f) std::cout << ", taa rejected: " << s_rejected / static_cast<double>(logging_interval) / settings.total_size;
  if (settings.taau_scale > 0)
    std::cout << ", taau rejected: " << s_rejected / static_cast<double>(logging_interval) / settings.total_size / (settings.taau_scale * settings.taau_scale);
  if (settings.reproject > 1) std::cout << ", holes: " << s_holes / static_cast<double>(std::max(s_warped, 1)) << " (" << s_warped << " warped frames)";
  if (settings.interpolate > 1) std::cout << ", holes: " << s_holes / static_cast<double>(std::max(s_warped, 1)) << " (" << s_warped << " interpolated frames)";
  if (settings.fovea_temporal_alpha > 0.f) std::cout << ", fovea-temporal rejected: " << s_rejected / static_cast<double>(logging_interval) / settings.total_size;
  if (!settings.density_stride.empty()) std::cout << ", rendered fraction: " << s_density_rendered / static_cast<double>(logging_interval) / settings.total_size;
  if (cap_in_force > 0.f)
    std::cout << ", sample cap: " << cap_in_force << ", cap threshold max: " << s_cap_thr << ", cap kept / selected: " << s_cap_kept << " / " << s_cap_selected;
  if (!settings.rerender.empty()) std::cout << ", rerendered: " << s_rerendered / static_cast<double>(std::max(s_warped, 1));
  std::cout << std::endl;
  s_inference1 = s_inference2 = s_fc2 = s_rm = s_total = 0;
  s_num_total_samples = 0;
  s_holes = 0;
  s_rerendered = 0;
  s_density_rendered = 0;
  s_refined = 0;
  s_rejected = 0;
  s_rendered = s_warped = 0;
  s_cap_thr = -1.f / 0.f;
  s_cap_selected = s_cap_kept = 0;
}

// -w: the frame at its render size, exactly as before; --write-window: the frame as the viewer's blit would show it in a window of
// -ws W H (interoprenderbuffer.cpp:87), presented on the device
bool NeuralRenderer::writeImageToFile() {
  const void* shown = d_shown ? d_shown : d_frame;
  const int up = shown == d_up && d_up ? settings.taau_scale : 1;      // --taau: the shown frame is S times the render size
  const int sw = static_cast<int>(settings.width) * up, sh = static_cast<int>(settings.height) * up;
  if (settings.write_images && !writeBmp("out.bmp", shown, sw, sh)) return false;
  if (!settings.write_window) return true;
  const int ww = static_cast<int>(settings.window_width), wh = static_cast<int>(settings.window_height);
  const int filter = settings.present_filter == "area" ? ADANERF_PRESENT_AREA
                                                       : (settings.present_filter == "linear" ? ADANERF_PRESENT_LINEAR
                                                                                              : (settings.present_filter == "nearest" ? ADANERF_PRESENT_NEAREST : 0));
  if (adanerf_present(ctx, shown, sw, sh, d_window, ww, wh, filter) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  return writeBmp("out_window.bmp", d_window, ww, wh);
}

bool NeuralRenderer::writeBmp(const std::string& name, const void* d_image, int w, int h) {
  std::vector<unsigned char> image(static_cast<size_t>(w) * h * 4);
  if (adanerf_memcpy_d2h(ctx, image.data(), d_image, image.size()) != ADANERF_OK) {
    err = adanerf_last_error(ctx);
    return false;
  }
  std::string path = settings.model_path;
  if (!path.empty() && path.back() != '/') path += '/';
  path += name;
  std::ofstream fout(path, std::ios::binary);
  if (!fout) {
    err = "cannot write " + path;
    return false;
  }
  // 24-bit BMP, bottom-up rows, BGR, rows padded to 4 bytes
  const int row_bytes = (w * 3 + 3) & ~3;
  const uint32_t data_size = static_cast<uint32_t>(row_bytes) * h, off = 54, file_size = off + data_size;
  unsigned char hdr[54] = {'B', 'M'};
  auto put32 = [&](int at, uint32_t v) {
    hdr[at] = v & 255;
    hdr[at + 1] = (v >> 8) & 255;
    hdr[at + 2] = (v >> 16) & 255;
    hdr[at + 3] = (v >> 24) & 255;
  };
  put32(2, file_size);
  put32(10, off);
  put32(14, 40);
  put32(18, static_cast<uint32_t>(w));
  put32(22, static_cast<uint32_t>(h));
  hdr[26] = 1;
  hdr[28] = 24;
  put32(34, data_size);
  fout.write(reinterpret_cast<char*>(hdr), 54);
  std::vector<unsigned char> row(row_bytes, 0);
  for (int y = h - 1; y >= 0; --y) {
    for (int x = 0; x < w; ++x) {
      const unsigned char* px = &image[(static_cast<size_t>(y) * w + x) * 4];
      row[3 * x + 0] = px[2];
      row[3 * x + 1] = px[1];
      row[3 * x + 2] = px[0];
    }
    fout.write(reinterpret_cast<char*>(row.data()), row_bytes);
  }
  return true;
}
