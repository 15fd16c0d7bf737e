// The image-space stages of the C ABI (include/adanerf_hip.h): entry points that work on finished images, with their kernels (compiled
// here and nowhere else; no MFMA in them).  They use none of the networks, the batch buffers, the guard or the selection of
// adanerf_hip.hip: only the context's stream, its frame geometry and StageScratch.  A new stage takes its checks from the helpers below
// wherever its rule and its wording are theirs.
#include "context.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "flip_tables.hpp"
#include "k_flip.hip.hpp"
#include "k_present.hip.hpp"
#include "k_reproject.hip.hpp"
#include "k_reproject_gather.hip.hpp"
#include "k_reproject_pair.hip.hpp"
#include "k_accumulate.hip.hpp"
#include "k_temporal.hip.hpp"
#include "k_upsample.hip.hpp"
#include "k_blend.hip.hpp"
#include "k_density.hip.hpp"
#include "k_sparse_temporal.hip.hpp"
#include "k_contrast.hip.hpp"

using namespace adanerf;

namespace {

// ---- what the stages share; `who` names the entry point in the error text ----------------------------------------------------

int reject(adanerf_ctx* c, int code, const char* who, const std::string& what) { return fail(c, code, std::string(who) + ": " + what); }

// byte ranges [a, a + na) and [b, b + nb) share a byte
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// one of these pointers is not 4-byte aligned (a NULL is)
bool misaligned4(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 3) != 0;
}

// The pose of the frame and the one it is carried from or to: none NULL, every entry finite.  Without `has_prev` (a temporal stage
// that was handed no history) the previous pose is not read.
int check_poses(adanerf_ctx* c, const char* who, const float pos[3], const float rot[9], const float prev_pos[3], const float prev_rot[9], bool has_prev) {
  if (!pos || !rot || (has_prev && (!prev_pos || !prev_rot))) return reject(c, ADANERF_EINVAL, who, "NULL pose");
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(rot[k]) || (k < 3 && !std::isfinite(pos[k])) || (has_prev && (!std::isfinite(prev_rot[k]) || (k < 3 && !std::isfinite(prev_pos[k])))))
      return reject(c, ADANERF_EINVAL, who, "a pose entry is not finite");
  return ADANERF_OK;
}

// the blend of a temporal resolve; every comparison also refuses a NaN
int check_blend(adanerf_ctx* c, const char* who, float alpha, float depth_tol, float acc_min, int32_t flags) {
  if (!(alpha > 0.f && alpha <= 1.f)) return reject(c, ADANERF_EINVAL, who, "alpha must lie in (0, 1]");
  if (!(depth_tol >= 0.f)) return reject(c, ADANERF_EINVAL, who, "depth_tol must be >= 0");
  if (!(acc_min >= 0.f)) return reject(c, ADANERF_EINVAL, who, "acc_min must be >= 0");
  if (flags & ~ADANERF_TEMPORAL_CLAMP) return reject(c, ADANERF_EINVAL, who, "flags must be 0 or ADANERF_TEMPORAL_CLAMP");
  return ADANERF_OK;
}

// what a stage that follows a depth map through a change of pose needs of the context
int check_depth_frames(adanerf_ctx* c, const char* who) {
  if (c->ms.info.use_ndc) return reject(c, ADANERF_EUNSUPPORTED, who, "the depth_map of a useNDC model is NDC depth, not a distance along the ray");
  if (c->ms.rg.world != 1) return reject(c, ADANERF_EUNSUPPORTED, who, "whole frames only (shard_world must be 1)");
  return ADANERF_OK;
}

void copy_pose(float to_pos[3], float to_rot[9], const float pos[3], const float rot[9]) {
  std::memcpy(to_pos, pos, 3 * sizeof(float));
  std::memcpy(to_rot, rot, 9 * sizeof(float));
}

// The one device word a stage counts in: the holes of adanerf_reproject, the rejected pixels of the three temporal resolves, the
// unfilled pixels of adanerf_fill_density[_phased], the flagged pixels of adanerf_contrast_mask.  All six enqueue on the context's
// stream, where each zeroes the word, counts and reads it back before the next one starts: they share it.  Allocated on first use.
int stage_count(adanerf_ctx* c, int32_t** count) {
  const int rc = c->stages.count.p ? ADANERF_OK : dev_alloc(c, &c->stages.count, 64);
  *count = reinterpret_cast<int32_t*>(c->stages.count.p);
  return rc;
}

// a count (or FLIP's mean: any 4-byte word) to the caller who asked for it, behind everything enqueued so far
int read_count(adanerf_ctx* c, const void* d_word, void* out) {
  if (!out) return ADANERF_OK;
  HIP_TRY(c, hipMemcpyAsync(out, d_word, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_RETURN(c, hipStreamSynchronize(c->stream));
}

// at least `bytes` in *b, for a buffer that enqueued work may still use at its smaller size
int grow_in_use(adanerf_ctx* c, DevBuf* b, size_t bytes) {
  if (b->bytes >= bytes) return ADANERF_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return dev_alloc(c, b, bytes);
}

// what adanerf_temporal_resolve and its sparse form hand their kernels: the context's generator at pixel centres (the offset of
// adanerf_set_pixel_offset is not applied) with the current pose; without a history the previous pose is not read
TemporalParams temporal_params(const adanerf_ctx* c, const float cur_pos[3], const float cur_rot[9], bool has_prev, const float prev_pos[3], const float prev_rot[9],
                               float alpha, float depth_tol, float acc_min, int32_t flags) {
  TemporalParams p{};
  p.g = c->ms.rg;
  copy_pose(p.g.pos, p.g.rot, cur_pos, cur_rot);
  if (has_prev) copy_pose(p.prev_pos, p.prev_rot, prev_pos, prev_rot);
  p.alpha = alpha;
  p.depth_tol = depth_tol;
  p.acc_min = acc_min;
  p.origin_is_camera = c->ms.coarse_fine ? 1 : 0;
  p.clamp = (flags & ADANERF_TEMPORAL_CLAMP) ? 1 : 0;
  return p;
}

// ---- bodies of the stages that have one apart from their entry point ------------------------------------------------------------

int flip_prepare(adanerf_ctx* c, double ppd) {
  StageScratch& s = c->stages;
  if (s.flip_tab.p && s.flip_ppd == ppd) return ADANERF_OK;
  std::vector<float> tab;
  if (!flip_tables(ppd, &tab, &s.flip_params))
    return fail(c, ADANERF_EINVAL, "adanerf_flip: filter radius outside 1.." + std::to_string(kFlipMaxRadius) + " at this pixels_per_degree");
  if (int rc = dev_alloc(c, &s.flip_tab, tab.size() * sizeof(float))) return rc;
  s.flip_ppd = 0.0;
  HIP_TRY(c, hipMemcpyAsync(s.flip_tab.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // `tab` leaves scope
  s.flip_ppd = ppd;
  return ADANERF_OK;
}

int launch_flip(adanerf_ctx* c, const float* d_test, const float* d_ref, int width, int height, double ppd, float* d_map, float* mean_out) {
  if (int rc = flip_prepare(c, ppd)) return rc;
  StageScratch& s = c->stages;
  FlipParams p = s.flip_params;
  p.tiles_x = (width + kFlipTile - 1) / kFlipTile;
  const int tiles = p.tiles_x * ((height + kFlipTile - 1) / kFlipTile);
  if (int rc = dev_alloc(c, &s.flip_partial, static_cast<size_t>(tiles) * sizeof(double))) return rc;
  if (int rc = dev_alloc(c, &s.flip_mean, sizeof(float))) return rc;
  p.test = d_test;
  p.ref = d_ref;
  p.map = d_map;
  p.partial = reinterpret_cast<double*>(s.flip_partial.p);
  p.tab = reinterpret_cast<const float*>(s.flip_tab.p);
  p.width = width;
  p.height = height;
  const int S = kFlipTile + 2 * p.halo;
  const size_t lds = static_cast<size_t>(6) * S * S * sizeof(float);      // >= 24 KB: also holds the 2 KB reduction tree
  if (lds > 64 * 1024 && !s.flip_lds_raised) {
    constexpr int Smax = kFlipTile + 2 * kFlipMaxRadius;
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(flip_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 6 * Smax * Smax * static_cast<int>(sizeof(float))));
    s.flip_lds_raised = true;
  }
  hipLaunchKernelGGL(flip_kernel, dim3(tiles), dim3(kFlipThreads), lds, c->stream, p);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(flip_mean_kernel, dim3(1), dim3(kFlipThreads), 0, c->stream, reinterpret_cast<const double*>(s.flip_partial.p), tiles,
                     static_cast<double>(width) * height, reinterpret_cast<float*>(s.flip_mean.p));
  HIP_TRY(c, hipGetLastError());
  return read_count(c, s.flip_mean.p, mean_out);
}

// N5 / N11: the sum and the mean of several frames, of every pixel (!masked) or of the pixels a mask selects
int accumulate(adanerf_ctx* c, const char* who, const float* d_rgb, bool masked, const uint8_t* d_mask, uint32_t values, int32_t n_rays, float* d_sum, int32_t first) {
  if (!c) return ADANERF_EINVAL;
  if (!d_rgb || !d_sum) return reject(c, ADANERF_EINVAL, who, "NULL image");
  if (masked && (!d_mask || values == 0)) return reject(c, ADANERF_EINVAL, who, "NULL mask, or values == 0 selects no mask byte");
  if (n_rays < 0 || n_rays > 0x7fffffff / 3) return reject(c, ADANERF_EINVAL, who, "n_rays must be >= 0 and n_rays * 3 <= 2^31 - 1");
  if (misaligned4({d_rgb, d_sum})) return reject(c, ADANERF_EINVAL, who, "images must be 4-byte aligned");
  const size_t bytes = static_cast<size_t>(n_rays) * 3 * sizeof(float);
  if (d_rgb != d_sum && ranges_overlap(d_rgb, bytes, d_sum, bytes)) return reject(c, ADANERF_EINVAL, who, "frame and sum overlap without being the same image");
  if (masked && ranges_overlap(d_mask, static_cast<size_t>(n_rays), d_sum, bytes)) return reject(c, ADANERF_EINVAL, who, "the mask overlaps the sum");
  BIND(c);
  if (n_rays == 0) return ADANERF_OK;
  const int n = n_rays * 3;
  const dim3 grid(std::min((n + 255) / 256, 65536)), block(256);      // grid-stride beyond 2^24 values
  if (masked) hipLaunchKernelGGL(accumulate_masked_kernel, grid, block, 0, c->stream, d_rgb, d_mask, values, d_sum, n, first != 0 ? 1 : 0);
  else hipLaunchKernelGGL(accumulate_kernel, grid, block, 0, c->stream, d_rgb, d_sum, n, first != 0 ? 1 : 0);
  HIP_RETURN(c, hipGetLastError());
}

int resolve_mean(adanerf_ctx* c, const char* who, const float* d_sum, bool masked, const uint8_t* d_mask, uint32_t values, int32_t n_rays, int32_t frames,
                 void* d_rgba8, float* d_rgb) {
  if (!c) return ADANERF_EINVAL;
  if (!d_sum || (!d_rgba8 && !d_rgb)) return reject(c, ADANERF_EINVAL, who, "NULL sum, or both outputs NULL");
  if (masked && (!d_mask || values == 0)) return reject(c, ADANERF_EINVAL, who, "NULL mask, or values == 0 selects no mask byte");
  if (n_rays < 0 || n_rays > 0x7fffffff / 3) return reject(c, ADANERF_EINVAL, who, "n_rays must be >= 0 and n_rays * 3 <= 2^31 - 1");
  if (frames < 1 || frames > 65536) return reject(c, ADANERF_EINVAL, who, "frames must be in 1..65536");
  if (misaligned4({d_sum, d_rgba8, d_rgb})) return reject(c, ADANERF_EINVAL, who, "images must be 4-byte aligned");
  const size_t bytes = static_cast<size_t>(n_rays) * 3 * sizeof(float), bytes8 = static_cast<size_t>(n_rays) * 4;
  if ((d_rgb && d_rgb != d_sum && ranges_overlap(d_sum, bytes, d_rgb, bytes)) ||
      (d_rgba8 && (ranges_overlap(d_sum, bytes, d_rgba8, bytes8) || (d_rgb && ranges_overlap(d_rgb, bytes, d_rgba8, bytes8)))))
    return reject(c, ADANERF_EINVAL, who, "images overlap (only d_rgb_f32_out may be d_sum itself)");
  if (masked && ((d_rgb && ranges_overlap(d_mask, static_cast<size_t>(n_rays), d_rgb, bytes)) ||
                 (d_rgba8 && ranges_overlap(d_mask, static_cast<size_t>(n_rays), d_rgba8, bytes8))))
    return reject(c, ADANERF_EINVAL, who, "the mask overlaps an output");
  BIND(c);
  if (n_rays == 0) return ADANERF_OK;
  const dim3 grid((n_rays + 255) / 256), block(256);
  if (masked)
    hipLaunchKernelGGL(resolve_mean_masked_kernel, grid, block, 0, c->stream, d_sum, d_mask, values, n_rays, static_cast<float>(frames), d_rgb,
                       static_cast<uchar4*>(d_rgba8));
  else hipLaunchKernelGGL(resolve_mean_kernel, grid, block, 0, c->stream, d_sum, n_rays, static_cast<float>(frames), d_rgb, static_cast<uchar4*>(d_rgba8));
  HIP_RETURN(c, hipGetLastError());
}

// N10 / N12: adanerf_foveate_density and adanerf_fill_density are phase (0, 0) of their phased forms
int foveate_density_at(adanerf_ctx* c, const char* who, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride,
                       int32_t phase_x, int32_t phase_y, uint8_t* d_mask) {
  if (!c) return ADANERF_EINVAL;
  if (!d_mask) return reject(c, ADANERF_EINVAL, who, "NULL mask");
  DensityRule f;
  if (const char* why = density_rule_fill(gaze_x, gaze_y, n_rings, radius_px, stride, &f, phase_x, phase_y)) return reject(c, ADANERF_EINVAL, who, why);
  // not check_depth_frames' line: no depth is followed here, and the text gives this stage's own reason
  if (c->ms.rg.world != 1) return reject(c, ADANERF_EUNSUPPORTED, who, "whole frames only (shard_world must be 1): the reconstruction reads a pixel's neighbours");
  BIND(c);
  const int w = c->ms.info.width, h = c->ms.info.height;
  const int64_t groups = (static_cast<int64_t>(w) * h + 3) / 4;      // four pixels per thread
  if (groups <= 0) return ADANERF_OK;
  hipLaunchKernelGGL(density_mask_kernel, dim3(static_cast<unsigned>((groups + 255) / 256)), dim3(256), 0, c->stream, f, w, h,
                     (reinterpret_cast<uintptr_t>(d_mask) & 3) == 0 ? 1 : 0, d_mask);
  HIP_RETURN(c, hipGetLastError());
}

int fill_density_at(adanerf_ctx* c, const char* who, const uint8_t* d_mask, int32_t width, int32_t height, int32_t phase_x, int32_t phase_y, float* d_rgb,
                    float* d_depth_map, float* d_acc_map, void* d_rgba8, int32_t* unfilled_out) {
  if (!c) return ADANERF_EINVAL;
  if (!d_mask || !d_rgb) return reject(c, ADANERF_EINVAL, who, "NULL mask or d_rgb");
  if (width < 1 || height < 1 || width > kPresentMaxSide || height > kPresentMaxSide)
    return reject(c, ADANERF_EINVAL, who, "every side must be in 1.." + std::to_string(kPresentMaxSide));
  if (phase_x < 0 || phase_x > 7 || phase_y < 0 || phase_y > 7) return reject(c, ADANERF_EINVAL, who, "phase_x and phase_y must be in 0..7");
  if (misaligned4({d_rgb, d_depth_map, d_acc_map, d_rgba8})) return reject(c, ADANERF_EINVAL, who, "fp32 and uchar4 images must be 4-byte aligned");
  const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
  const void* const img[5] = {d_mask, d_rgb, d_depth_map, d_acc_map, d_rgba8};
  const size_t img_bytes[5] = {n, n * 3 * sizeof(float), n * sizeof(float), n * sizeof(float), n * 4};
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j)
      if (img[i] && img[j] && ranges_overlap(img[i], img_bytes[i], img[j], img_bytes[j]))
        return reject(c, ADANERF_EINVAL, who, "the images overlap one another or the mask");
  BIND(c);
  int32_t* unfilled = nullptr;
  if (int rc = stage_count(c, &unfilled)) return rc;
  HIP_TRY(c, hipMemsetAsync(unfilled, 0, sizeof(int32_t), c->stream));
  const DensityFill d{d_mask, d_rgb, d_depth_map, d_acc_map, static_cast<uchar4*>(d_rgba8), unfilled};
  hipLaunchKernelGGL(density_fill_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, c->stream, d, width, height, phase_x, phase_y);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, unfilled, unfilled_out);
}

}  // namespace

extern "C" {

int adanerf_flip(adanerf_ctx* c, const float* d_test_rgb, const float* d_ref_rgb, int32_t width, int32_t height, float pixels_per_degree,
                 float* d_error_map, float* mean_out) {
  if (!c) return ADANERF_EINVAL;
  if (!d_test_rgb || !d_ref_rgb) return fail(c, ADANERF_EINVAL, "adanerf_flip: NULL image");
  if (width < 1 || height < 1) return fail(c, ADANERF_EINVAL, "adanerf_flip: width and height must be >= 1");
  if (static_cast<int64_t>(width) * height > (1ll << 30)) return fail(c, ADANERF_EINVAL, "adanerf_flip: width * height exceeds 2^30");
  const double ppd = pixels_per_degree <= 0.f ? kFlipDefaultPpd : static_cast<double>(pixels_per_degree);
  if (!(ppd >= kFlipPpdMin && ppd <= kFlipPpdMax)) {      // also a NaN; a filter is never truncated to fit
    char msg[160];
    std::snprintf(msg, sizeof(msg), "adanerf_flip: pixels_per_degree %.6g outside the supported %.0f..%.0f (<= 0 selects the reference's %.4f)",
                  ppd, kFlipPpdMin, kFlipPpdMax, kFlipDefaultPpd);
    return fail(c, ADANERF_EINVAL, msg);
  }
  BIND(c);
  return launch_flip(c, d_test_rgb, d_ref_rgb, width, height, ppd, d_error_map, mean_out);
}

int adanerf_accumulate(adanerf_ctx* c, const float* d_rgb, int32_t n_rays, float* d_sum, int32_t first) {
  return accumulate(c, "adanerf_accumulate", d_rgb, false, nullptr, 0, n_rays, d_sum, first);
}

int adanerf_accumulate_masked(adanerf_ctx* c, const float* d_rgb, const uint8_t* d_mask, uint32_t values, int32_t n_rays, float* d_sum, int32_t first) {
  return accumulate(c, "adanerf_accumulate_masked", d_rgb, true, d_mask, values, n_rays, d_sum, first);
}

int adanerf_resolve_mean(adanerf_ctx* c, const float* d_sum, int32_t n_rays, int32_t frames, void* d_rgba8, float* d_rgb) {
  return resolve_mean(c, "adanerf_resolve_mean", d_sum, false, nullptr, 0, n_rays, frames, d_rgba8, d_rgb);
}

int adanerf_resolve_mean_masked(adanerf_ctx* c, const float* d_sum, const uint8_t* d_mask, uint32_t values, int32_t n_rays, int32_t frames, void* d_rgba8,
                                float* d_rgb) {
  return resolve_mean(c, "adanerf_resolve_mean_masked", d_sum, true, d_mask, values, n_rays, frames, d_rgba8, d_rgb);
}

int adanerf_present(adanerf_ctx* c, const void* d_src_rgba8, int32_t src_w, int32_t src_h, void* d_dst_rgba8, int32_t dst_w, int32_t dst_h,
                    int32_t flags) {
  if (!c) return ADANERF_EINVAL;
  if (!d_src_rgba8 || !d_dst_rgba8) return fail(c, ADANERF_EINVAL, "adanerf_present: NULL image");
  if (src_w < 1 || src_h < 1 || dst_w < 1 || dst_h < 1 || src_w > kPresentMaxSide || src_h > kPresentMaxSide || dst_w > kPresentMaxSide ||
      dst_h > kPresentMaxSide)
    return fail(c, ADANERF_EINVAL, "adanerf_present: every side must be in 1.." + std::to_string(kPresentMaxSide));
  constexpr int32_t kFilters = ADANERF_PRESENT_NEAREST | ADANERF_PRESENT_LINEAR | ADANERF_PRESENT_AREA;
  if ((flags & ~(ADANERF_PRESENT_FLIP_Y | kFilters)) || ((flags & kFilters) & ((flags & kFilters) - 1)))
    return fail(c, ADANERF_EINVAL, "adanerf_present: flags must be ADANERF_PRESENT_FLIP_Y with at most one of _NEAREST / _LINEAR / _AREA");
  const bool area = (flags & ADANERF_PRESENT_AREA) != 0;
  if (area && (src_w > 8 * dst_w || src_h > 8 * dst_h))      // bounds the kernel's loop at 9 taps per axis
    return fail(c, ADANERF_EINVAL, "adanerf_present: ADANERF_PRESENT_AREA reduces by at most 8 per axis (reduce in two steps)");
  if (misaligned4({d_src_rgba8, d_dst_rgba8})) return fail(c, ADANERF_EINVAL, "adanerf_present: images must be 4-byte aligned (uchar4)");
  if (ranges_overlap(d_src_rgba8, static_cast<size_t>(src_w) * src_h * 4, d_dst_rgba8, static_cast<size_t>(dst_w) * dst_h * 4))
    return fail(c, ADANERF_EINVAL, "adanerf_present: source and destination overlap");
  BIND(c);
  if (area) {
    const uint64_t den_a = 2ull * static_cast<uint64_t>(src_w) * static_cast<uint64_t>(src_h);      // 2 S
    hipLaunchKernelGGL(present_area_kernel, dim3((dst_w * dst_h + 255) / 256), dim3(256), 0, c->stream, static_cast<const uchar4*>(d_src_rgba8),
                       static_cast<uchar4*>(d_dst_rgba8), src_w, src_h, dst_w, dst_h, (flags & ADANERF_PRESENT_FLIP_Y) ? 1 : 0, den_a, ~0ull / den_a);
    HIP_RETURN(c, hipGetLastError());
  }
  const bool linear = (flags & kFilters) ? (flags & ADANERF_PRESENT_LINEAR) != 0 : dst_w > src_w;      // the reference's rule
  const uint64_t den = 8ull * static_cast<uint64_t>(dst_w) * static_cast<uint64_t>(dst_h);               // 2 D E
  const int threads = (1 + (dst_w + 3) / 4) * dst_h;
  hipLaunchKernelGGL(present_kernel, dim3((threads + 255) / 256), dim3(256), 0, c->stream, static_cast<const uchar4*>(d_src_rgba8),
                     static_cast<uchar4*>(d_dst_rgba8), src_w, src_h, dst_w, dst_h, linear ? 1 : 0, (flags & ADANERF_PRESENT_FLIP_Y) ? 1 : 0,
                     static_cast<uint32_t>((reinterpret_cast<uintptr_t>(d_dst_rgba8) >> 2) & 3), den, ~0ull / den);
  HIP_RETURN(c, hipGetLastError());
}

int adanerf_reproject(adanerf_ctx* c, const void* d_src_rgba8, const float* d_src_depth_map, const float* d_src_acc_map, const float src_pos[3],
                      const float src_rot_c2w[9], const float dst_pos[3], const float dst_rot_c2w[9], float acc_min, uint32_t hole_rgba8,
                      int32_t flags, void* d_dst_rgba8, float* d_dst_depth, uint8_t* d_dst_mask, int32_t* holes_out) {
  constexpr const char* who = "adanerf_reproject";
  if (!c) return ADANERF_EINVAL;
  if (!d_src_rgba8 || !d_src_depth_map || !d_src_acc_map || !d_dst_rgba8) return reject(c, ADANERF_EINVAL, who, "NULL image");
  if (int rc = check_poses(c, who, src_pos, src_rot_c2w, dst_pos, dst_rot_c2w, true)) return rc;
  if (!(acc_min >= 0.f)) return reject(c, ADANERF_EINVAL, who, "acc_min must be >= 0");      // also a NaN; check_blend has three more rules
  if (flags & ~ADANERF_REPROJECT_FILL) return reject(c, ADANERF_EINVAL, who, "flags must be 0 or ADANERF_REPROJECT_FILL");
  const int w = c->ms.info.width, h = c->ms.info.height, n = w * h;
  if (misaligned4({d_src_rgba8, d_dst_rgba8})) return reject(c, ADANERF_EINVAL, who, "colour images must be 4-byte aligned (uchar4)");
  if (ranges_overlap(d_src_rgba8, static_cast<size_t>(n) * 4, d_dst_rgba8, static_cast<size_t>(n) * 4))      // the resolve pass reads the source colour while it writes
    return reject(c, ADANERF_EINVAL, who, "source and destination colour overlap");
  if (int rc = check_depth_frames(c, who)) return rc;
  BIND(c);
  if (int rc = grow_in_use(c, &c->stages.zbuf, static_cast<size_t>(n) * sizeof(uint64_t))) return rc;      // a warp in flight may still use the smaller z-buffer
  int32_t* holes = nullptr;
  if (int rc = stage_count(c, &holes)) return rc;
  ReprojectParams p{};
  p.g = c->ms.rg;
  copy_pose(p.g.pos, p.g.rot, src_pos, src_rot_c2w);
  copy_pose(p.dst_pos, p.dst_rot, dst_pos, dst_rot_c2w);
  p.acc_min = acc_min;
  p.origin_is_camera = c->ms.coarse_fine ? 1 : 0;      // what the render path writes to ADANERF_BUF_RAYS (camera_rays_kernel)
  unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(c->stages.zbuf.p);
  const dim3 grid((n + 255) / 256), block(256);
  hipLaunchKernelGGL(reproject_clear_kernel, grid, block, 0, c->stream, zbuf, n, holes);      // zeroes the count as well
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(reproject_splat_kernel, grid, block, 0, c->stream, p, d_src_depth_map, d_src_acc_map, zbuf);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(reproject_resolve_kernel, grid, block, 0, c->stream, zbuf, static_cast<const uint32_t*>(d_src_rgba8), w, h,
                     (flags & ADANERF_REPROJECT_FILL) ? 1 : 0, hole_rgba8, static_cast<uint32_t*>(d_dst_rgba8), d_dst_depth, d_dst_mask, holes);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, holes, holes_out);
}

int adanerf_reproject_gather(adanerf_ctx* c, const float* d_src_rgb, const float* d_src_depth_map, const float* d_src_acc_map, const float src_pos[3],
                             const float src_rot_c2w[9], const float dst_pos[3], const float dst_rot_c2w[9], float acc_min, float depth_tol,
                             int32_t iterations, uint32_t hole_rgba8, int32_t flags, float* d_dst_rgb, void* d_dst_rgba8, float* d_dst_depth,
                             uint8_t* d_dst_mask, int32_t* holes_out) {
  constexpr const char* who = "adanerf_reproject_gather";
  if (!c) return ADANERF_EINVAL;
  if (!d_src_rgb || !d_src_depth_map || !d_src_acc_map || !d_dst_rgb) return reject(c, ADANERF_EINVAL, who, "NULL image");
  if (int rc = check_poses(c, who, src_pos, src_rot_c2w, dst_pos, dst_rot_c2w, true)) return rc;
  if (!(acc_min >= 0.f)) return reject(c, ADANERF_EINVAL, who, "acc_min must be >= 0");      // every comparison also refuses a NaN
  if (!(depth_tol >= 0.f)) return reject(c, ADANERF_EINVAL, who, "depth_tol must be >= 0");
  if (iterations < 1 || iterations > kGatherMaxIterations) return reject(c, ADANERF_EINVAL, who, "iterations must lie in 1..8");
  if (flags & ~ADANERF_GATHER_GUESS) return reject(c, ADANERF_EINVAL, who, "flags must be 0 or ADANERF_GATHER_GUESS");
  if (misaligned4({d_src_rgb, d_src_depth_map, d_src_acc_map, d_dst_rgb, d_dst_rgba8, d_dst_depth}))
    return reject(c, ADANERF_EINVAL, who, "fp32 and uchar4 images must be 4-byte aligned");
  const int w = c->ms.info.width, h = c->ms.info.height, n = w * h;
  const size_t b1 = static_cast<size_t>(n) * sizeof(float);
  struct Range { const void* p; size_t bytes; };
  const Range in[3] = {{d_src_rgb, 3 * b1}, {d_src_depth_map, b1}, {d_src_acc_map, b1}};
  const Range out[4] = {{d_dst_rgb, 3 * b1}, {d_dst_rgba8, b1}, {d_dst_depth, b1}, {d_dst_mask, static_cast<size_t>(n)}};
  for (int a = 0; a < 4; ++a) {      // both passes read the sources while the second writes; no output may be another's or a source's bytes
    if (!out[a].p) continue;
    for (const Range& r : in)
      if (ranges_overlap(out[a].p, out[a].bytes, r.p, r.bytes)) return reject(c, ADANERF_EINVAL, who, "an output overlaps a source image");
    for (int b = a + 1; b < 4; ++b)
      if (out[b].p && ranges_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) return reject(c, ADANERF_EINVAL, who, "two outputs overlap");
  }
  if (int rc = check_depth_frames(c, who)) return rc;
  BIND(c);
  if (int rc = grow_in_use(c, &c->stages.gather_surface, static_cast<size_t>(n) * sizeof(float4))) return rc;      // a warp in flight may still use the smaller table
  int32_t* holes = nullptr;
  if (int rc = stage_count(c, &holes)) return rc;
  GatherSurfaceParams ps{};
  ps.g = c->ms.rg;
  copy_pose(ps.g.pos, ps.g.rot, src_pos, src_rot_c2w);
  ps.acc_min = acc_min;
  ps.origin_is_camera = c->ms.coarse_fine ? 1 : 0;      // what the render path writes to ADANERF_BUF_RAYS (camera_rays_kernel)
  GatherWarpParams pw{};
  pw.g = c->ms.rg;
  copy_pose(pw.g.pos, pw.g.rot, dst_pos, dst_rot_c2w);
  copy_pose(pw.src_pos, pw.src_rot, src_pos, src_rot_c2w);
  pw.depth_tol = depth_tol;
  pw.iterations = iterations;
  pw.guess = (flags & ADANERF_GATHER_GUESS) ? 1 : 0;
  pw.hole_rgba8 = hole_rgba8;
  float4* surface = reinterpret_cast<float4*>(c->stages.gather_surface.p);
  HIP_TRY(c, hipMemsetAsync(holes, 0, sizeof(int32_t), c->stream));
  hipLaunchKernelGGL(gather_surface_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, ps, d_src_depth_map, d_src_acc_map, surface);
  HIP_TRY(c, hipGetLastError());
  const dim3 grid((w + kGatherTileW - 1) / kGatherTileW, (h + kGatherTileH - 1) / kGatherTileH);
  hipLaunchKernelGGL(gather_warp_kernel, grid, dim3(256), 0, c->stream, pw, surface, d_src_rgb, d_dst_rgb, static_cast<uchar4*>(d_dst_rgba8), d_dst_depth,
                     d_dst_mask, holes);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, holes, holes_out);
}

int adanerf_reproject_pair(adanerf_ctx* c, const float* d_a_rgb, const float* d_a_depth_map, const float* d_a_acc_map, const float a_pos[3],
                           const float a_rot_c2w[9], const float* d_b_rgb, const float* d_b_depth_map, const float* d_b_acc_map, const float b_pos[3],
                           const float b_rot_c2w[9], const float dst_pos[3], const float dst_rot_c2w[9], float weight_b, float acc_min, float depth_tol,
                           uint32_t hole_rgba8, int32_t flags, float* d_dst_rgb, void* d_dst_rgba8, float* d_dst_depth, uint8_t* d_dst_mask,
                           uint8_t* d_dst_source, int32_t* holes_out) {
  constexpr const char* who = "adanerf_reproject_pair";
  if (!c) return ADANERF_EINVAL;
  if (!d_a_rgb || !d_a_depth_map || !d_a_acc_map || !d_b_rgb || !d_b_depth_map || !d_b_acc_map || !d_dst_rgb) return reject(c, ADANERF_EINVAL, who, "NULL image");
  if (int rc = check_poses(c, who, a_pos, a_rot_c2w, b_pos, b_rot_c2w, true)) return rc;
  if (int rc = check_poses(c, who, dst_pos, dst_rot_c2w, nullptr, nullptr, false)) return rc;
  if (!(weight_b >= 0.f && weight_b <= 1.f)) return reject(c, ADANERF_EINVAL, who, "weight_b must lie in [0, 1]");      // every comparison also refuses a NaN
  if (!(acc_min >= 0.f)) return reject(c, ADANERF_EINVAL, who, "acc_min must be >= 0");
  if (!(depth_tol >= 0.f)) return reject(c, ADANERF_EINVAL, who, "depth_tol must be >= 0");
  if (flags & ~ADANERF_REPROJECT_FILL) return reject(c, ADANERF_EINVAL, who, "flags must be 0 or ADANERF_REPROJECT_FILL");
  if (misaligned4({d_a_rgb, d_a_depth_map, d_a_acc_map, d_b_rgb, d_b_depth_map, d_b_acc_map, d_dst_rgb, d_dst_rgba8, d_dst_depth}))
    return reject(c, ADANERF_EINVAL, who, "fp32 and uchar4 images must be 4-byte aligned");
  const int w = c->ms.info.width, h = c->ms.info.height, n = w * h;
  const size_t b1 = static_cast<size_t>(n) * sizeof(float);
  struct Range { const void* p; size_t bytes; };
  const Range in[6] = {{d_a_rgb, 3 * b1}, {d_a_depth_map, b1}, {d_a_acc_map, b1}, {d_b_rgb, 3 * b1}, {d_b_depth_map, b1}, {d_b_acc_map, b1}};
  const Range out[5] = {{d_dst_rgb, 3 * b1}, {d_dst_rgba8, b1}, {d_dst_depth, b1}, {d_dst_mask, static_cast<size_t>(n)}, {d_dst_source, static_cast<size_t>(n)}};
  for (int a = 0; a < 5; ++a) {      // the resolve reads both sources' colour while it writes; A and B may be the same images
    if (!out[a].p) continue;
    for (const Range& r : in)
      if (ranges_overlap(out[a].p, out[a].bytes, r.p, r.bytes)) return reject(c, ADANERF_EINVAL, who, "an output overlaps a source image");
    for (int b = a + 1; b < 5; ++b)
      if (out[b].p && ranges_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) return reject(c, ADANERF_EINVAL, who, "two outputs overlap");
  }
  if (int rc = check_depth_frames(c, who)) return rc;
  BIND(c);
  if (int rc = grow_in_use(c, &c->stages.zbuf, static_cast<size_t>(n) * 2 * sizeof(uint64_t))) return rc;      // adanerf_reproject's scratch: its z-buffer, and a second behind it
  int32_t* holes = nullptr;
  if (int rc = stage_count(c, &holes)) return rc;
  PairSplatParams ps{};
  const float* const pos[2] = {a_pos, b_pos};
  const float* const rot[2] = {a_rot_c2w, b_rot_c2w};
  for (int s = 0; s < 2; ++s) {
    ps.s[s].g = c->ms.rg;
    copy_pose(ps.s[s].g.pos, ps.s[s].g.rot, pos[s], rot[s]);
    copy_pose(ps.s[s].dst_pos, ps.s[s].dst_rot, dst_pos, dst_rot_c2w);
    ps.s[s].acc_min = acc_min;
    ps.s[s].origin_is_camera = c->ms.coarse_fine ? 1 : 0;      // what the render path writes to ADANERF_BUF_RAYS (camera_rays_kernel)
  }
  ps.depth[0] = d_a_depth_map;
  ps.depth[1] = d_b_depth_map;
  ps.acc[0] = d_a_acc_map;
  ps.acc[1] = d_b_acc_map;
  const PairResolveParams pr{{d_a_rgb, d_b_rgb}, w, h, (flags & ADANERF_REPROJECT_FILL) ? 1 : 0, weight_b, depth_tol, hole_rgba8};
  unsigned long long* zbuf = reinterpret_cast<unsigned long long*>(c->stages.zbuf.p);
  const unsigned blocks = static_cast<unsigned>((n + 255) / 256);
  hipLaunchKernelGGL(reproject_clear_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, c->stream, zbuf, 2 * n, holes);      // both z-buffers; zeroes the count as well
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(reproject_pair_splat_kernel, dim3(blocks, 2), dim3(256), 0, c->stream, ps, zbuf);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(reproject_pair_resolve_kernel, dim3(blocks), dim3(256), 0, c->stream, pr, zbuf, d_dst_rgb, static_cast<uchar4*>(d_dst_rgba8), d_dst_depth,
                     d_dst_mask, d_dst_source, holes);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, holes, holes_out);
}

int adanerf_temporal_resolve(adanerf_ctx* c, const float* d_cur_rgb, const float* d_cur_depth_map, const float* d_cur_acc_map, const float cur_pos[3],
                             const float cur_rot_c2w[9], const float* d_hist_rgb, const float* d_hist_depth, const uint8_t* d_hist_count,
                             const float prev_pos[3], const float prev_rot_c2w[9], float alpha, float depth_tol, float acc_min, int32_t flags,
                             float* d_out_rgb, float* d_out_depth, uint8_t* d_out_count, void* d_out_rgba8, uint8_t* d_out_mask,
                             int32_t* rejected_out) {
  constexpr const char* who = "adanerf_temporal_resolve";
  if (!c) return ADANERF_EINVAL;
  if (!d_cur_rgb || !d_cur_depth_map || !d_cur_acc_map || !d_out_rgb) return reject(c, ADANERF_EINVAL, who, "NULL image");
  if (int rc = check_poses(c, who, cur_pos, cur_rot_c2w, prev_pos, prev_rot_c2w, d_hist_rgb != nullptr)) return rc;
  if (int rc = check_blend(c, who, alpha, depth_tol, acc_min, flags)) return rc;
  if (misaligned4({d_cur_rgb, d_cur_depth_map, d_cur_acc_map, d_hist_rgb, d_hist_depth, d_out_rgb, d_out_depth, d_out_rgba8}))
    return reject(c, ADANERF_EINVAL, who, "fp32 and uchar4 images must be 4-byte aligned");
  const int w = c->ms.info.width, h = c->ms.info.height, n = w * h;
  const size_t b3 = static_cast<size_t>(n) * 3 * sizeof(float), b1 = static_cast<size_t>(n) * sizeof(float);
  if ((d_hist_rgb && ranges_overlap(d_out_rgb, b3, d_hist_rgb, b3)) || ranges_overlap(d_out_rgb, b3, d_cur_rgb, b3) ||
      (d_out_depth && d_hist_depth && ranges_overlap(d_out_depth, b1, d_hist_depth, b1)) ||
      (d_out_count && d_hist_count && ranges_overlap(d_out_count, static_cast<size_t>(n), d_hist_count, static_cast<size_t>(n))))
    return reject(c, ADANERF_EINVAL, who, "an output overlaps the image it is gathered from (the history is ping-ponged, not updated in place)");
  if (int rc = check_depth_frames(c, who)) return rc;
  BIND(c);
  int32_t* rejected = nullptr;
  if (int rc = stage_count(c, &rejected)) return rc;
  const TemporalParams p = temporal_params(c, cur_pos, cur_rot_c2w, d_hist_rgb != nullptr, prev_pos, prev_rot_c2w, alpha, depth_tol, acc_min, flags);
  HIP_TRY(c, hipMemsetAsync(rejected, 0, sizeof(int32_t), c->stream));
  const dim3 grid((w + kTemporalTileW - 1) / kTemporalTileW, (h + kTemporalTileH - 1) / kTemporalTileH), block(256);
  hipLaunchKernelGGL(temporal_resolve_kernel, grid, block, 0, c->stream, p, d_cur_rgb, d_cur_depth_map, d_cur_acc_map, d_hist_rgb, d_hist_depth, d_hist_count, d_out_rgb,
                     d_out_depth, d_out_count, static_cast<uchar4*>(d_out_rgba8), d_out_mask, rejected);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, rejected, rejected_out);
}

int adanerf_temporal_upsample(adanerf_ctx* c, int32_t scale, const float* d_cur_rgb, const float* d_cur_depth_map, const float* d_cur_acc_map, float cur_dx,
                              float cur_dy, const float cur_pos[3], const float cur_rot_c2w[9], const float* d_hist_rgb, const float* d_hist_depth,
                              const uint8_t* d_hist_count, const float prev_pos[3], const float prev_rot_c2w[9], float alpha, float depth_tol,
                              float acc_min, int32_t flags, float* d_out_rgb, float* d_out_depth, uint8_t* d_out_count, void* d_out_rgba8,
                              uint8_t* d_out_mask, int32_t* rejected_out) {
  constexpr const char* who = "adanerf_temporal_upsample";
  if (!c) return ADANERF_EINVAL;
  if (!d_cur_rgb || !d_cur_depth_map || !d_cur_acc_map || !d_out_rgb) return reject(c, ADANERF_EINVAL, who, "NULL image");
  if (int rc = check_poses(c, who, cur_pos, cur_rot_c2w, prev_pos, prev_rot_c2w, d_hist_rgb != nullptr)) return rc;
  if (scale < 1 || scale > kUpsampleMaxScale) return reject(c, ADANERF_EINVAL, who, "scale must lie in 1..4");
  if (!(std::fabs(cur_dx) <= 1.f && std::fabs(cur_dy) <= 1.f))      // also a NaN
    return reject(c, ADANERF_EINVAL, who, "the pixel offset must lie in [-1, 1] on both axes");
  if (int rc = check_blend(c, who, alpha, depth_tol, acc_min, flags)) return rc;
  if (misaligned4({d_cur_rgb, d_cur_depth_map, d_cur_acc_map, d_hist_rgb, d_hist_depth, d_out_rgb, d_out_depth, d_out_rgba8}))
    return reject(c, ADANERF_EINVAL, who, "fp32 and uchar4 images must be 4-byte aligned");
  const int w = c->ms.info.width, h = c->ms.info.height, n = w * h;
  const int64_t N64 = static_cast<int64_t>(n) * scale * scale;
  if (N64 >= (1ll << 25)) return reject(c, ADANERF_EINVAL, who, "the output's width*height must be < 2^25");
  const int W = w * scale, H = h * scale;
  const size_t N = static_cast<size_t>(N64), sf = sizeof(float);
  if ((d_hist_rgb && ranges_overlap(d_out_rgb, N * 3 * sf, d_hist_rgb, N * 3 * sf)) || ranges_overlap(d_out_rgb, N * 3 * sf, d_cur_rgb, n * 3 * sf) ||
      (d_out_depth && ((d_hist_depth && ranges_overlap(d_out_depth, N * sf, d_hist_depth, N * sf)) || ranges_overlap(d_out_depth, N * sf, d_cur_depth_map, n * sf) ||
                       ranges_overlap(d_out_depth, N * sf, d_cur_acc_map, n * sf))) ||
      (d_out_count && d_hist_count && ranges_overlap(d_out_count, N, d_hist_count, N)))
    return reject(c, ADANERF_EINVAL, who, "an output overlaps the image it is gathered from (the history is ping-ponged, not updated in place)");
  if (int rc = check_depth_frames(c, who)) return rc;
  BIND(c);
  int32_t* rejected = nullptr;
  if (int rc = stage_count(c, &rejected)) return rc;
  const bool depth_test = d_hist_rgb && d_hist_depth;
  if (int rc = depth_test ? grow_in_use(c, &c->stages.upsample_zp, static_cast<size_t>(n) * sf) : 0) return rc;
  UpsampleParams p{};
  p.g_lo = with_pixel_offset(c->ms.rg, cur_dx, cur_dy);      // the offset handed in, never the context's own
  p.g_hi = c->ms.rg;
  ray_geometry(c->ms.cfg.fov, W, H, c->ms.rg.strip_rows, 1, 0, &p.g_hi);      // what frame_geometry yields for (W, H); its focal as fp32 is read in the kernel
  copy_pose(p.g_lo.pos, p.g_lo.rot, cur_pos, cur_rot_c2w);
  copy_pose(p.g_hi.pos, p.g_hi.rot, cur_pos, cur_rot_c2w);
  if (d_hist_rgb) copy_pose(p.prev_pos, p.prev_rot, prev_pos, prev_rot_c2w);
  p.alpha = alpha;
  p.depth_tol = depth_tol;
  p.acc_min = acc_min;
  p.cur_dx = cur_dx;
  p.cur_dy = cur_dy;
  p.scale = scale;
  p.origin_is_camera = c->ms.coarse_fine ? 1 : 0;
  p.clamp = (flags & ADANERF_TEMPORAL_CLAMP) ? 1 : 0;
  float* zp = reinterpret_cast<float*>(c->stages.upsample_zp.p);
  HIP_TRY(c, hipMemsetAsync(rejected, 0, sizeof(int32_t), c->stream));
  if (depth_test) {
    hipLaunchKernelGGL(upsample_depth_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, p, d_cur_depth_map, d_cur_acc_map, zp);
    HIP_TRY(c, hipGetLastError());
  }
  const dim3 grid((W + kTemporalTileW - 1) / kTemporalTileW, (H + kTemporalTileH - 1) / kTemporalTileH), block(256);
  hipLaunchKernelGGL(upsample_resolve_kernel, grid, block, 0, c->stream, p, d_cur_rgb, d_cur_depth_map, d_cur_acc_map, zp, d_hist_rgb, d_hist_depth, d_hist_count,
                     d_out_rgb, d_out_depth, d_out_count, static_cast<uchar4*>(d_out_rgba8), d_out_mask, rejected);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, rejected, rejected_out);
}

int adanerf_temporal_resolve_sparse(adanerf_ctx* c, const uint8_t* d_mask, int32_t phase_x, int32_t phase_y, const float* d_cur_rgb, const float* d_cur_depth_map,
                                    const float* d_cur_acc_map, const float cur_pos[3], const float cur_rot_c2w[9], const float* d_hist_rgb,
                                    const float* d_hist_depth, const uint8_t* d_hist_count, const float prev_pos[3], const float prev_rot_c2w[9], float alpha,
                                    float depth_tol, float acc_min, int32_t flags, float* d_out_rgb, float* d_out_depth, uint8_t* d_out_count, void* d_out_rgba8,
                                    uint8_t* d_out_mask, int32_t* rejected_out) {
  constexpr const char* who = "adanerf_temporal_resolve_sparse";
  if (!c) return ADANERF_EINVAL;
  if (!d_mask) return reject(c, ADANERF_EINVAL, who, "NULL mask");
  if (!d_cur_rgb || !d_cur_depth_map || !d_cur_acc_map || !d_out_rgb) return reject(c, ADANERF_EINVAL, who, "NULL image");
  if (!d_out_count) return reject(c, ADANERF_EINVAL, who, "NULL d_out_count (without a count a placeholder cannot be told from a sample)");
  if (d_hist_rgb && !d_hist_count) return reject(c, ADANERF_EINVAL, who, "a history needs its count");
  if (phase_x < 0 || phase_x > 7 || phase_y < 0 || phase_y > 7) return reject(c, ADANERF_EINVAL, who, "phase_x and phase_y must be in 0..7");
  if (int rc = check_poses(c, who, cur_pos, cur_rot_c2w, prev_pos, prev_rot_c2w, d_hist_rgb != nullptr)) return rc;
  if (int rc = check_blend(c, who, alpha, depth_tol, acc_min, flags)) return rc;
  if (misaligned4({d_cur_rgb, d_cur_depth_map, d_cur_acc_map, d_hist_rgb, d_hist_depth, d_out_rgb, d_out_depth, d_out_rgba8}))
    return reject(c, ADANERF_EINVAL, who, "fp32 and uchar4 images must be 4-byte aligned");
  const int w = c->ms.info.width, h = c->ms.info.height, n = w * h;
  const size_t n1 = static_cast<size_t>(n), b3 = n1 * 3 * sizeof(float), b1 = n1 * sizeof(float);
  if ((d_hist_rgb && ranges_overlap(d_out_rgb, b3, d_hist_rgb, b3)) || ranges_overlap(d_out_rgb, b3, d_cur_rgb, b3) ||
      (d_out_depth && d_hist_depth && ranges_overlap(d_out_depth, b1, d_hist_depth, b1)) ||
      (d_hist_count && ranges_overlap(d_out_count, n1, d_hist_count, n1)))
    return reject(c, ADANERF_EINVAL, who, "an output overlaps the image it is gathered from (the history is ping-ponged, not updated in place)");
  if (ranges_overlap(d_mask, n1, d_out_rgb, b3) || (d_out_depth && ranges_overlap(d_mask, n1, d_out_depth, b1)) || ranges_overlap(d_mask, n1, d_out_count, n1) ||
      (d_out_rgba8 && ranges_overlap(d_mask, n1, d_out_rgba8, b1)) || (d_out_mask && ranges_overlap(d_mask, n1, d_out_mask, n1)))
    return reject(c, ADANERF_EINVAL, who, "the mask overlaps an output (a reconstructed pixel reads the bytes of its cell)");
  if (int rc = check_depth_frames(c, who)) return rc;
  BIND(c);
  int32_t* rejected = nullptr;
  if (int rc = stage_count(c, &rejected)) return rc;
  const bool depth_test = d_hist_rgb && d_hist_depth;
  if (int rc = depth_test ? grow_in_use(c, &c->stages.upsample_zp, b1) : 0) return rc;      // the scratch adanerf_temporal_upsample keeps its pass A in
  const TemporalParams p = temporal_params(c, cur_pos, cur_rot_c2w, d_hist_rgb != nullptr, prev_pos, prev_rot_c2w, alpha, depth_tol, acc_min, flags);
  UpsampleParams a{};      // pass A is adanerf_temporal_upsample's with the same generator and poses; it reads nothing else of g_hi
  a.g_lo = p.g;
  copy_pose(a.prev_pos, a.prev_rot, p.prev_pos, p.prev_rot);
  a.acc_min = acc_min;
  a.origin_is_camera = p.origin_is_camera;
  float* zp = reinterpret_cast<float*>(c->stages.upsample_zp.p);
  HIP_TRY(c, hipMemsetAsync(rejected, 0, sizeof(int32_t), c->stream));
  if (depth_test) {
    hipLaunchKernelGGL(upsample_depth_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, a, d_cur_depth_map, d_cur_acc_map, zp);
    HIP_TRY(c, hipGetLastError());
  }
  const dim3 grid((w + kTemporalTileW - 1) / kTemporalTileW, (h + kTemporalTileH - 1) / kTemporalTileH), block(256);
  hipLaunchKernelGGL(sparse_resolve_kernel, grid, block, 0, c->stream, p, phase_x, phase_y, d_mask, d_cur_rgb, d_cur_depth_map, d_cur_acc_map, zp, d_hist_rgb,
                     d_hist_depth, d_hist_count, d_out_rgb, d_out_depth, d_out_count, static_cast<uchar4*>(d_out_rgba8), d_out_mask, rejected);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, rejected, rejected_out);
}

int adanerf_blend_behind(adanerf_ctx* c, const float* d_rgb, const float* d_acc, const float* d_behind_rgb, int32_t n, float* d_out_rgb, void* d_out_rgba8) {
  if (!c) return ADANERF_EINVAL;
  if (!d_rgb || !d_acc || !d_behind_rgb) return fail(c, ADANERF_EINVAL, "adanerf_blend_behind: NULL input image");
  if (!d_out_rgb && !d_out_rgba8) return fail(c, ADANERF_EINVAL, "adanerf_blend_behind: both outputs NULL");
  if (n < 0 || n > 0x7fffffff / 3) return fail(c, ADANERF_EINVAL, "adanerf_blend_behind: n must be >= 0 and n * 3 <= 2^31 - 1");
  if (misaligned4({d_rgb, d_acc, d_behind_rgb, d_out_rgb, d_out_rgba8})) return fail(c, ADANERF_EINVAL, "adanerf_blend_behind: images must be 4-byte aligned");
  const size_t bytes = static_cast<size_t>(n) * 3 * sizeof(float), bytes1 = static_cast<size_t>(n) * 4;
  const void* const in[3] = {d_rgb, d_acc, d_behind_rgb};
  const size_t in_bytes[3] = {bytes, bytes1, bytes};
  for (int i = 0; i < 3; ++i) {
    if (d_out_rgb && !(i == 0 && d_out_rgb == d_rgb) && ranges_overlap(in[i], in_bytes[i], d_out_rgb, bytes))
      return fail(c, ADANERF_EINVAL, "adanerf_blend_behind: d_out_rgb overlaps an input (only d_rgb itself may be the output)");
    if (d_out_rgba8 && ranges_overlap(in[i], in_bytes[i], d_out_rgba8, bytes1)) return fail(c, ADANERF_EINVAL, "adanerf_blend_behind: d_out_rgba8 overlaps an input");
  }
  if (d_out_rgb && d_out_rgba8 && ranges_overlap(d_out_rgb, bytes, d_out_rgba8, bytes1)) return fail(c, ADANERF_EINVAL, "adanerf_blend_behind: the two outputs overlap");
  BIND(c);
  if (n == 0) return ADANERF_OK;
  hipLaunchKernelGGL(blend_behind_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_rgb, d_acc, d_behind_rgb, n, d_out_rgb, static_cast<uchar4*>(d_out_rgba8));
  HIP_RETURN(c, hipGetLastError());
}

int adanerf_foveate_density(adanerf_ctx* c, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride, uint8_t* d_mask) {
  return foveate_density_at(c, "adanerf_foveate_density", gaze_x, gaze_y, n_rings, radius_px, stride, 0, 0, d_mask);
}

int adanerf_foveate_density_phased(adanerf_ctx* c, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride, int32_t phase_x,
                                   int32_t phase_y, uint8_t* d_mask) {
  return foveate_density_at(c, "adanerf_foveate_density_phased", gaze_x, gaze_y, n_rings, radius_px, stride, phase_x, phase_y, d_mask);
}

int adanerf_fill_density(adanerf_ctx* c, const uint8_t* d_mask, int32_t width, int32_t height, float* d_rgb, float* d_depth_map, float* d_acc_map, void* d_rgba8,
                         int32_t* unfilled_out) {
  return fill_density_at(c, "adanerf_fill_density", d_mask, width, height, 0, 0, d_rgb, d_depth_map, d_acc_map, d_rgba8, unfilled_out);
}

int adanerf_fill_density_phased(adanerf_ctx* c, const uint8_t* d_mask, int32_t width, int32_t height, int32_t phase_x, int32_t phase_y, float* d_rgb,
                                float* d_depth_map, float* d_acc_map, void* d_rgba8, int32_t* unfilled_out) {
  return fill_density_at(c, "adanerf_fill_density_phased", d_mask, width, height, phase_x, phase_y, d_rgb, d_depth_map, d_acc_map, d_rgba8, unfilled_out);
}

int adanerf_contrast_mask(adanerf_ctx* c, const float* d_rgb, int32_t width, int32_t height, float threshold, uint8_t* d_mask, int32_t* n_flagged) {
  if (!c) return ADANERF_EINVAL;
  if (!d_rgb || !d_mask) return fail(c, ADANERF_EINVAL, "adanerf_contrast_mask: NULL image or mask");
  if (const char* why = contrast_rule_check(width, height, threshold)) return fail(c, ADANERF_EINVAL, std::string("adanerf_contrast_mask: ") + why);
  if (misaligned4({d_rgb})) return fail(c, ADANERF_EINVAL, "adanerf_contrast_mask: d_rgb must be 4-byte aligned");
  const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
  if (ranges_overlap(d_rgb, n * 3 * sizeof(float), d_mask, n)) return fail(c, ADANERF_EINVAL, "adanerf_contrast_mask: the mask overlaps the image");
  BIND(c);
  int32_t* flagged = nullptr;
  if (int rc = stage_count(c, &flagged)) return rc;
  if (n_flagged) HIP_TRY(c, hipMemsetAsync(flagged, 0, sizeof(int32_t), c->stream));      // counted only when the caller asks
  const dim3 grid(static_cast<unsigned>((width + kContrastTileW - 1) / kContrastTileW), static_cast<unsigned>((height + kContrastTileH - 1) / kContrastTileH));
  hipLaunchKernelGGL(contrast_mask_kernel, grid, dim3(256), 0, c->stream, d_rgb, width, height, threshold, d_mask, n_flagged ? flagged : nullptr);
  HIP_TRY(c, hipGetLastError());
  return read_count(c, flagged, n_flagged);
}

}  // extern "C"
