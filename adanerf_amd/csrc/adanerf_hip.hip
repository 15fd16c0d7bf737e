// C ABI of libadanerf_hip.so (see include/adanerf_hip.h).  Host side of the render path: the context (context.hpp), weight upload, buffer ownership,
// every launcher of the 16-bit kernels and the per-frame launch sequence on the context's own HIP stream.  The entry points that work on finished
// images live in stages.hip; the device-free parts in model_setup.cpp, guard_record.cpp and flip_tables.cpp; the fp32-MFMA kernels in launch_f32.hip.
#include "context.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <string>
#include <vector>

#include "guard_record.hpp"
#include "kernels.hip.hpp"
#include "launch_f32.hpp"
#include "k_generic_f32.hip.hpp"   // (the kernels themselves live in launch_f32.hip)
#include "k_generic16.hip.hpp"     // the 16-bit form of the run-time-shaped shading kernel

using namespace adanerf;

namespace adanerf {      // declared in context.hpp: stages.hip calls them too

int fail(adanerf_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  else g_create_error = msg;
  return code;
}

int hip_rc(adanerf_ctx* c, hipError_t e, const char* what) {
  return e == hipSuccess ? ADANERF_OK : fail(c, ADANERF_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

int dev_alloc(adanerf_ctx* c, DevBuf* b, size_t bytes) {
  if (b->bytes >= bytes && b->p) return ADANERF_OK;
  void* grown = nullptr;      // before the old one goes: a failed growth leaves the buffer usable
  if (bytes) HIP_TRY(c, hipMalloc(&grown, bytes));
  if (b->p) HIP_TRY(c, hipFree(b->p));
  b->p = grown;
  b->bytes = bytes;
  return ADANERF_OK;
}

}  // namespace adanerf

namespace {

// int32 slots of the `total` block (64 B on the device, imaged to pinned memory after every recorded batch): samples of the batch, rays
// re-evaluated by the guarded selection, its monitor (SelectOut::guard_seen: kGuardSeenSlots running values, indexed by kSeen*)
enum { kTotalSamples = 0, kTotalRefined = 4, kTotalGuardSeen = 8, kTotalSlots = 16 };
enum { kSeenMax = 0, kSeenViolations = 1, kSeenPair = 2, kSeenAuditMismatch = 3, kSeenAudited = 4, kGuardSeenSlots = 5 };

constexpr const char* kOccupancyQuery = "hipOccupancyMaxActiveBlocksPerMultiprocessor";      // where launch_persistent() can fail

int upload_net(adanerf_ctx* c, const PackedNet& pn, PackedDev* d) {
  int rc;
  if ((rc = dev_alloc(c, &d->w, pn.weights.size()))) return rc;
  if ((rc = dev_alloc(c, &d->b, pn.bias.size() * sizeof(float)))) return rc;
  HIP_TRY(c, hipMemcpy(d->w.p, pn.weights.data(), pn.weights.size(), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(d->b.p, pn.bias.data(), pn.bias.size() * sizeof(float), hipMemcpyHostToDevice));
  d->params.w = reinterpret_cast<const u32x4*>(d->w.p);
  d->params.bias = reinterpret_cast<const float*>(d->b.p);
  for (size_t i = 0; i < pn.w_off.size() && i < kMaxLayers; ++i) {
    d->params.w_off[i] = pn.w_off[i];
    d->params.b_off[i] = pn.b_off[i];
  }
  d->params.n_bias = static_cast<uint32_t>(pn.bias.size());
  d->params.out_scale[0] = std::ldexp(1.0f, pn.out_exp[0]);      // 1 unless the bf16 packing scaled the layers (pack.cpp scale_layer)
  d->params.out_scale[1] = std::ldexp(1.0f, pn.out_exp[1]);
  return ADANERF_OK;
}

// the shading net packed for `prec`, on first use; coarse: model0.onnx of a coarse/fine directory, a NeRF net with the encoding posEncArgs[0]
int ensure_shading_net(adanerf_ctx* c, int prec, bool coarse) {
  if (prec < 0 || prec > 2) return fail(c, ADANERF_EINVAL, "precision must be ADANERF_PREC_{BF16,FP16,FP32}");
  PackedDev& dev = coarse ? c->netc[prec] : c->net1[prec];
  if (dev.w.p) return ADANERF_OK;
  PackedNet pn;
  std::string err;
  const NetShape sh = coarse ? shape_of(c->ms.fp0, c->ms.fd0, c->ms.fp0, c->ms.fd0, 0, false)
                             : shape_of(c->ms.fp0, c->ms.fd0, c->ms.fp1, c->ms.fd1, c->ms.ray_samples, !c->ms.coarse_fine);
  if (!pack_shading_net(coarse ? c->net0_host : c->net1_host, sh, elem_of(prec), &pn, &err))
    return fail(c, ADANERF_EIO, (coarse ? "model0.onnx: " : "model1.onnx: ") + err);
  return upload_net(c, pn, &dev);
}

int ensure_batch_buffers(adanerf_ctx* c, int n_rays, int n_max) {
  if (n_rays <= c->cap_rays && n_max <= c->cap_nmax) return ADANERF_OK;
  n_rays = std::max(n_rays, c->cap_rays);
  n_max = std::max(n_max, c->cap_nmax);
  if (c->cap_rays > 0) HIP_TRY(c, hipStreamSynchronize(c->stream));      // growth frees buffers that enqueued frames may still use
  const size_t R = static_cast<size_t>(n_rays), S = R * static_cast<size_t>(n_max);
  const size_t nblk = (R + 31) / 32;     // segment totals: per 64 rays (select_kernel) or per 32 (pair selection)
  int rc;
  if ((rc = dev_alloc(c, &c->rays, R * 8 * sizeof(float)))) return rc;
  if ((rc = dev_alloc(c, &c->ray_offsets, R * sizeof(int32_t)))) return rc;
  if ((rc = dev_alloc(c, &c->ray_counts, R * sizeof(int32_t)))) return rc;
  if (c->ms.coarse_fine) {      // no oracle values, no selection scratch; the coarse pass has its own keys and raw outputs
    const size_t Sc = R * static_cast<size_t>(c->ms.n_coarse);
    if ((rc = dev_alloc(c, &c->key_coarse, Sc * sizeof(uint32_t)))) return rc;
    if ((rc = dev_alloc(c, &c->raw_coarse, Sc * 4 * sizeof(float)))) return rc;
    if ((rc = dev_alloc(c, &c->sample_z, S * sizeof(float)))) return rc;
  } else {
    if ((rc = dev_alloc(c, &c->oracle, R * kBins * sizeof(float)))) return rc;
    if ((rc = dev_alloc(c, &c->selbin, S))) return rc;
    if ((rc = dev_alloc(c, &c->selw, S * sizeof(float)))) return rc;
    if (c->sampling_mode == ADANERF_SAMPLING_GUARDED) {
      if ((rc = dev_alloc(c, &c->guard_mask, nblk * sizeof(uint32_t)))) return rc;
      if ((rc = dev_alloc(c, &c->refine_list, R * sizeof(int32_t)))) return rc;
      if ((rc = dev_alloc(c, &c->guard_probe, R * 2 * sizeof(float)))) return rc;
    }
  }
  if ((rc = dev_alloc(c, &c->block_total, nblk * sizeof(int32_t)))) return rc;
  if ((rc = dev_alloc(c, &c->block_offset, nblk * sizeof(int32_t)))) return rc;
  if (!c->total.p) {
    if ((rc = dev_alloc(c, &c->total, kTotalSlots * sizeof(int32_t)))) return rc;
    HIP_TRY(c, hipMemset(c->total.p, 0, kTotalSlots * sizeof(int32_t)));
  }
  if ((rc = dev_alloc(c, &c->sample_key, S * sizeof(uint32_t)))) return rc;
  if ((rc = dev_alloc(c, &c->sample_w, S * sizeof(float)))) return rc;
  if ((rc = dev_alloc(c, &c->raw, S * 4 * sizeof(float)))) return rc;
  if (c->ms.info.sampler_mode == ADANERF_SAMPLER_PDF && (rc = dev_alloc(c, &c->sample_z, S * sizeof(float)))) return rc;
  c->cap_rays = n_rays;
  c->cap_nmax = n_max;
  return ADANERF_OK;
}

// Scratch of the selection / compaction stage only.  The stage entry point adanerf_compact must not re-allocate the
// per-batch buffers: a caller may hold pointers from adanerf_get_buffer (e.g. pass the context's own oracle buffer).
int ensure_compact_scratch(adanerf_ctx* c, int n_rays, int n_max) {
  const size_t R = static_cast<size_t>(std::max(n_rays, 1)), S = R * static_cast<size_t>(n_max);
  const size_t nblk = (R + 31) / 32;
  int rc;
  if (c->selbin.bytes < S || c->selw.bytes < S * sizeof(float) || c->block_total.bytes < nblk * sizeof(int32_t) ||
      c->block_offset.bytes < nblk * sizeof(int32_t)) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // a previous launch may still use the old scratch
    if ((rc = dev_alloc(c, &c->selbin, S))) return rc;
    if ((rc = dev_alloc(c, &c->selw, S * sizeof(float)))) return rc;
    if ((rc = dev_alloc(c, &c->block_total, nblk * sizeof(int32_t)))) return rc;
    if ((rc = dev_alloc(c, &c->block_offset, nblk * sizeof(int32_t)))) return rc;
  }
  return ADANERF_OK;
}

// ---- launches ------------------------------------------------------------------------------

int ensure_guard_band(adanerf_ctx* c);

// the sampling net has a split-precision packing: not with raySampleInput on the run-time-shaped kernels, not above width 256 (pack.cpp)
bool has_split_sampling(const adanerf_ctx* c) { return (!c->generic0 || c->ms.ray_samples == 0) && c->topo0.width != kWideWidth; }

// a sampling net of another topology / layout on the split-precision run-time-shaped kernel (else: the fp32 one)
bool generic_split_sampling(const adanerf_ctx* c) {
  return c->generic0 && c->sampling_mode != ADANERF_SAMPLING_FP32 && c->ms.ray_samples == 0 && c->net0_split.w.p != nullptr;
}

// The ray generator in force: ms.rg with the sub-pixel offset applied to the pitch of the moment (model_setup.hpp with_pixel_offset).  What
// the render path and the ray-generating stage entry points hand to their kernels; adanerf_reproject, adanerf_foveate,
// adanerf_assemble_strips and the guard calibration read ms.rg itself.
RayGenParams rg_in_force(const adanerf_ctx* c) { return with_pixel_offset(c->ms.rg, c->px_dx, c->px_dy); }

bool has_budget_map(const adanerf_ctx* c) { return c->budget_n != nullptr || c->budget_thr != nullptr; }

// A batch whose rays are listed (adanerf_render_masked): ray i of the batch is ray first_ray + ids[i] of the frame, i < min(n_rays, *count).
struct RayList {
  const int32_t* ids;        // device, ascending ray ids
  const int32_t* count;      // device, >= the n_rays of every launch over the list
};

// sel != nullptr: the adaptive selection runs in the kernel's epilogue (k_select_pair.hip.hpp) and d_oracle may be null
// list != nullptr: sample_mlp16x3_kernel alone generates the listed rays and writes rows, counts, segment totals and ray records at the list
// position, as a dense batch (sel.refine_list stays null); a guarded context runs it as the split engine -- no first pass, no monitor
int launch_sample_mlp(adanerf_ctx* c, int first_ray, int n_rays, float* d_oracle, float* d_rays, const SelectOut* sel = nullptr,
                      const RayList* list = nullptr) {
  if (n_rays <= 0) return ADANERF_OK;
  if (list && (c->generic0 || !sel || (c->sampling_mode != ADANERF_SAMPLING_SPLIT_FP16 && c->sampling_mode != ADANERF_SAMPLING_GUARDED)))
    return fail(c, ADANERF_EUNSUPPORTED, "a ray list needs the 8 x 256 sampling network on the split-precision engine with the fused selection");
  SampleArgs a{};
  if (sel) {
    a.sel = *sel;
    a.fused_select = 1;
  }
  a.g = rg_in_force(c);
  a.net = c->net0.params;
  a.net16 = c->net0_split.params;
  a.overflow_flag = reinterpret_cast<int32_t*>(c->overflow.p);
  a.first_ray = first_ray;
  a.n_rays = n_rays;
  a.oracle_out = d_oracle;
  a.rays_out = d_rays;
  dim3 grid((n_rays + 127) / 128), block(256);
  if (c->generic0) {      // any other topology / encoding layout / raySampleInput: run-time-shaped kernels, no fused selection
    if (generic_split_sampling(c)) {
      // split-precision engine (fp32-class accuracy at 3 / 16 of the fp32-MFMA cycle count), weight tiles staged through LDS
      const int W0 = c->topo0.width;
      if (a.net16.n_bias > dispatch<64, 128, 256>(W0, [](auto w) { return uint32_t(gen_bias_cap<w()>()); }, 0u))
        return fail(c, ADANERF_EUNSUPPORTED, "sampling network: bias table exceeds the kernel's LDS capacity");      // cannot happen for depth <= 8
      return hip_rc(c, dispatch<kEnc10_4, kEnc2_2, kEncMax>(c->enc0, [&](auto e) {
        return dispatch<64, 128, 256>(W0, [&](auto w) {
          hipLaunchKernelGGL((sample_mlp16x3_gen_kernel<enc_fp(e()), enc_fd(e()), w()>), grid, block, 0, c->stream, a, c->gen0);
          return hipGetLastError();
        }, hipErrorInvalidValue);
      }, hipErrorInvalidValue), "hipGetLastError()");
    }
    if (sel) return fail(c, ADANERF_EINVAL, "fused selection is not available on the fp32 run-time-shaped sampling kernel");
    HIP_RETURN(c, launch_sample_mlp_gen(a, c->gen0, c->enc0, c->topo0.width, grid.x, c->stream));      // exact fp32 MFMA (and raySampleInput)
  }
  // Guarded two-precision selection: plain fp16 for every ray, then the split engine on the rays the guard band flagged.
  // Only where the selection is fused; otherwise this mode is the split-precision engine.
  // Nor under a budget map or a sample cap: unrefined rays keep the fp16 engine's values in selw, and a trim by them would not be the exact selection.
  const bool guarded = c->sampling_mode == ADANERF_SAMPLING_GUARDED && sel != nullptr && !has_budget_map(c) && !(c->sample_cap > 0.f) && !list;
  if (list) {      // guard_mask, guard_rows, guard_seen and sel.refine_list stay null: guard_flush has nothing to write
    a.ray_list = list->ids;
    a.n_list = list->count;
  }
  if (guarded) {
    // first guarded frame of a context created without a band: the model's record, or measure one
    if (int rc = c->guard_eps > 0.f ? 0 : ensure_guard_band(c)) return rc;
    a.sel.guard_mask = reinterpret_cast<uint32_t*>(c->guard_mask.p);
    a.sel.guard_eps = guard_band_of(c->ms.transform, c->guard_eps);
    a.sel.guard_pair = guard_pair_of(c->ms.transform, c->guard_eps, c->guard_eps_pair);
    a.sel.audit_period = c->guard_audit_period;
    a.sel.audit_phase = c->guard_audit_period > 0 ? static_cast<int32_t>(c->guard_frame & static_cast<uint32_t>(c->guard_audit_period - 1)) : 0;
    a.sel.guard_probe = reinterpret_cast<float*>(c->guard_probe.p);
    a.sel.guard_rows = reinterpret_cast<float*>(c->oracle.p);      // free on this path: the selection is fused, nobody else writes the oracle buffer
    if (c->debug_guard & 1) a.sel.guard_rows = nullptr;      // measurement knob (profiles/r04_guard_monitor_cost.md): no whole-row monitor
    a.sel.guard_seen = reinterpret_cast<uint32_t*>(c->total.p) + kTotalGuardSeen;
  }
  if (c->sampling_mode == ADANERF_SAMPLING_FP32) HIP_RETURN(c, launch_sample_mlp_f32(a, c->enc0, grid.x, c->stream));
  // from here on the 8 x 256 network in its two specialised encodings (generic0 is false): f(fp, fd) with the bands as constants
  auto for_enc = [&](auto&& f) {
    return dispatch<kEnc10_4, kEnc2_2>(c->enc0, [&](auto e) { return f(std::integral_constant<int, enc_fp(e())>{}, std::integral_constant<int, enc_fd(e())>{}); },
                                       hipErrorInvalidValue);
  };
  if (c->sampling_mode == ADANERF_SAMPLING_FP16 || guarded) {
    if (!c->net0_f16.w.p) {
      PackedNet pn;
      std::string err;
      const NetShape sh = shape_of(c->ms.fp0, c->ms.fd0, c->ms.fp1, c->ms.fd1, c->ms.ray_samples);
      if (!pack_sampling_net(c->net0_host, sh, Elem::F16, &pn, &err)) return fail(c, ADANERF_EIO, "model0.onnx: " + err);
      if (int rc = upload_net(c, pn, &c->net0_f16)) return rc;
    }
    a.net16 = c->net0_f16.params;
    // large batches with the fused selection: two ray blocks per wave (sample_mlp16x2_kernel, bit-identical outputs); $ADANERF_DEBUG_GUARD bit 1 keeps
    // the 8-wave kernel, bit 2 takes the two-block kernel whatever the batch size (tests)
    const bool two_blocks = sel != nullptr && a.fused_select && !a.oracle_out && !(c->debug_guard & 2) && (n_rays >= kSample16x2MinRays || (c->debug_guard & 4));
    // either way wave tiles are dealt out evenly over the grid: every workgroup of a small batch gets a share
    if (int rc = hip_rc(c, for_enc([&](auto fp, auto fd) {
      return two_blocks ? launch_persistent(c->grids, sample_mlp16x2_kernel<fp(), fd()>, (n_rays + 255) / 256, 256, c->stream, a)
                        : launch_persistent(c->grids, sample_mlp16_kernel<fp(), fd()>, (n_rays + 255) / 256, 512, c->stream, a);
    }), kOccupancyQuery)) return rc;
    if (guarded) {
      // undecided rays -> ascending list (+ count at total[kTotalRefined]) -> split engine over the list, rows overwritten in place
      const int n_words = (n_rays + 31) / 32;
      int32_t* n_list = reinterpret_cast<int32_t*>(c->total.p) + kTotalRefined;
      int resident = 0;
      if (int rc = hip_rc(c, for_enc([&](auto fp, auto fd) { return persistent_grid(c->grids, sample_mlp16x3_kernel<fp(), fd()>, 256, &resident); }), kOccupancyQuery)) return rc;
      const int rgrid = std::min(static_cast<int>(grid.x), resident);
      // ADANERF_FLAG_GUARD_AUDIT_FILL: the audit only fills the last round of the refinement pass (rgrid tiles of 128 rays per round)
      const int cap_round = (c->opt.flags & ADANERF_FLAG_GUARD_AUDIT_FILL) ? rgrid * 128 : 0;
      const int cycle = a.sel.audit_period > 0 ? static_cast<int>((c->guard_frame / static_cast<uint32_t>(a.sel.audit_period)) & 0x7fffffffu) : 0;
      hipLaunchKernelGGL(refine_list_kernel, dim3((n_words + 255) / 256), dim3(256), 0, c->stream, reinterpret_cast<const uint32_t*>(c->guard_mask.p),
                         n_words, n_rays, a.sel.audit_period, a.sel.audit_phase, cap_round, cycle, reinterpret_cast<int32_t*>(c->refine_list.p), n_list);
      SampleArgs r = a;
      r.net16 = c->net0_split.params;
      r.rays_out = nullptr;              // the first pass wrote the ray records
      r.sel.guard_mask = nullptr;
      // the second pass only monitors, in RAW units: the bound on single values, and -- where pass 1 used a measured one -- on differences
      r.sel.guard_band = c->guard_eps;
      r.sel.guard_band_pair = c->ms.transform == kOracleRaw ? a.sel.guard_pair : 0.f;
      r.sel.guard_eps = 0.f;
      r.sel.guard_pair = 0.f;
      r.sel.audit_period = 0;
      r.sel.refine_list = reinterpret_cast<const int32_t*>(c->refine_list.p);
      r.ray_list = r.sel.refine_list;
      r.n_list = n_list;
      if (int rc = hip_rc(c, for_enc([&](auto fp, auto fd) { return launch_persistent(c->grids, sample_mlp16x3_kernel<fp(), fd()>, rgrid, 256, c->stream, r); }), kOccupancyQuery)) return rc;
    }
  } else {
    if (int rc = hip_rc(c, for_enc([&](auto fp, auto fd) { return launch_persistent(c->grids, sample_mlp16x3_kernel<fp(), fd()>, static_cast<int>(grid.x), 256, c->stream, a); }), kOccupancyQuery)) return rc;
  }
  HIP_RETURN(c, hipGetLastError());
}

// above this many segment totals (one per 32 or 64 rays) they are scanned by their own kernel
constexpr int kInlineScanMaxBlocks = 65536;

SelectOut select_out(adanerf_ctx* c, int n_max, float thr, int32_t* d_cnt) {
  SelectOut so{};
  so.counts = d_cnt;
  so.selbin = reinterpret_cast<uint8_t*>(c->selbin.p);
  so.selw = reinterpret_cast<float*>(c->selw.p);
  so.seg_total = reinterpret_cast<int32_t*>(c->block_total.p);
  so.n_max = n_max;
  so.thr = thr;
  so.transform = c->ms.transform;
  return so;
}

// the selection (counts, selbin, selw, segment totals per 2^seg_shift rays) is in place: offsets + compacted arrays
int launch_expand(adanerf_ctx* c, int n_rays, int n_max, int seg_shift, int32_t* d_off, const int32_t* d_cnt, uint32_t* d_key, float* d_w,
                  int32_t* d_total) {
  const int nblk = (n_rays + (1 << seg_shift) - 1) >> seg_shift;
  const int32_t* bt = reinterpret_cast<const int32_t*>(c->block_total.p);
  int32_t* bo = reinterpret_cast<int32_t*>(c->block_offset.p);
  const dim3 egrid((n_rays + 255) / 256);
  const bool inline_scan = nblk <= kInlineScanMaxBlocks;
  if (!inline_scan) hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, c->stream, bt, nblk, bo, d_total);
  hipLaunchKernelGGL(inline_scan ? expand_kernel<true> : expand_kernel<false>, egrid, dim3(256), 0, c->stream, d_cnt, reinterpret_cast<const uint8_t*>(c->selbin.p),
                     reinterpret_cast<const float*>(c->selw.p), bo, bt, nblk, n_rays, n_max, seg_shift, d_off, d_key, d_w, d_total);
  HIP_RETURN(c, hipGetLastError());
}

// Per-ray budgets: the selection of the batch (counts, selbin, selw, segment totals per 2^seg_shift rays) trimmed to (n_r, thr_r) before
// launch_expand (k_budget.hip.hpp).  The maps are indexed by local ray: ray 0 of the batch is entry map_first.
struct BudgetMaps {
  const uint8_t* n;
  const float* thr;
  int first;
};

int launch_trim(adanerf_ctx* c, const BudgetMaps& bm, int n_rays, int n_max, float thr, int seg_shift, int32_t* d_cnt) {
  if (n_rays <= 0) return ADANERF_OK;
  const bool per_thread = n_max <= kTrimThreadMaxN;
  const dim3 grid(per_thread ? (n_rays + 255) / 256 : (n_rays + (1 << seg_shift) - 1) >> seg_shift);
  hipLaunchKernelGGL(per_thread ? trim_rows_kernel : trim_rows_wave_kernel, grid, dim3(256), 0, c->stream, d_cnt, reinterpret_cast<uint8_t*>(c->selbin.p),
                     reinterpret_cast<float*>(c->selw.p), bm.n, bm.thr, bm.first, n_rays, n_max, thr, seg_shift, reinterpret_cast<int32_t*>(c->block_total.p));
  HIP_RETURN(c, hipGetLastError());
}

// Per-ray depth limits: the selection of the batch (after the budget trim, if any) trimmed to the entries in front of the caller's surface
// before launch_expand (k_depth_limit.hip.hpp).  zc is indexed by local ray: ray i of the batch is entry first + i, with a list first + list[i].
struct DepthLimit {
  const float* zc;
  int first;
  const int32_t* list;       // device ray ids of a listed batch, or null
  const float* rays;         // [n,8] ray records of the batch
  const float* ztab;         // [128] depth per bin
  DepthPose pose;
};

DepthPose depth_pose(const float pos[3], const float rot[9]) { return DepthPose{{pos[0], pos[1], pos[2]}, rot[2], rot[5], rot[8]}; }

int launch_depth_limit(adanerf_ctx* c, const DepthLimit& dl, int n_rays, int n_max, int seg_shift, int32_t* d_cnt) {
  if (n_rays <= 0) return ADANERF_OK;
  hipLaunchKernelGGL(depth_limit_kernel, dim3((n_rays + 255) / 256), dim3(256), 0, c->stream, d_cnt, reinterpret_cast<uint8_t*>(c->selbin.p),
                     reinterpret_cast<float*>(c->selw.p), dl.rays, dl.zc, dl.list, dl.first, dl.pose, dl.ztab, n_rays, n_max, seg_shift,
                     reinterpret_cast<int32_t*>(c->block_total.p));
  HIP_RETURN(c, hipGetLastError());
}

// A bound on the batch's samples (adanerf_set_sample_cap, k_cap.hip.hpp): after the selection, the budget trim and the depth limit, before
// launch_expand.  Three histogram passes over the rows, each followed by its one-workgroup digit search; then t* goes into the context's
// threshold map and the unchanged trim kernels run at (n_max, t*).  Nothing is read back; when the batch fits, the later passes return at once
// and the trim changes no row.
bool has_sample_cap(const adanerf_ctx* c) { return c->sample_cap > 0.f; }

// a cap at or above N cannot trim: nothing is launched for it
bool cap_trims(const adanerf_ctx* c) { return has_sample_cap(c) && c->sample_cap < static_cast<float>(c->ms.info.num_samples); }

int64_t cap_total_of(const adanerf_ctx* c, int n_rays) { return static_cast<int64_t>(std::floor(static_cast<double>(c->sample_cap) * n_rays)); }

constexpr size_t kCapStateBytes = sizeof(CapState) + static_cast<size_t>(kCapLevels) * 2 * kCapBins * sizeof(uint32_t);

// scratch of the cap for batches of n_rays; grown on demand, freed with the context
int ensure_cap_buffers(adanerf_ctx* c, int n_rays) {
  const size_t map_bytes = static_cast<size_t>(std::max(n_rays, 1)) * sizeof(float);
  if (c->cap_state.p && c->cap_record.p && c->cap_map.bytes >= map_bytes) return ADANERF_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // an enqueued batch may still read the smaller map
  int rc;
  if ((rc = dev_alloc(c, &c->cap_state, kCapStateBytes))) return rc;
  if ((rc = dev_alloc(c, &c->cap_map, map_bytes))) return rc;
  if (!c->cap_record.p) {
    if ((rc = dev_alloc(c, &c->cap_record, sizeof(CapRecord)))) return rc;
    hipLaunchKernelGGL(cap_reset_kernel, dim3(1), dim3(1), 0, c->stream, reinterpret_cast<CapRecord*>(c->cap_record.p));
    HIP_TRY(c, hipGetLastError());
  }
  return ADANERF_OK;
}

int launch_cap(adanerf_ctx* c, int n_rays, int n_max, float thr, int seg_shift, int32_t* d_cnt, int64_t cap_total) {
  if (n_rays <= 0) return ADANERF_OK;
  CapState* st = reinterpret_cast<CapState*>(c->cap_state.p);
  uint32_t* hist = reinterpret_cast<uint32_t*>(st + 1);
  CapRecord* rec = reinterpret_cast<CapRecord*>(c->cap_record.p);
  float* map = reinterpret_cast<float*>(c->cap_map.p);
  const float* selw = reinterpret_cast<const float*>(c->selw.p);
  HIP_TRY(c, hipMemsetAsync(st, 0, kCapStateBytes, c->stream));
  const bool wave = n_max > kCapThreadMaxN;
  // few workgroups, each over many rays: a workgroup flushes every occupied bin of its private histograms with one global atomic, and where the
  // values share their leading bits every workgroup adds to the same few words (measured at 640 000 rays: 194 us for the first pass with 2 048
  // workgroups and a wave's counters added straight to global memory, profiles/sample_cap_measured.md)
  const int cus = std::max(c->ms.info.compute_units, 1);
  const dim3 grid(wave ? std::min((n_rays + 3) / 4, 4 * cus) : std::min((n_rays + 255) / 256, 2 * cus));
  for (int level = 0; level < kCapLevels; ++level) {
    uint32_t* h = hist + static_cast<size_t>(level) * 2 * kCapBins;
    hipLaunchKernelGGL(wave ? cap_hist_kernel<true> : cap_hist_kernel<false>, grid, dim3(256), 0, c->stream, d_cnt, selw, n_rays, n_max, level, st, h);
    hipLaunchKernelGGL(cap_search_kernel, dim3(1), dim3(1024), 0, c->stream, level, static_cast<long long>(cap_total), st, h, rec);
  }
  hipLaunchKernelGGL(cap_fill_kernel, dim3((n_rays + 255) / 256), dim3(256), 0, c->stream, rec, n_rays, map);
  HIP_TRY(c, hipGetLastError());
  return launch_trim(c, BudgetMaps{nullptr, map, 0}, n_rays, n_max, thr, seg_shift, d_cnt);
}

// the pair selection keeps its sorted candidate lists in registers: n_max <= kPairMaxN; ADANERF_FLAG_WAVE_SELECT forces the
// wave-per-ray select_kernel (any n_max)
bool use_pair_select(const adanerf_ctx* c, int n_max) { return n_max <= kPairMaxN && !(c->opt.flags & ADANERF_FLAG_WAVE_SELECT); }

int launch_compact(adanerf_ctx* c, const float* d_oracle, int n_rays, int n_max, float thr, int32_t* d_off, int32_t* d_cnt,
                   uint32_t* d_key, float* d_w, int32_t* d_total, const BudgetMaps* bm = nullptr, const DepthLimit* dl = nullptr,
                   const int64_t* cap_total = nullptr) {
  if (n_rays <= 0) return ADANERF_OK;
  if (thr == 0.0f) {
    const size_t n = static_cast<size_t>(n_rays) * kBins;
    dim3 grid(static_cast<unsigned>((n + 255) / 256)), block(256);
    hipLaunchKernelGGL(dense_expand_kernel, grid, block, 0, c->stream, d_oracle, n_rays, d_off, d_cnt, d_key, d_w, d_total);
    HIP_RETURN(c, hipGetLastError());
  }
  if (use_pair_select(c, n_max)) {
    hipLaunchKernelGGL(select_rows_kernel, dim3((n_rays + 127) / 128), dim3(256), 0, c->stream, d_oracle, n_rays, select_out(c, n_max, thr, d_cnt),
                       static_cast<const int32_t*>(nullptr));
    if (bm)
      if (int rc = launch_trim(c, *bm, n_rays, n_max, thr, kPairSegShift, d_cnt)) return rc;
    if (dl)
      if (int rc = launch_depth_limit(c, *dl, n_rays, n_max, kPairSegShift, d_cnt)) return rc;
    if (cap_total)
      if (int rc = launch_cap(c, n_rays, n_max, thr, kPairSegShift, d_cnt, *cap_total)) return rc;
    return launch_expand(c, n_rays, n_max, kPairSegShift, d_off, d_cnt, d_key, d_w, d_total);
  }
  const int nblk = (n_rays + kSelRaysPerBlock - 1) / kSelRaysPerBlock;
  hipLaunchKernelGGL(select_kernel, dim3(nblk), dim3(256), 0, c->stream, d_oracle, n_rays, n_max, thr, c->ms.transform, d_cnt,
                     reinterpret_cast<uint8_t*>(c->selbin.p), reinterpret_cast<float*>(c->selw.p),
                     reinterpret_cast<int32_t*>(c->block_total.p));
  if (bm)
    if (int rc = launch_trim(c, *bm, n_rays, n_max, thr, kSelSegShift, d_cnt)) return rc;
  if (dl)
    if (int rc = launch_depth_limit(c, *dl, n_rays, n_max, kSelSegShift, d_cnt)) return rc;
  if (cap_total)
    if (int rc = launch_cap(c, n_rays, n_max, thr, kSelSegShift, d_cnt, *cap_total)) return rc;
  return launch_expand(c, n_rays, n_max, kSelSegShift, d_off, d_cnt, d_key, d_w, d_total);
}

// what the calibration record of this context's guarded selection is filed under (guard_record.hpp)
GuardKey guard_key(adanerf_ctx* c) {
  if (!c->model0_hash) c->model0_hash = fnv1a64_file(join_path(c->model_dir, "model0.onnx"));
  return GuardKey{c->model0_hash, c->ms.fp0, c->ms.fd0, c->ms.transform, kGuardEngineRev, c->ms.info.num_samples, c->ms.info.threshold, c->model_dir, c->opt.flags};
}

void install_guard_band(adanerf_ctx* c, float max_diff, float max_pair, int poses, int source) {
  c->guard_eps = std::max(ADANERF_GUARD_CALIB_MARGIN * max_diff, ADANERF_GUARD_EPS_MIN);
  // a measured pair bound applies to untransformed outputs only (guard_pair_of); never below the floor, never above what the
  // single-value bound implies
  c->guard_eps_pair = (c->ms.transform == kOracleRaw && max_pair > 0.f)
                          ? std::min(std::max(ADANERF_GUARD_CALIB_MARGIN * max_pair, ADANERF_GUARD_EPS_MIN), 2.0f * c->guard_eps)
                          : 2.0f * c->guard_eps;
  c->ms.info.guard_eps = c->guard_eps;
  c->ms.info.guard_eps_pair = c->guard_eps_pair;
  c->ms.info.guard_calib_source = source;
  c->ms.info.guard_calib_poses = poses;
}

// Largest |plain-fp16 - split-precision| raw output of the sampling network over n_poses x 64 x 64 calibration rays, and the largest
// error of a (kept - candidate) difference under the single-value bound that gives (include/adanerf_hip.h: adanerf_calibrate_guard).
// Two sweeps over the same seeded poses: the second statistic needs the first.  Temporarily replaces the ray generator's image and camera.
int calibrate_guard(adanerf_ctx* c, int n_poses, uint32_t seed, bool install, float* max_diff, float* max_pair) {
  if (c->ms.coarse_fine || c->generic0) return fail(c, ADANERF_EUNSUPPORTED, "guard calibration needs an 8 x 256 sampling network");
  if (n_poses < 1 || n_poses > 4096) return fail(c, ADANERF_EINVAL, "n_poses must be in 1..4096");
  constexpr int CW = 64, CH = 64, CR = CW * CH;
  const RayGenParams saved = c->ms.rg;
  const int saved_mode = c->sampling_mode;
  const float saved_dx = c->px_dx, saved_dy = c->px_dy;      // its own 64 x 64 rays through pixel centres: the band must not depend on a jitter
  c->px_dx = c->px_dy = 0.f;
  RayGenParams g = saved;
  // same field of view on a 64 x 64 image (setup_model's arithmetic): x_dist = tan(fov / 2) focal, y_dist = x_dist h / w
  const double x_dist = -saved.start_x + saved.x_pp / 2, y_dist = -saved.start_y + saved.y_pp / 2;
  g.w = CW;
  g.h = CH;
  g.x_pp = x_dist / (CW / 2.0);
  g.y_pp = y_dist / (CH / 2.0);
  g.start_x = -(x_dist - g.x_pp / 2);
  g.start_y = -(y_dist - g.y_pp / 2);
  g.strip_rows = CH;
  g.world = 1;
  g.rank = 0;
  DevBuf a_buf, b_buf, acc;
  int rc = ADANERF_OK;
  auto done = [&](int code) {
    (void)hipStreamSynchronize(c->stream);      // before a_buf, b_buf and acc leave scope
    c->ms.rg = saved;
    c->sampling_mode = saved_mode;
    c->px_dx = saved_dx;
    c->px_dy = saved_dy;
    return code;
  };
  if ((rc = dev_alloc(c, &a_buf, static_cast<size_t>(CR) * kBins * sizeof(float)))) return done(rc);
  if ((rc = dev_alloc(c, &b_buf, static_cast<size_t>(CR) * kBins * sizeof(float)))) return done(rc);
  if ((rc = dev_alloc(c, &acc, 64))) return done(rc);
  if (hipMemsetAsync(acc.p, 0, 64, c->stream) != hipSuccess) return done(fail(c, ADANERF_EDEVICE, "hipMemsetAsync failed"));
  const bool want_pairs = c->ms.transform == kOracleRaw && c->ms.info.threshold > 0.f && c->ms.info.num_samples <= kPairMaxN;
  float d = 0.f, dp = 0.f;
  bool nonfinite = false;
  for (int sweep = 0; sweep < (want_pairs ? 2 : 1) && !nonfinite; ++sweep) {
    const float two_eps = sweep == 0 ? 0.f : 2.0f * std::max(ADANERF_GUARD_CALIB_MARGIN * d, ADANERF_GUARD_EPS_MIN);
    uint64_t st = 0x9E3779B97F4A7C15ull ^ (static_cast<uint64_t>(seed) << 17);
    auto rnd = [&]() {      // xorshift64*, uniform in [0, 1)
      st ^= st >> 12;
      st ^= st << 25;
      st ^= st >> 27;
      return static_cast<double>((st * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
    };
    for (int k = 0; k < n_poses; ++k) {
      for (int i = 0; i < 3; ++i) g.pos[i] = g.center[i] + static_cast<float>((rnd() - 0.5) * 0.9 * c->ms.info.view_cell_size[i]);
      // orientation: yaw about z, then pitch (the viewer's camera: z up, looking along -z of the camera frame)
      const double yaw = 2.0 * M_PI * rnd(), pitch = (rnd() - 0.5) * (c->ms.info.use_ndc ? 0.2 : 1.4);
      const double cy = std::cos(yaw), sy = std::sin(yaw), cp = std::cos(pitch), sp = std::sin(pitch);
      double fwd[3], right[3], up[3];
      if (c->ms.info.use_ndc) {      // forward-facing scenes look down -z
        fwd[0] = sp * cy; fwd[1] = sp * sy; fwd[2] = -cp;
        right[0] = 1; right[1] = 0; right[2] = 0;
      } else {
        fwd[0] = cp * cy; fwd[1] = cp * sy; fwd[2] = sp;
        right[0] = sy; right[1] = -cy; right[2] = 0;
      }
      // re-orthogonalise: right = normalize(right - (right . fwd) fwd), up = right x fwd
      const double rf = right[0] * fwd[0] + right[1] * fwd[1] + right[2] * fwd[2];
      double n = 0;
      for (int i = 0; i < 3; ++i) { right[i] -= rf * fwd[i]; n += right[i] * right[i]; }
      n = std::sqrt(n);
      for (int i = 0; i < 3; ++i) right[i] /= n;
      up[0] = right[1] * fwd[2] - right[2] * fwd[1];
      up[1] = right[2] * fwd[0] - right[0] * fwd[2];
      up[2] = right[0] * fwd[1] - right[1] * fwd[0];
      for (int i = 0; i < 3; ++i) {      // columns of c2w: camera x = right, y = up, -z = forward
        g.rot[3 * i + 0] = static_cast<float>(right[i]);
        g.rot[3 * i + 1] = static_cast<float>(up[i]);
        g.rot[3 * i + 2] = static_cast<float>(-fwd[i]);
      }
      c->ms.rg = g;
      c->sampling_mode = ADANERF_SAMPLING_SPLIT_FP16;
      if ((rc = launch_sample_mlp(c, 0, CR, reinterpret_cast<float*>(a_buf.p), nullptr))) return done(rc);
      c->sampling_mode = ADANERF_SAMPLING_FP16;
      if ((rc = launch_sample_mlp(c, 0, CR, reinterpret_cast<float*>(b_buf.p), nullptr))) return done(rc);
      hipLaunchKernelGGL(guard_stats_kernel, dim3((CR + 3) / 4), dim3(256), 0, c->stream, reinterpret_cast<const float*>(b_buf.p),
                         reinterpret_cast<const float*>(a_buf.p), CR, c->ms.info.num_samples, c->ms.info.threshold, two_eps, reinterpret_cast<uint32_t*>(acc.p));
    }
    uint32_t res[3] = {0, 0, 0};
    if (hipMemcpyAsync(res, acc.p, sizeof(res), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
      return done(fail(c, ADANERF_EDEVICE, "guard calibration: read-back failed"));
    std::memcpy(&d, &res[0], sizeof(d));
    std::memcpy(&dp, &res[2], sizeof(dp));
    nonfinite = res[1] != 0;
  }
  if (max_diff) *max_diff = nonfinite ? INFINITY : d;
  if (max_pair) *max_pair = (nonfinite || !want_pairs) ? 0.f : dp;
  if (install) {
    if (nonfinite) {
      c->guard_eps = ADANERF_GUARD_EPS_DEFAULT;
      c->guard_eps_pair = 2.0f * c->guard_eps;
      c->ms.info.guard_eps = c->guard_eps;
      c->ms.info.guard_eps_pair = c->guard_eps_pair;
      c->ms.info.guard_calib_source = ADANERF_GUARD_FROM_CALIBRATION;
      c->ms.info.guard_calib_poses = n_poses;
    } else {
      install_guard_band(c, d, want_pairs ? dp : 0.f, n_poses, ADANERF_GUARD_FROM_CALIBRATION);
      const GuardKey key = guard_key(c);
      GuardRecord old;      // a record from more poses than this measurement stays
      if (!(read_guard_record(key, &old) && old.poses > n_poses)) write_guard_record(key, GuardRecord{n_poses, seed, d, want_pairs ? dp : 0.f});
    }
  }
  return done(ADANERF_OK);
}

// first guarded frame of a context created without a band: the model's calibration record if it is current, else a measurement
int ensure_guard_band(adanerf_ctx* c) {
  GuardRecord r;
  if (read_guard_record(guard_key(c), &r) && r.poses >= ADANERF_GUARD_CALIB_POSES) {
    install_guard_band(c, r.max_diff, r.max_pair, r.poses, ADANERF_GUARD_FROM_RECORD);
    return ADANERF_OK;
  }
  float d = 0.f, dp = 0.f;
  return calibrate_guard(c, ADANERF_GUARD_CALIB_POSES, 1u, true, &d, &dp);
}

// The guarded selection's band belongs to (model, N, threshold): the state of a context before its first guarded frame -- bounds from
// the options if they give any, else 0 = the key's calibration record or a measurement at that frame (ensure_guard_band); the audit
// starts over.  The counters adanerf_stats documents as "since create" (and the device's running maxima behind them) go on; the per-frame
// count of re-evaluated rays does not: only a fused guarded frame writes it, and the new pair may have none (cleared in stream order, so
// the frames already enqueued still report theirs).
int reset_guard_band(adanerf_ctx* c) {
  if (c->sampling_mode == ADANERF_SAMPLING_GUARDED)      // first: the one step that can fail
    HIP_TRY(c, hipMemsetAsync(reinterpret_cast<int32_t*>(c->total.p) + kTotalRefined, 0, sizeof(int32_t), c->stream));
  const adanerf_options& opt = c->opt;
  c->guard_eps = opt.guard_eps > 0.f ? opt.guard_eps : 0.f;
  c->guard_eps_pair = (c->guard_eps > 0.f && opt.guard_eps_pair > 0.f) ? std::min(opt.guard_eps_pair, 2.0f * c->guard_eps) : 2.0f * c->guard_eps;
  c->ms.info.guard_eps = c->guard_eps;
  c->ms.info.guard_eps_pair = c->guard_eps_pair;
  c->ms.info.guard_calib_source = c->guard_eps > 0.f ? ADANERF_GUARD_FROM_OPTIONS : ADANERF_GUARD_FROM_NONE;
  c->ms.info.guard_calib_poses = 0;
  c->guard_frame = 0;
  c->guard_ev_stale = c->guard_ev_pending;
  return ADANERF_OK;
}

// Context state that follows from the (N, threshold) select_samples left in ms.info: adanerf_create and adanerf_set_selection both end
// here.  Buffer capacities follow the largest N the context has held (ensure_batch_buffers never shrinks); row strides, the selection
// path, the compositing kernel and the calibration record's key are read off ms.info at every launch.
int apply_selection(adanerf_ctx* c) {
  if (int rc = ensure_batch_buffers(c, c->ms.info.batch_rays, c->ms.info.num_samples)) return rc;
  if (int rc = reset_guard_band(c)) return rc;
  c->ms.sp.ztab = reinterpret_cast<const float*>(c->ztab.p) + (c->ms.info.dense ? kBins : 0);
  return ADANERF_OK;
}

// Context state that follows from the (width, height) frame_geometry left in ms.info / ms.rg: adanerf_set_frame_size ends here (create
// goes through apply_selection, whose buffer call sees the same batch).  Capacities follow the largest batch the context has held; the
// caller's per-ray outputs were sized for `was_rays` rays.  The guard band belongs to (model, N, threshold) and stays; its audit starts over.
int apply_frame_size(adanerf_ctx* c, int was_rays) {
  const size_t B = static_cast<size_t>(c->ms.info.batch_rays);
  if (int rc = ensure_batch_buffers(c, c->ms.info.batch_rays, c->ms.info.num_samples)) return rc;
  if (c->disp_scratch.p && c->disp_scratch.bytes < B * 2 * sizeof(float)) {      // adanerf_render would grow it: not with frames in flight
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int rc = dev_alloc(c, &c->disp_scratch, B * 2 * sizeof(float))) return rc;
  }
  if (c->ms.info.rays_local != was_rays) {
    c->aux_depth = c->aux_acc = c->aux_disp = nullptr;
    c->budget_n = nullptr;      // the budget maps were sized for the old rays_local too
    c->budget_thr = nullptr;
    c->depth_limit = nullptr;      // and so was the depth limit
  }
  c->guard_frame = 0;
  return ADANERF_OK;
}

int launch_shade_mlp(adanerf_ctx* c, const float* d_rays, const uint32_t* d_key, const int32_t* d_total, int max_samples, int prec,
                     float* d_raw, const float* d_z = nullptr, bool coarse = false) {
  if (max_samples <= 0) return ADANERF_OK;
  // coarse: the first network of the vanilla-NeRF mode (model0.onnx as a NeRF net, uniform depth table)
  const bool generic = coarse ? c->genericc : c->generic1;
  const NetTopology& topo = coarse ? c->topoc : c->topo1;
  const GenericTopo& gen = coarse ? c->genc : c->gen1;
  int rc = ensure_shading_net(c, prec, coarse);
  if (rc) return rc;
  ShadeArgs a{};
  a.sp = coarse ? c->spc : c->ms.sp;
  a.net = coarse ? c->netc[prec].params : c->net1[prec].params;
  a.rays = d_rays;
  a.sample_key = d_key;
  a.sample_z = d_z;
  a.total = d_total;
  a.max_samples = max_samples;
  a.raw_out = d_raw;
  // a position that is not finite, or beyond what the scaled bf16 packing was proved for, comes out as NaN (k_mlp16.hip.hpp position_outside)
  a.pos_limit = prec == ADANERF_PREC_BF16 ? static_cast<float>(kPosIdentityBound) : std::numeric_limits<float>::max();
  const int enc = coarse ? enc_layout(c->ms.fp0, c->ms.fd0, false) : c->enc1;      // generic nets only: kEnc10_4, or the catch-all 16-band layout
  auto for_elem = [&](auto&& f) { return prec == ADANERF_PREC_BF16 ? f(Bf16{}) : f(Fp16{}); };
  if (generic && prec != ADANERF_PREC_FP32) {
    // Any topology / encoding layout on the 16-bit MFMA pipe (k_generic16.hip.hpp): one copy of every weight tile per workgroup
    // through LDS, gen_blocks 32-sample blocks per wave.  Persistent grid = the workgroups the chosen
    // instantiation really keeps resident (registers and LDS differ per width / layout).
    if (a.net.n_bias > dispatch<64, 128, 256, 512>(topo.width, [](auto w) { return uint32_t(gen_bias_cap<w()>()); }, 0u))
      return fail(c, ADANERF_EUNSUPPORTED, "shading network: bias table exceeds the kernel's LDS capacity");      // cannot happen for depth <= 8 (pack.hpp kMaxDepth)
    if ((rc = hip_rc(c, for_elem([&](auto et) {
      return dispatch<kEnc10_4, kEncMax>(enc, [&](auto e) {
        return dispatch<64, 128, 256, 512>(topo.width, [&](auto w) {
          using ET = decltype(et);
          constexpr int FP = enc_fp(e()), FD = enc_fd(e()), W = w(), NB = gen_blocks<W, FP>();
          const int tiles = (max_samples + 128 * NB - 1) / (128 * NB);
          return launch_persistent(c->grids, shade_mlp16_gen_staged_kernel<ET, FP, FD, W, NB, gen_occupancy<W, FP>()>, tiles, 256, c->stream, a, gen);
        }, hipErrorInvalidValue);
      }, hipErrorInvalidValue);
    }), kOccupancyQuery))) return rc;
  } else if (generic) {
    const int per_wg = topo.width == kWideWidth ? 64 : 128;      // the wide form runs 16-sample blocks
    HIP_TRY(c, launch_shade_mlp_gen(c->grids, a, gen, enc, topo.width, (max_samples + per_wg - 1) / per_wg, c->stream));
  } else if (prec == ADANERF_PREC_FP32) {
    HIP_TRY(c, launch_shade_mlp_f32(c->grids, a, (max_samples + 127) / 128, c->stream));
  } else {
    const int tiles = (max_samples + 255) / 256;
    if ((rc = hip_rc(c, for_elem([&](auto et) {
      using ET = decltype(et);
      // two sample blocks per wave, 4 waves x 64 samples = 256-sample tiles, one workgroup per CU
      hipLaunchKernelGGL((shade_mlp16x2_kernel<ET, 10, 4>), dim3(std::min(tiles, c->ms.info.compute_units)), dim3(256), 0, c->stream, a);
      return hipSuccess;
    }), kOccupancyQuery))) return rc;
  }
  HIP_RETURN(c, hipGetLastError());
}

int launch_sample_pdf(adanerf_ctx* c, const float* d_oracle, int n_rays, int n, int32_t* d_off, int32_t* d_cnt, uint32_t* d_key, float* d_w,
                      float* d_z, int32_t* d_total) {
  if (n_rays <= 0) return ADANERF_OK;
  const int grid = std::min((n_rays + 3) / 4, c->ms.info.compute_units * 8);
  hipLaunchKernelGGL(pdf_sample_kernel, dim3(grid), dim3(256), 0, c->stream, d_oracle, n_rays, n, c->ms.transform, c->ms.dm, d_off, d_cnt, d_key, d_w, d_z, d_total);
  HIP_RETURN(c, hipGetLastError());
}

int launch_camera_rays(adanerf_ctx* c, int first_ray, int n_rays, float* d_rays) {
  if (n_rays <= 0) return ADANERF_OK;
  hipLaunchKernelGGL(camera_rays_kernel, dim3((n_rays + 255) / 256), dim3(256), 0, c->stream, rg_in_force(c), first_ray, n_rays, d_rays);
  HIP_RETURN(c, hipGetLastError());
}

int launch_sample_uniform(adanerf_ctx* c, int n_rays, int n, int32_t* d_off, int32_t* d_cnt, uint32_t* d_key, int32_t* d_total) {
  if (n_rays <= 0) return ADANERF_OK;
  const int64_t s = static_cast<int64_t>(n_rays) * n;
  hipLaunchKernelGGL(uniform_sample_kernel, dim3(static_cast<unsigned>((s + 255) / 256)), dim3(256), 0, c->stream, n_rays, n, d_off, d_cnt, d_key, d_total);
  HIP_RETURN(c, hipGetLastError());
}

int launch_sample_fine(adanerf_ctx* c, const float* d_raw_coarse, const float* d_rays, int n_rays, int32_t* d_off, int32_t* d_cnt,
                       uint32_t* d_key, float* d_z, int32_t* d_total) {
  if (n_rays <= 0) return ADANERF_OK;
  hipLaunchKernelGGL(fine_sample_kernel, dim3((n_rays + kFineRaysPerBlock - 1) / kFineRaysPerBlock), dim3(kFineRaysPerBlock), 0, c->stream,
                     reinterpret_cast<const float4*>(d_raw_coarse), reinterpret_cast<const float*>(c->ztab_coarse.p), d_rays, n_rays, c->ms.n_coarse,
                     c->ms.info.num_samples - c->ms.n_coarse, d_off, d_cnt, d_key, d_z, d_total);
  HIP_RETURN(c, hipGetLastError());
}

int launch_composite_classic(adanerf_ctx* c, const float* d_raw, const float* d_z, const float* d_rays, int n_rays, int n, float* d_rgb,
                             void* d_rgba8, float* d_depth = nullptr, float* d_acc = nullptr) {
  if (n_rays <= 0) return ADANERF_OK;
  const bool wave = n > 32;      // long rays: one wave per ray, coalesced
  hipLaunchKernelGGL(wave ? composite_classic_wave_kernel : composite_classic_kernel, dim3((n_rays + (wave ? 3 : 255)) / (wave ? 4 : 256)), dim3(256), 0, c->stream,
                     reinterpret_cast<const float4*>(d_raw), d_z, d_rays, n_rays, n, d_rgb, reinterpret_cast<uchar4*>(d_rgba8), d_depth, d_acc);
  HIP_RETURN(c, hipGetLastError());
}

int launch_composite(adanerf_ctx* c, const float* d_raw, const float* d_w, const int32_t* d_off, const int32_t* d_cnt, int n_rays,
                     float* d_rgb, void* d_rgba8, const uint32_t* d_key = nullptr, float* d_depth = nullptr, float* d_acc = nullptr) {
  if (n_rays <= 0) return ADANERF_OK;
  AuxOut aux{};
  if ((d_key || c->ms.info.dense) && (d_depth || d_acc)) {
    aux.depth = d_depth;
    aux.acc = d_acc;
    aux.sample_key = d_key;      // null in dense mode: the bin of sample i is i & 127
    aux.ztab = c->ms.sp.ztab;
  }
  if (c->ms.info.num_samples > 32)   // long rays (dense mode): one wave per ray, coalesced
    hipLaunchKernelGGL(composite_wave_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, c->stream, reinterpret_cast<const float4*>(d_raw), d_w,
                       d_off, d_cnt, n_rays, c->ms.mult_mode, d_rgb, reinterpret_cast<uchar4*>(d_rgba8), aux);
  else {
    // samples of RB consecutive rays staged in LDS (20 B each), RB chosen so that RB * N * 20 B <= 48 KB
    const int N = c->ms.info.num_samples;
    auto run = [&](auto rb_tag) {
      constexpr int RB = decltype(rb_tag)::value;
      const int cap = RB * N;
      hipLaunchKernelGGL(composite_kernel<RB>, dim3((n_rays + RB - 1) / RB), dim3(RB), static_cast<size_t>(cap) * 20, c->stream,
                         reinterpret_cast<const float4*>(d_raw), d_w, d_off, d_cnt, n_rays, c->ms.mult_mode, cap, d_rgb,
                         reinterpret_cast<uchar4*>(d_rgba8), aux);
    };
    if (N <= 9) run(std::integral_constant<int, 256>{});
    else if (N <= 19) run(std::integral_constant<int, 128>{});
    else run(std::integral_constant<int, 64>{});
  }
  HIP_RETURN(c, hipGetLastError());
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================

extern "C" {

const char* adanerf_last_error(const adanerf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

static int create_on(adanerf_ctx* c, const char* model_dir, const adanerf_options* opt, adanerf_ctx** out);

int adanerf_create(const char* model_dir, const adanerf_options* opt, adanerf_ctx** out) {
  if (!out) return fail(nullptr, ADANERF_EINVAL, "out == NULL");
  *out = nullptr;
  if (!model_dir || !opt) return fail(nullptr, ADANERF_EINVAL, "model_dir/opt == NULL");
  adanerf_ctx* c = nullptr;
  try {
    c = new adanerf_ctx();
    return create_on(c, model_dir, opt, out);
  } catch (const std::exception& e) {      // see setup_model: the loader's exceptions end here, with the context released
    *out = nullptr;
    adanerf_destroy(c);
    return fail(nullptr, ADANERF_EIO, std::string("adanerf_create: ") + e.what());
  }
}

static int create_on(adanerf_ctx* c, const char* model_dir, const adanerf_options* opt, adanerf_ctx** out) {
  auto bail = [&](int code, const std::string& msg) {
    g_create_error = msg;
    adanerf_destroy(c);
    return code;
  };
  std::string err;
  ModelSetup& ms = c->ms;
  int rc = setup_model(model_dir, opt, &ms, &err);
  if (rc) return bail(rc, err);
  c->opt = *opt;

  // ---- weights: parse + pack on the host before touching the device ----
  TensorMap& n0 = c->net0_host;
  if (!read_onnx_initializers(join_path(model_dir, "model0.onnx"), &n0, &err)) return bail(ADANERF_EIO, err);
  if (!read_onnx_initializers(join_path(model_dir, "model1.onnx"), &c->net1_host, &err)) return bail(ADANERF_EIO, err);
  const NetShape sh = shape_of(c->ms.fp0, c->ms.fd0, c->ms.fp1, c->ms.fd1, c->ms.ray_samples, !c->ms.coarse_fine);
  c->enc0 = enc_layout(c->ms.fp0, c->ms.fd0, !c->ms.coarse_fine);
  c->enc1 = enc_layout(c->ms.fp1, c->ms.fd1, false);
  PackedNet p0, p0s, p1;
  if (c->ms.coarse_fine) {       // model0.onnx is a NeRF net here (src/models.py:199-277); probe its topology with the fp32 packing
    const NetShape shc = shape_of(c->ms.fp0, c->ms.fd0, c->ms.fp0, c->ms.fd0, 0, false);
    if (!pack_shading_net(n0, shc, Elem::F32, &p0, &err)) return bail(ADANERF_EIO, "model0.onnx: " + err);
    c->topoc = p0.topo;
    c->genericc = !p0.topo.is_default(true) || c->enc0 == kEncMax;
    if (opt->precision != ADANERF_PREC_FP32 && !pack_shading_net(n0, shc, elem_of(opt->precision), &p0, &err))
      return bail(ADANERF_EIO, "model0.onnx: " + err);
  } else {
    if (!pack_sampling_net(n0, sh, Elem::F32, &p0, &err)) return bail(ADANERF_EIO, "model0.onnx: " + err);
    if (p0.topo.bins != ms.bins)
      return bail(ADANERF_EIO, "model0.onnx has " + std::to_string(p0.topo.bins) + " outputs, config.ini says multiDepthFeatures = " + std::to_string(ms.bins));
    c->topo0 = p0.topo;
    c->generic0 = !p0.topo.is_default(false) || c->enc0 == kEncMax;
    // the split-precision packing: the ring-streamed kernel's for the 8 x 256 net, the run-time-shaped kernel's otherwise (not with raySampleInput,
    // not above width 256: such nets run the fp32 kernel in every sampling mode)
    if (has_split_sampling(c) && !pack_sampling_net(n0, sh, Elem::F16_SPLIT, &p0s, &err)) return bail(ADANERF_EIO, "model0.onnx: " + err);
    // a weight outside the fp16 range packs as +-inf: a 16-bit engine can return a finite, wrong row for it (pack.hpp).  Only the fp32 engine runs it.
    if (has_split_sampling(c) && opt->sampling_mode != ADANERF_SAMPLING_FP32 && !sampling_weights_fit_fp16(n0, &err))
      return bail(ADANERF_EUNSUPPORTED, "model0.onnx: " + err + " is outside the fp16 range (|w| < 65520) of the 16-bit sampling engines: use ADANERF_SAMPLING_FP32");
  }
  c->sampling_mode = opt->sampling_mode;
  c->model_dir = model_dir;
  if (const char* dbg = std::getenv("ADANERF_DEBUG_GUARD")) c->debug_guard = std::atoi(dbg);
  c->guard_audit_period = opt->guard_audit_period == 0 ? ADANERF_GUARD_AUDIT_PERIOD : std::max(opt->guard_audit_period, 0);
  c->ms.info.guard_audit_period = c->sampling_mode == ADANERF_SAMPLING_GUARDED ? c->guard_audit_period : 0;
  if (c->sampling_mode == ADANERF_SAMPLING_GUARDED) c->model0_hash = fnv1a64_file(join_path(model_dir, "model0.onnx"));
  {   // topology of the shading net first (fp32 packing accepts every supported topology)
    PackedNet probe;
    if (!pack_shading_net(c->net1_host, sh, Elem::F32, &probe, &err)) return bail(ADANERF_EIO, "model1.onnx: " + err);
    c->topo1 = probe.topo;
    c->generic1 = !probe.topo.is_default(true) || c->enc1 == kEncMax;
    if (opt->precision == ADANERF_PREC_FP32) p1 = std::move(probe);
    else if (!pack_shading_net(c->net1_host, sh, elem_of(opt->precision), &p1, &err)) return bail(ADANERF_EIO, "model1.onnx: " + err);
  }
  // the run-time-shaped kernels are instantiated for these widths (k_generic_f32.hip.hpp); the packer pads any width <= 512 up to one of them
  auto width_ok = [](int w) { return w == 64 || w == 128 || w == 256 || w == kWideWidth; };
  if (c->genericc && !width_ok(c->topoc.width)) return bail(ADANERF_EUNSUPPORTED, "model0.onnx: layer width " + std::to_string(c->topoc.width) + " (64, 128, 256 or 512 supported)");
  if (c->generic0 && !width_ok(c->topo0.width)) return bail(ADANERF_EUNSUPPORTED, "model0.onnx: layer width " + std::to_string(c->topo0.width) + " (64, 128, 256 or 512 supported)");
  if (c->generic1 && !width_ok(c->topo1.width)) return bail(ADANERF_EUNSUPPORTED, "model1.onnx: layer width " + std::to_string(c->topo1.width) + " (64, 128, 256 or 512 supported)");

  // ---- device ----
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
    return bail(ADANERF_EDEVICE, "no HIP device available: libadanerf_hip has no CPU fallback");
  if (hipSetDevice(opt->device_id) != hipSuccess) return bail(ADANERF_EDEVICE, "hipSetDevice failed");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, opt->device_id) != hipSuccess) return bail(ADANERF_EDEVICE, "hipGetDeviceProperties failed");
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return bail(ADANERF_EDEVICE, std::string("device is ") + prop.gcnArchName + "; this library is built for gfx950 (MI355X) only");
  c->ms.info.compute_units = c->grids.compute_units = prop.multiProcessorCount;
  c->device = opt->device_id;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(ADANERF_EDEVICE, "hipStreamCreate failed");
  c->stream = c->own_stream;

  rc = dev_alloc(c, &c->ztab, 2 * kBins * sizeof(float));
  if (rc) return bail(rc, c->err);
  float ztabs[2 * kBins];
  depth_table(ms, false, ztabs);
  depth_table(ms, true, ztabs + kBins);
  if (hipMemcpy(c->ztab.p, ztabs, sizeof(ztabs), hipMemcpyHostToDevice) != hipSuccess)
    return bail(ADANERF_EDEVICE, "ztab upload failed");
  if (c->ms.coarse_fine) {
    if ((rc = upload_net(c, p0, &c->netc[opt->precision]))) return bail(rc, c->err);
    if ((rc = dev_alloc(c, &c->ztab_coarse, kMaxCoarse * sizeof(float)))) return bail(rc, c->err);
    if (hipMemcpy(c->ztab_coarse.p, ms.ztab_coarse.data(), ms.ztab_coarse.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return bail(ADANERF_EDEVICE, "coarse depth table upload failed");
    c->spc = c->ms.sp;
    c->spc.normalize = ms.normalize0;
    c->ms.sp.unit_dir = 0;      // the fine pass encodes rays_d as RayMarchFromPoses handed it over: un-normalised under NDC (src/features.py:654-668)
    c->spc.ztab = reinterpret_cast<const float*>(c->ztab_coarse.p);
    c->genc = GenericTopo{c->topoc.depth, c->topoc.cat_mask, 0, 0, nullptr, 0.f};
  } else {
    if ((rc = upload_net(c, p0, &c->net0))) return bail(rc, c->err);
    if (has_split_sampling(c) && (rc = upload_net(c, p0s, &c->net0_split))) return bail(rc, c->err);
  }
  if (c->ms.ray_samples > 0) {
    if ((rc = dev_alloc(c, &c->rsi_z, ms.rsi_z.size() * sizeof(float)))) return bail(rc, c->err);
    if (hipMemcpy(c->rsi_z.p, ms.rsi_z.data(), ms.rsi_z.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
      return bail(ADANERF_EDEVICE, "raySampleInput depth table upload failed");
  }
  c->gen0 = GenericTopo{c->topo0.depth, 0, c->ms.ray_samples, p0.rsi_w_off, reinterpret_cast<const float*>(c->rsi_z.p), c->ms.cfg.depthRange[1]};
  c->gen1 = GenericTopo{c->topo1.depth, c->topo1.cat_mask, 0, 0, nullptr, 0.f};
  if ((rc = dev_alloc(c, &c->overflow, 64))) return bail(rc, c->err);
  if (hipMemset(c->overflow.p, 0, 64) != hipSuccess) return bail(ADANERF_EDEVICE, "hipMemset failed");
  if ((rc = upload_net(c, p1, &c->net1[opt->precision]))) return bail(rc, c->err);
  if ((rc = apply_selection(c))) return bail(rc, c->err);
  *out = c;
  return ADANERF_OK;
}

int adanerf_destroy(adanerf_ctx* c) {
  if (!c) return ADANERF_OK;
  (void)hipSetDevice(c->device);
  if (c->peer_event) (void)hipEventDestroy(c->peer_event);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
  for (int32_t* p : c->pinned_totals) (void)hipHostFree(p);
  if (c->guard_host) (void)hipHostFree(c->guard_host);
  if (c->guard_ev) (void)hipEventDestroy(c->guard_ev);
  const hipStream_t own = c->own_stream;
  delete c;      // frees every DevBuf
  if (own) (void)hipStreamDestroy(own);
  return ADANERF_OK;
}

int adanerf_get_info(const adanerf_ctx* c, adanerf_info* info) {
  if (!c || !info) return ADANERF_EINVAL;
  *info = c->ms.info;
  return ADANERF_OK;
}

int adanerf_set_camera(adanerf_ctx* c, const float pos[3], const float rot[9]) {
  if (!c) return ADANERF_EINVAL;
  if (!pos || !rot) return fail(c, ADANERF_EINVAL, "pos/rot == NULL");
  if (c->ms.pos_bound.active) {
    // bf16 shading: the layers were scaled for positions below kPosIdentityBound with the camera inside the view cell (setup_model); a pose far
    // outside it (a free-fly viewer) is refused rather than rendered with activations cut by the clamped conversion
    double d2 = 0.0;
    for (int i = 0; i < 3; ++i) d2 += (pos[i] - c->ms.pos_bound.center[i]) * (pos[i] - c->ms.pos_bound.center[i]);
    const double bound = c->ms.pos_bound.at(std::sqrt(d2));
    if (!(bound <= kPosIdentityBound)) {
      char msg[256];
      std::snprintf(msg, sizeof(msg), "camera %.3g away from the view-cell centre: sample positions can reach %.3g, beyond the %.0f the bf16 shading path's "
                    "layer scaling assumes -- create the context with precision fp16 or fp32 for such poses", std::sqrt(d2), bound, kPosIdentityBound);
      return fail(c, ADANERF_EUNSUPPORTED, msg);
    }
  }
  std::memcpy(c->ms.rg.pos, pos, 3 * sizeof(float));
  std::memcpy(c->ms.rg.rot, rot, 9 * sizeof(float));
  return ADANERF_OK;
}

int adanerf_set_selection(adanerf_ctx* c, int32_t num_samples, float threshold) {
  BIND(c);
  if (std::isnan(threshold)) return fail(c, ADANERF_EINVAL, "threshold is not a number (a negative value keeps the one in force)");
  if (threshold >= 0.f && c->ms.info.sampler_mode != ADANERF_SAMPLER_ADAPTIVE)
    return fail(c, ADANERF_EUNSUPPORTED, "this model's sampler takes no threshold (adanerf_create ignores options.threshold for it): pass a negative one");
  if (threshold == 0.f && has_budget_map(c))
    return fail(c, ADANERF_EUNSUPPORTED, "threshold 0 (dense) keeps every bin: remove the budget map first (adanerf_set_budget_map with two NULLs)");
  if (threshold == 0.f && c->depth_limit)
    return fail(c, ADANERF_EUNSUPPORTED, "threshold 0 (dense) keeps every bin with implicit keys: remove the depth limit first (adanerf_set_depth_limit with NULL)");
  if (threshold == 0.f && has_sample_cap(c))
    return fail(c, ADANERF_EUNSUPPORTED, "threshold 0 (dense) keeps every bin: remove the sample cap first (adanerf_set_sample_cap with 0)");
  ModelSetup& ms = c->ms;
  const adanerf_info was = ms.info;
  const ModelSetup::PosBound was_bound = ms.pos_bound;
  const int was_n = ms.sel_n;
  const float was_thr = ms.sel_thr;
  std::vector<float> was_ztab = ms.ztab;
  std::string err;
  if (int rc = select_samples(&ms, num_samples, threshold, &err)) return fail(c, rc, err);
  if (ms.info.num_samples == was.num_samples && ms.info.threshold == was.threshold) return ADANERF_OK;      // the pair in force: band and audit go on
  if (int rc = apply_selection(c)) {      // the buffers could not grow: back to the pair that renders
    ms.info = was;
    ms.pos_bound = was_bound;
    ms.sel_n = was_n;
    ms.sel_thr = was_thr;
    ms.ztab = std::move(was_ztab);
    return rc;
  }
  return ADANERF_OK;
}

int adanerf_set_frame_size(adanerf_ctx* c, int32_t width, int32_t height) {
  BIND(c);
  ModelSetup& ms = c->ms;
  const int w = width > 0 ? width : ms.info.width, h = height > 0 ? height : ms.info.height;
  if (w == ms.info.width && h == ms.info.height) return ADANERF_OK;      // the size in force: buffers, outputs and the audit go on
  const adanerf_info was = ms.info;
  const RayGenParams was_rg = ms.rg;
  std::string err;
  if (int rc = frame_geometry(&ms, &c->opt, w, h, &err)) return fail(c, rc, err);
  if (int rc = apply_frame_size(c, was.rays_local)) {      // the buffers could not grow: back to the size that renders
    ms.info = was;
    ms.rg = was_rg;
    return rc;
  }
  c->opt.width = w;
  c->opt.height = h;
  return ADANERF_OK;
}

int adanerf_set_pixel_offset(adanerf_ctx* c, float dx, float dy) {
  if (!c) return ADANERF_EINVAL;
  if (!(std::fabs(dx) <= 1.f) || !(std::fabs(dy) <= 1.f))      // also a NaN
    return fail(c, ADANERF_EINVAL, "adanerf_set_pixel_offset: dx and dy must be finite and within -1..1 (pixels)");
  c->px_dx = dx;
  c->px_dy = dy;
  return ADANERF_OK;
}

int adanerf_get_pixel_offset(const adanerf_ctx* c, float out[2]) {
  if (!c || !out) return ADANERF_EINVAL;
  out[0] = c->px_dx;
  out[1] = c->px_dy;
  return ADANERF_OK;
}

int adanerf_sync(adanerf_ctx* c) {
  BIND(c);
  HIP_RETURN(c, hipStreamSynchronize(c->stream));
}

int adanerf_ray_features(adanerf_ctx* c, int32_t first_ray, int32_t n_rays, float* d_feat, float* d_rays) {
  BIND(c);
  if (c->ms.coarse_fine) return fail(c, ADANERF_EUNSUPPORTED, "coarse/fine models have no sampling network");
  if (first_ray < 0 || n_rays < 0 || first_ray + n_rays > c->ms.info.rays_local) return fail(c, ADANERF_EINVAL, "ray range outside this context's rays");
  if (n_rays == 0) return ADANERF_OK;
  dim3 grid((n_rays + 255) / 256), block(256);
  const float* rz = reinterpret_cast<const float*>(c->rsi_z.p);
  const float d1 = c->ms.cfg.depthRange[1];
  hipLaunchKernelGGL(ray_features_kernel, grid, block, 0, c->stream, rg_in_force(c), first_ray, n_rays, d_feat, d_rays, c->ms.ray_samples, rz, d1, c->ms.fp0, c->ms.fd0);
  HIP_RETURN(c, hipGetLastError());
}

int adanerf_sample_mlp(adanerf_ctx* c, int32_t first_ray, int32_t n_rays, float* d_oracle, float* d_rays) {
  BIND(c);
  if (c->ms.coarse_fine) return fail(c, ADANERF_EUNSUPPORTED, "coarse/fine models have no sampling network (adanerf_sample_uniform / adanerf_shade_mlp_coarse)");
  if (first_ray < 0 || n_rays < 0 || first_ray + n_rays > c->ms.info.rays_local) return fail(c, ADANERF_EINVAL, "ray range outside this context's rays");
  return launch_sample_mlp(c, first_ray, n_rays, d_oracle, d_rays);
}

int adanerf_compact(adanerf_ctx* c, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr, int32_t* d_off, int32_t* d_cnt,
                    uint32_t* d_key, float* d_w, int32_t* d_total) {
  BIND(c);
  if (!d_oracle || !d_off || !d_cnt || !d_key || !d_w || !d_total) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0 || n_max < 1 || n_max > kBins || thr < 0.f) return fail(c, ADANERF_EINVAL, "n_rays/n_max/thr out of range");
  if (thr == 0.f && n_max != kBins) return fail(c, ADANERF_EINVAL, "dense mode (thr == 0) requires n_max == 128");
  if (static_cast<int64_t>(n_rays) >= (1ll << 25)) return fail(c, ADANERF_EINVAL, "n_rays must be < 2^25 per batch");
  if (static_cast<int64_t>(n_rays) * n_max > 0x7fffffffll) return fail(c, ADANERF_EINVAL, "n_rays * n_max exceeds 2^31 - 1");
  if (int rc = ensure_compact_scratch(c, n_rays, n_max)) return rc;
  return launch_compact(c, d_oracle, n_rays, n_max, thr, d_off, d_cnt, d_key, d_w, d_total);
}

int adanerf_compact_guarded(adanerf_ctx* c, const float* d_approx, const float* d_exact, int32_t n_rays, int32_t n_max, float thr, float eps,
                            float eps_pair, int32_t audit_period, int32_t audit_phase, int32_t audit_fill_cap, int32_t audit_cycle, int32_t* d_off,
                            int32_t* d_cnt, uint32_t* d_key, float* d_w, int32_t* d_total, int32_t* d_refined, uint32_t* d_monitor) {
  BIND(c);
  if (!d_approx || !d_exact || !d_off || !d_cnt || !d_key || !d_w || !d_total || !d_refined) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0 || n_max < 1 || n_max > kPairMaxN || !(thr > 0.f) || !(eps > 0.f)) return fail(c, ADANERF_EINVAL, "n_rays/n_max/thr/eps out of range");
  if (audit_period > 32 || (audit_period > 0 && (audit_period & (audit_period - 1)) != 0)) return fail(c, ADANERF_EINVAL, "audit_period must be a power of two <= 32");
  if (static_cast<int64_t>(n_rays) >= (1ll << 25)) return fail(c, ADANERF_EINVAL, "n_rays must be < 2^25 per batch");
  if (n_rays == 0) return ADANERF_OK;
  int rc = ensure_compact_scratch(c, n_rays, n_max);
  if (rc) return rc;
  const int n_words = (n_rays + 31) / 32;
  if (c->guard_mask.bytes < n_words * sizeof(uint32_t) || c->refine_list.bytes < static_cast<size_t>(n_rays) * sizeof(int32_t) ||
      c->guard_probe.bytes < static_cast<size_t>(n_rays) * 2 * sizeof(float)) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = dev_alloc(c, &c->guard_mask, n_words * sizeof(uint32_t)))) return rc;
    if ((rc = dev_alloc(c, &c->refine_list, static_cast<size_t>(n_rays) * sizeof(int32_t)))) return rc;
    if ((rc = dev_alloc(c, &c->guard_probe, static_cast<size_t>(n_rays) * 2 * sizeof(float)))) return rc;
  }
  const int period = audit_period > 0 ? audit_period : 0, phase = period ? (audit_phase & (period - 1)) : 0;
  SelectOut so = select_out(c, n_max, thr, d_cnt);
  so.guard_mask = reinterpret_cast<uint32_t*>(c->guard_mask.p);
  so.guard_eps = guard_band_of(c->ms.transform, eps);
  so.guard_pair = guard_pair_of(c->ms.transform, eps, eps_pair);
  so.audit_period = period;
  so.audit_phase = phase;
  so.guard_probe = reinterpret_cast<float*>(c->guard_probe.p);      // the cut values of the rays pass 2 will look at; their rows are d_approx itself
  const dim3 grid((n_rays + 127) / 128), block(256);
  hipLaunchKernelGGL(select_rows_kernel, grid, block, 0, c->stream, d_approx, n_rays, so, static_cast<const int32_t*>(nullptr));
  hipLaunchKernelGGL(refine_list_kernel, dim3((n_words + 255) / 256), dim3(256), 0, c->stream, reinterpret_cast<const uint32_t*>(c->guard_mask.p), n_words,
                     n_rays, period, phase, audit_fill_cap > 0 ? audit_fill_cap : 0, audit_cycle, reinterpret_cast<int32_t*>(c->refine_list.p), d_refined);
  so.guard_mask = nullptr;
  so.guard_band = eps;
  so.guard_band_pair = c->ms.transform == kOracleRaw ? so.guard_pair : 0.f;
  so.guard_eps = 0.f;
  so.guard_pair = 0.f;
  so.audit_period = 0;
  so.refine_list = reinterpret_cast<const int32_t*>(c->refine_list.p);
  so.guard_rows = d_monitor ? const_cast<float*>(d_approx) : nullptr;      // pass 2 only reads them
  so.guard_seen = d_monitor;
  hipLaunchKernelGGL(select_rows_kernel, grid, block, 0, c->stream, d_exact, n_rays, so, static_cast<const int32_t*>(d_refined));
  return launch_expand(c, n_rays, n_max, kPairSegShift, d_off, d_cnt, d_key, d_w, d_total);
}

int adanerf_calibrate_guard(adanerf_ctx* c, int32_t n_poses, uint32_t seed, int32_t set, float* max_diff, float* max_pair_diff) {
  BIND(c);
  return calibrate_guard(c, n_poses, seed, set != 0, max_diff, max_pair_diff);
}

int adanerf_guard_calibration_file(const adanerf_ctx* c, char* buf, size_t buf_bytes) {
  if (!c) return ADANERF_EINVAL;
  const std::string p = guard_record_path(guard_key(const_cast<adanerf_ctx*>(c)));
  if (buf && buf_bytes > 0) {
    const size_t n = std::min(p.size(), buf_bytes - 1);
    std::memcpy(buf, p.data(), n);
    buf[n] = 0;
  }
  return static_cast<int>(p.size() + 1);
}

int adanerf_abi_version(void) { return ADANERF_ABI_VERSION; }

int adanerf_struct_sizes(int32_t sizes_out[3]) {
  if (!sizes_out) return ADANERF_EINVAL;
  sizes_out[0] = static_cast<int32_t>(sizeof(adanerf_options));
  sizes_out[1] = static_cast<int32_t>(sizeof(adanerf_info));
  sizes_out[2] = static_cast<int32_t>(sizeof(adanerf_stats));
  return ADANERF_OK;
}

int adanerf_shade_features(adanerf_ctx* c, const float* d_rays, const uint32_t* d_key, int32_t n_samples, float* d_feat) {
  BIND(c);
  if (!d_rays || !d_key || !d_feat || n_samples < 0) return fail(c, ADANERF_EINVAL, "bad argument");
  if (n_samples == 0) return ADANERF_OK;
  ShadeArgs a{};
  a.sp = c->ms.sp;
  a.rays = d_rays;
  a.sample_key = d_key;
  a.max_samples = n_samples;
  hipLaunchKernelGGL(shade_features_kernel, dim3((n_samples + 255) / 256), dim3(256), 0, c->stream, a, d_feat, c->ms.fp1, c->ms.fd1);
  HIP_RETURN(c, hipGetLastError());
}

int adanerf_shade_mlp(adanerf_ctx* c, const float* d_rays, const uint32_t* d_key, const int32_t* d_total, int32_t max_samples,
                      int32_t precision, float* d_raw) {
  return adanerf_shade_mlp_z(c, d_rays, d_key, nullptr, d_total, max_samples, precision, d_raw);
}

int adanerf_shade_mlp_z(adanerf_ctx* c, const float* d_rays, const uint32_t* d_key, const float* d_z, const int32_t* d_total,
                        int32_t max_samples, int32_t precision, float* d_raw) {
  BIND(c);
  if (!d_rays || !d_key || !d_raw || max_samples < 0) return fail(c, ADANERF_EINVAL, "bad argument");
  return launch_shade_mlp(c, d_rays, d_key, d_total, max_samples, precision < 0 ? c->ms.info.precision : precision, d_raw, d_z);
}

int adanerf_sample_uniform(adanerf_ctx* c, int32_t first_ray, int32_t n_rays, float* d_rays, int32_t* d_off, int32_t* d_cnt, uint32_t* d_key,
                           int32_t* d_total) {
  BIND(c);
  if (!c->ms.coarse_fine) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_sample_uniform: not a coarse/fine model");
  if (!d_rays || !d_off || !d_cnt || !d_key || !d_total) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (first_ray < 0 || n_rays < 0 || first_ray + n_rays > c->ms.info.rays_local) return fail(c, ADANERF_EINVAL, "ray range outside this context's rays");
  int rc = launch_camera_rays(c, first_ray, n_rays, d_rays);
  return rc ? rc : launch_sample_uniform(c, n_rays, c->ms.n_coarse, d_off, d_cnt, d_key, d_total);
}

int adanerf_shade_mlp_coarse(adanerf_ctx* c, const float* d_rays, const uint32_t* d_key, const int32_t* d_total, int32_t max_samples,
                             int32_t precision, float* d_raw) {
  BIND(c);
  if (!c->ms.coarse_fine) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_shade_mlp_coarse: not a coarse/fine model");
  if (!d_rays || !d_key || !d_raw || max_samples < 0) return fail(c, ADANERF_EINVAL, "bad argument");
  return launch_shade_mlp(c, d_rays, d_key, d_total, max_samples, precision < 0 ? c->ms.info.precision : precision, d_raw, nullptr, true);
}

int adanerf_sample_from_coarse(adanerf_ctx* c, const float* d_raw_coarse, const float* d_rays, int32_t n_rays, int32_t* d_off, int32_t* d_cnt,
                               uint32_t* d_key, float* d_z, int32_t* d_total) {
  BIND(c);
  if (!c->ms.coarse_fine) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_sample_from_coarse: not a coarse/fine model");
  if (!d_raw_coarse || !d_rays || !d_off || !d_cnt || !d_key || !d_z || !d_total) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0 || static_cast<int64_t>(n_rays) * c->ms.info.num_samples > 0x7fffffffll || n_rays >= (1 << 25))
    return fail(c, ADANERF_EINVAL, "n_rays out of range");
  return launch_sample_fine(c, d_raw_coarse, d_rays, n_rays, d_off, d_cnt, d_key, d_z, d_total);
}

int adanerf_sample_pdf(adanerf_ctx* c, const float* d_oracle, int32_t n_rays, int32_t n, int32_t* d_off, int32_t* d_cnt, uint32_t* d_key,
                       float* d_w, float* d_z, int32_t* d_total) {
  BIND(c);
  if (!d_oracle || !d_off || !d_cnt || !d_key || !d_w || !d_z || !d_total) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0 || n < 1 || n > 4096) return fail(c, ADANERF_EINVAL, "n_rays/n out of range");
  if (static_cast<int64_t>(n_rays) * n > 0x7fffffffll || n_rays >= (1 << 25)) return fail(c, ADANERF_EINVAL, "n_rays * n too large");
  return launch_sample_pdf(c, d_oracle, n_rays, n, d_off, d_cnt, d_key, d_w, d_z, d_total);
}

int adanerf_composite_classic(adanerf_ctx* c, const float* d_raw, const float* d_z, const float* d_rays, int32_t n_rays, int32_t n,
                              float* d_rgb, void* d_rgba8) {
  BIND(c);
  if (!d_raw || !d_z || !d_rays || n_rays < 0 || n < 1) return fail(c, ADANERF_EINVAL, "bad argument");
  return launch_composite_classic(c, d_raw, d_z, d_rays, n_rays, n, d_rgb, d_rgba8);
}

int adanerf_composite(adanerf_ctx* c, const float* d_raw, const float* d_w, const int32_t* d_off, const int32_t* d_cnt, int32_t n_rays,
                      float* d_rgb, void* d_rgba8) {
  BIND(c);
  if (!d_raw || !d_w || !d_off || !d_cnt || n_rays < 0) return fail(c, ADANERF_EINVAL, "bad argument");
  return launch_composite(c, d_raw, d_w, d_off, d_cnt, n_rays, d_rgb, d_rgba8);
}

int adanerf_composite_aux(adanerf_ctx* c, const float* d_raw, const float* d_w, const int32_t* d_off, const int32_t* d_cnt, const uint32_t* d_key,
                          int32_t n_rays, float* d_rgb, void* d_rgba8, float* d_depth, float* d_acc) {
  BIND(c);
  if (!d_raw || !d_w || !d_off || !d_cnt || n_rays < 0) return fail(c, ADANERF_EINVAL, "bad argument");
  if (!d_key && !c->ms.info.dense && (d_depth || d_acc))      // launch_composite would leave the maps unwritten
    return fail(c, ADANERF_EINVAL, "adanerf_composite_aux: a depth or acc map needs d_sample_key unless the context is dense (threshold 0)");
  return launch_composite(c, d_raw, d_w, d_off, d_cnt, n_rays, d_rgb, d_rgba8, d_key, d_depth, d_acc);
}

int adanerf_composite_classic_aux(adanerf_ctx* c, const float* d_raw, const float* d_z, const float* d_rays, int32_t n_rays, int32_t n,
                                  float* d_rgb, void* d_rgba8, float* d_depth, float* d_acc) {
  BIND(c);
  if (!d_raw || !d_z || !d_rays || n_rays < 0 || n < 1) return fail(c, ADANERF_EINVAL, "bad argument");
  return launch_composite_classic(c, d_raw, d_z, d_rays, n_rays, n, d_rgb, d_rgba8, d_depth, d_acc);
}

int adanerf_disp_map(adanerf_ctx* c, const float* d_depth, const float* d_acc, int32_t n, float* d_disp) {
  BIND(c);
  if (!d_depth || !d_acc || !d_disp || n < 0) return fail(c, ADANERF_EINVAL, "adanerf_disp_map: NULL buffer or n < 0");
  if (n == 0) return ADANERF_OK;
  hipLaunchKernelGGL(disp_map_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_depth, d_acc, n, d_disp);
  HIP_RETURN(c, hipGetLastError());
}

namespace {

constexpr size_t kMaxProfiledBatches = 1 << 16;

void reset_record(adanerf_ctx* c) {
  c->events_used = 0;
  c->prof_frames = 0;
  c->folded = adanerf_stats{};
}

int sum_stats(adanerf_ctx* c, adanerf_stats* stats) {
  std::memset(stats, 0, sizeof(*stats));
  const size_t nb = c->events_used / 5;
  for (size_t b = 0; b < nb; ++b) {
    hipEvent_t* ev = &c->events[b * 5];
    float t;
    HIP_TRY(c, hipEventElapsedTime(&t, ev[0], ev[1]));
    stats->ms_sample_mlp += t;
    HIP_TRY(c, hipEventElapsedTime(&t, ev[1], ev[2]));
    stats->ms_compact += t;
    HIP_TRY(c, hipEventElapsedTime(&t, ev[2], ev[3]));
    stats->ms_shade_mlp += t;
    HIP_TRY(c, hipEventElapsedTime(&t, ev[3], ev[4]));
    stats->ms_composite += t;
    HIP_TRY(c, hipEventElapsedTime(&t, ev[0], ev[4]));
    stats->ms_total += t;
    const int32_t* tot = c->pinned_totals[b];
    stats->total_samples += tot[kTotalSamples];
    if (c->sampling_mode == ADANERF_SAMPLING_GUARDED) {
      stats->rays_refined += tot[kTotalRefined];
      const int32_t* gs = tot + kTotalGuardSeen;       // cumulative on the device: the latest batch holds the running values
      float seen, pair;                                // (the two largest errors are float bits)
      std::memcpy(&seen, &gs[kSeenMax], sizeof(seen));
      std::memcpy(&pair, &gs[kSeenPair], sizeof(pair));
      stats->guard_max_seen = std::max(stats->guard_max_seen, seen);
      stats->guard_pair_seen = std::max(stats->guard_pair_seen, pair);
      stats->guard_violations = std::max(stats->guard_violations, gs[kSeenViolations]);
      stats->guard_audit_mismatch = std::max(stats->guard_audit_mismatch, gs[kSeenAuditMismatch]);
      stats->guard_audited = std::max(stats->guard_audited, gs[kSeenAudited]);
    }
  }
  int32_t ovf = 0;
  HIP_TRY(c, hipMemcpy(&ovf, c->overflow.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  stats->sampling_overflow = ovf;
  stats->batches = static_cast<int32_t>(nb);
  stats->shade_launches = static_cast<int32_t>(nb);
  stats->sample_launches = static_cast<int32_t>(nb);
  // plus whatever an earlier, full event pool was folded into
  const adanerf_stats& f = c->folded;
  stats->total_samples += f.total_samples;
  stats->rays_refined += f.rays_refined;
  stats->guard_max_seen = std::max(stats->guard_max_seen, f.guard_max_seen);
  stats->guard_violations = std::max(stats->guard_violations, f.guard_violations);
  stats->guard_pair_seen = std::max(stats->guard_pair_seen, f.guard_pair_seen);
  stats->guard_audit_mismatch = std::max(stats->guard_audit_mismatch, f.guard_audit_mismatch);
  stats->guard_audited = std::max(stats->guard_audited, f.guard_audited);
  stats->guard_widened = c->guard_widened;
  stats->ms_total += f.ms_total;
  stats->ms_sample_mlp += f.ms_sample_mlp;
  stats->ms_compact += f.ms_compact;
  stats->ms_shade_mlp += f.ms_shade_mlp;
  stats->ms_composite += f.ms_composite;
  stats->batches += f.batches;
  stats->shade_launches += f.shade_launches;
  stats->sample_launches += f.sample_launches;
  return ADANERF_OK;
}

}  // namespace

int adanerf_copy_result_sampling_network(adanerf_ctx* c, const float* d_oracle, int32_t n_rays, void* d_rgba8) {
  BIND(c);
  if (!d_oracle || !d_rgba8) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0) return fail(c, ADANERF_EINVAL, "n_rays out of range");
  if (n_rays == 0) return ADANERF_OK;
  hipLaunchKernelGGL(oracle_view_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, c->stream, d_oracle, n_rays, static_cast<uchar4*>(d_rgba8));
  HIP_RETURN(c, hipGetLastError());
}

int adanerf_render_oracle(adanerf_ctx* c, void* d_rgba8) {
  BIND(c);
  if (!d_rgba8) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (c->ms.coarse_fine) return fail(c, ADANERF_EUNSUPPORTED, "coarse/fine models have no sampling network to view");
  const int R = c->ms.info.rays_local, B = c->ms.info.batch_rays;
  int rc = ensure_batch_buffers(c, std::min(B, std::max(R, 1)), c->ms.info.num_samples);
  if (rc) return rc;
  float* rays = reinterpret_cast<float*>(c->rays.p);
  float* oracle = reinterpret_cast<float*>(c->oracle.p);
  for (int first = 0; first < R; first += B) {
    const int n = std::min(B, R - first);
    if ((rc = launch_sample_mlp(c, first, n, oracle, rays))) return rc;
    if ((rc = adanerf_copy_result_sampling_network(c, oracle, n, static_cast<char*>(d_rgba8) + static_cast<size_t>(first) * 4))) return rc;
  }
  return ADANERF_OK;
}

namespace {

// The band of the guarded selection rests on two measured assumptions (|fp16 output - split output| <= guard_eps on every raw
// output; the error of a (kept - candidate) difference <= guard_eps_pair) that the second pass re-measures on the whole row of every
// re-evaluated ray, and on an audit of the outcome (decided rays re-evaluated anyway).  All of it in RAW-output units -- the units
// guard_eps is in (round 3 compared transformed values with a raw band).  If a frame saw a bound violated, every later frame runs
// with ADANERF_GUARD_CALIB_MARGIN x the largest errors seen so far; an audit mismatch without a violated bound (the rule itself would
// be wrong) falls back to the doubled single-value bound with no pair bound.  adanerf_info follows, adanerf_stats.guard_widened
// counts.  Non-blocking: looks only at a copy that has already arrived.
void poll_guard(adanerf_ctx* c) {
  if (!c->guard_ev_pending) return;
  const hipError_t q = hipEventQuery(c->guard_ev);
  (void)hipGetLastError();      // hipErrorNotReady is not a failure of this context
  if (q != hipSuccess) return;
  c->guard_ev_pending = false;
  float seen, pair;
  std::memcpy(&seen, &c->guard_host[kSeenMax], sizeof(seen));
  std::memcpy(&pair, &c->guard_host[kSeenPair], sizeof(pair));
  const int viol = c->guard_host[kSeenViolations], mism = c->guard_host[kSeenAuditMismatch];
  if (c->guard_ev_stale) {      // frames of the (N, threshold) before adanerf_set_selection: counted, but their band is gone
    c->guard_ev_stale = false;
    c->guard_viol_seen = std::max(c->guard_viol_seen, viol);
    c->guard_mism_seen = std::max(c->guard_mism_seen, mism);
    return;
  }
  bool widened = false;
  if (viol > c->guard_viol_seen) {
    c->guard_viol_seen = viol;
    if (seen > c->guard_eps) {
      // the bound on single values was exceeded: widen it, and drop the measured pair bound -- it was measured over the candidates
      // the narrower band defined; 2 x the new bound is what holds by construction
      c->guard_eps = ADANERF_GUARD_CALIB_MARGIN * seen;
      c->guard_eps_pair = 2.0f * c->guard_eps;
      widened = true;
    } else if (pair > c->guard_eps_pair) {
      c->guard_eps_pair = ADANERF_GUARD_CALIB_MARGIN * pair;
      widened = true;
    }
  }
  if (mism > c->guard_mism_seen) {
    c->guard_mism_seen = mism;
    if (!widened) {
      c->guard_eps *= 2.0f;
      c->guard_eps_pair = 2.0f * c->guard_eps;
      widened = true;
    }
  }
  if (widened) {
    c->guard_eps_pair = std::min(std::max(c->guard_eps_pair, ADANERF_GUARD_EPS_MIN), 2.0f * c->guard_eps);
    c->ms.info.guard_eps = c->guard_eps;
    c->ms.info.guard_eps_pair = c->guard_eps_pair;
    c->ms.info.guard_calib_source = ADANERF_GUARD_FROM_MONITOR;
    ++c->guard_widened;
  }
}

// The three parts of a frame that adanerf_render and adanerf_render_masked share: the profiling record opened for n_batches batches
// (begin_record), one batch through every stage (render_batch), the record closed and summed into the caller's stats (end_record).

// *record: the frame's batches record events and the image of `total`
int begin_record(adanerf_ctx* c, adanerf_stats* stats, int n_batches, bool* record_out) {
  int rc;
  if (stats && c->profiling && c->events_used) {   // a synchronous call starts a fresh record
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    reset_record(c);
  }
  // a single frame of more batches than the event pool may hold is rendered without per-stage timing (stats then carry the
  // sample totals of nothing and zero times) rather than growing the pool without bound
  const bool record = (stats || c->profiling) && static_cast<size_t>(n_batches) <= kMaxProfiledBatches;
  if (record && c->events_used && c->events_used / 5 + n_batches > kMaxProfiledBatches) {
    // the event pool is full: fold what it holds into the running record (one synchronisation per 65 536 batches)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    adanerf_stats part;
    if ((rc = sum_stats(c, &part))) return rc;
    c->folded = part;
    c->events_used = 0;
  }
  if (record) {
    const size_t need = c->events_used + static_cast<size_t>(n_batches) * 5;
    while (c->events.size() < need) {
      hipEvent_t e;
      HIP_TRY(c, hipEventCreate(&e));
      c->events.push_back(e);
    }
    while (c->pinned_totals.size() < need / 5) {
      int32_t* p = nullptr;
      HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&p), kTotalSlots * sizeof(int32_t), hipHostMallocDefault));   // image of the `total` block
      std::memset(p, 0, kTotalSlots * sizeof(int32_t));
      c->pinned_totals.push_back(p);
    }
  }
  *record_out = record;
  return ADANERF_OK;
}

// Where the pixels of a batch go: the batch's part of the caller's images (adanerf_render), or staging buffers (adanerf_render_masked).
// depth / acc null with disp set: the disparity's two inputs go through the context's scratch.
struct BatchOut {
  float* rgb;
  void* rgba8;
  float* depth;
  float* acc;
  float* disp;
};

// Rays [first, first + n) of the context's rays -- or, with a list, the n rays list->ids[0 .. n) -- through every stage, on the context's stream.
int render_batch(adanerf_ctx* c, int first, int n, const RayList* list, const BatchOut& out, bool record) {
  const int B = c->ms.info.batch_rays, N = c->ms.info.num_samples;
  const float thr = c->ms.info.threshold;
  const bool budget = has_budget_map(c);      // adaptive sampler, threshold > 0 (adanerf_set_budget_map / adanerf_set_selection see to it)
  int rc;
  float* rays = reinterpret_cast<float*>(c->rays.p);
  float* oracle = reinterpret_cast<float*>(c->oracle.p);
  int32_t* off = reinterpret_cast<int32_t*>(c->ray_offsets.p);
  const bool cfm = c->ms.coarse_fine;
  int32_t* cnt = reinterpret_cast<int32_t*>(c->ray_counts.p);
  uint32_t* key = reinterpret_cast<uint32_t*>(c->sample_key.p);
  float* sw = reinterpret_cast<float*>(c->sample_w.p);
  float* raw = reinterpret_cast<float*>(c->raw.p);
  int32_t* total = reinterpret_cast<int32_t*>(c->total.p);
  hipEvent_t* ev = record ? &c->events[c->events_used] : nullptr;
  if (ev) HIP_TRY(c, hipEventRecord(ev[0], c->stream));
  const bool pdf = c->ms.info.sampler_mode == ADANERF_SAMPLER_PDF || cfm;      // explicit sample depths + classic compositing
  if (cfm) {
    // vanilla NeRF: camera rays, Nc uniform samples, coarse network ("sample_mlp" in the statistics: the first network)
    uint32_t* keyc = reinterpret_cast<uint32_t*>(c->key_coarse.p);
    float* rawc = reinterpret_cast<float*>(c->raw_coarse.p);
    if ((rc = launch_camera_rays(c, first, n, rays))) return rc;
    if ((rc = launch_sample_uniform(c, n, c->ms.n_coarse, off, cnt, keyc, total))) return rc;
    if ((rc = launch_shade_mlp(c, rays, keyc, total, n * c->ms.n_coarse, c->ms.info.precision, rawc, nullptr, true))) return rc;
    if (ev) HIP_TRY(c, hipEventRecord(ev[1], c->stream));
    // weights -> pdf -> Nf more depths, merged with the Nc coarse ones ("compact")
    if ((rc = launch_sample_fine(c, rawc, rays, n, off, cnt, key, reinterpret_cast<float*>(c->sample_z.p), total))) return rc;
  }
  // adaptive selection in the epilogue of the sampling kernel: the [R,128] oracle values never reach HBM
  const bool fused = !pdf && thr > 0.f && use_pair_select(c, N) && c->sampling_mode != ADANERF_SAMPLING_FP32 && (!c->generic0 || generic_split_sampling(c)) &&
                     !(c->opt.flags & ADANERF_FLAG_KEEP_ORACLE);
  const SelectOut so = select_out(c, N, thr, cnt);
  const BudgetMaps bm{c->budget_n, c->budget_thr, first};
  // adaptive sampler, threshold > 0, no NDC (adanerf_set_depth_limit / adanerf_set_selection see to it); the pose in force reaches the kernel by value
  const bool limited = c->depth_limit != nullptr;
  // adaptive sampler, threshold > 0 (adanerf_set_sample_cap / adanerf_set_selection see to it); the bound is on this batch's own rays
  const bool capped = cap_trims(c) && !pdf && thr > 0.f;
  const int64_t cap_total = capped ? cap_total_of(c, n) : 0;
  const DepthLimit dl{c->depth_limit, first, list ? list->ids : nullptr, rays, c->ms.sp.ztab, depth_pose(c->ms.rg.pos, c->ms.rg.rot)};
  if (!cfm && (rc = launch_sample_mlp(c, first, n, fused ? nullptr : oracle, rays, fused ? &so : nullptr, list))) return rc;
  if (ev && !cfm) HIP_TRY(c, hipEventRecord(ev[1], c->stream));
  float* sz = reinterpret_cast<float*>(c->sample_z.p);
  if (cfm) rc = ADANERF_OK;
  else if (pdf) rc = launch_sample_pdf(c, oracle, n, N, off, cnt, key, sw, sz, total);
  else if (fused) {
    rc = budget ? launch_trim(c, bm, n, N, thr, kPairSegShift, cnt) : ADANERF_OK;
    if (!rc && limited) rc = launch_depth_limit(c, dl, n, N, kPairSegShift, cnt);
    if (!rc && capped) rc = launch_cap(c, n, N, thr, kPairSegShift, cnt, cap_total);
    if (!rc) rc = launch_expand(c, n, N, kPairSegShift, off, cnt, key, sw, total);
  }
  else if (thr == 0.f) {      // dense: implicit keys, the oracle buffer is the weight array (dense_offsets_kernel)
    hipLaunchKernelGGL(dense_offsets_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, off, cnt, total);
    HIP_TRY(c, hipGetLastError());
  } else rc = launch_compact(c, oracle, n, N, thr, off, cnt, key, sw, total, budget ? &bm : nullptr, limited ? &dl : nullptr, capped ? &cap_total : nullptr);
  if (rc) return rc;
  const bool dense_implicit = !cfm && !pdf && !fused && thr == 0.f;
  const uint32_t* key_s = dense_implicit ? nullptr : key;
  const float* sw_s = dense_implicit ? oracle : sw;
  if (ev) HIP_TRY(c, hipEventRecord(ev[2], c->stream));
  const int64_t max_s = static_cast<int64_t>(n) * N;   // <= INT32_MAX: checked by setup_model
  if ((rc = launch_shade_mlp(c, rays, key_s, total, static_cast<int>(max_s), c->ms.info.precision, raw, pdf ? sz : nullptr))) return rc;
  if (ev) HIP_TRY(c, hipEventRecord(ev[3], c->stream));
  float* depth_b = out.depth;
  float* acc_b = out.acc;
  if (out.disp && (!depth_b || !acc_b)) {      // disparity needs both maps of the batch
    if ((rc = dev_alloc(c, &c->disp_scratch, static_cast<size_t>(B) * 2 * sizeof(float)))) return rc;
    if (!depth_b) depth_b = reinterpret_cast<float*>(c->disp_scratch.p);
    if (!acc_b) acc_b = reinterpret_cast<float*>(c->disp_scratch.p) + B;
  }
  if (pdf) rc = launch_composite_classic(c, raw, sz, rays, n, N, out.rgb, out.rgba8, depth_b, acc_b);
  else rc = launch_composite(c, raw, sw_s, off, cnt, n, out.rgb, out.rgba8, key_s, depth_b, acc_b);
  if (rc) return rc;
  if (out.disp && n > 0) {
    hipLaunchKernelGGL(disp_map_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, depth_b, acc_b, n, out.disp);
    HIP_TRY(c, hipGetLastError());
  }
  if (ev) {
    HIP_TRY(c, hipEventRecord(ev[4], c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->pinned_totals[c->events_used / 5], total, kTotalSlots * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    c->events_used += 5;
  }
  return ADANERF_OK;
}

// stats of the frame's n_batches batches (synchronous) when the caller asked for them; `rays`: what the frame rendered
int end_record(adanerf_ctx* c, adanerf_stats* stats, int n_batches, bool record, int rays) {
  if (record) c->prof_frames++;
  if (stats) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    poll_guard(c);
    if (int rc = sum_stats(c, stats)) return rc;
    stats->rays = rays;
    if (n_batches > 0 && record) {   // wall span of this frame, first launch -> last kernel end
      const size_t e0 = c->events_used - static_cast<size_t>(n_batches) * 5;
      HIP_TRY(c, hipEventElapsedTime(&stats->ms_total, c->events[e0], c->events[c->events_used - 1]));
    }
    reset_record(c);
  }
  return ADANERF_OK;
}

}  // namespace

int adanerf_render(adanerf_ctx* c, void* d_rgba8, float* d_rgb, adanerf_stats* stats) {
  BIND(c);
  poll_guard(c);
  const int R = c->ms.info.rays_local, B = c->ms.info.batch_rays, N = c->ms.info.num_samples;
  const int n_batches = R > 0 ? (R + B - 1) / B : 0;
  const bool budget = has_budget_map(c) || has_sample_cap(c);      // the trims that read values: a guarded context renders as the split engine
  int rc = ensure_batch_buffers(c, std::min(B, std::max(R, 1)), N);
  if (rc) return rc;
  if (has_sample_cap(c)) c->cap_record_live = cap_trims(c);      // a cap at or above N launches nothing: its report is the empty one
  if (cap_trims(c)) {      // the report covers this frame
    if ((rc = ensure_cap_buffers(c, std::min(B, std::max(R, 1))))) return rc;
    hipLaunchKernelGGL(cap_reset_kernel, dim3(1), dim3(1), 0, c->stream, reinterpret_cast<CapRecord*>(c->cap_record.p));
    HIP_TRY(c, hipGetLastError());
  }
  bool record = false;
  if ((rc = begin_record(c, stats, n_batches, &record))) return rc;
  int32_t* total = reinterpret_cast<int32_t*>(c->total.p);
  for (int b = 0; b < n_batches; ++b) {
    const int first = b * B, n = std::min(B, R - first);
    const BatchOut out{d_rgb ? d_rgb + static_cast<size_t>(first) * 3 : nullptr, d_rgba8 ? static_cast<char*>(d_rgba8) + static_cast<size_t>(first) * 4 : nullptr,
                       c->aux_depth ? c->aux_depth + first : nullptr, c->aux_acc ? c->aux_acc + first : nullptr, c->aux_disp ? c->aux_disp + first : nullptr};
    if ((rc = render_batch(c, first, n, nullptr, out, record))) return rc;
  }
  // under a budget map or a sample cap the guarded mode renders as the split engine: no audit to move on, no monitor to read
  if (c->sampling_mode == ADANERF_SAMPLING_GUARDED && c->guard_mask.p && n_batches > 0 && !budget) ++c->guard_frame;      // the audit moves on
  if (c->sampling_mode == ADANERF_SAMPLING_GUARDED && c->guard_mask.p && n_batches > 0 && !budget && !c->guard_ev_pending) {
    if (!c->guard_host) {
      HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->guard_host), 8 * sizeof(int32_t)));
      std::memset(c->guard_host, 0, 8 * sizeof(int32_t));
      HIP_TRY(c, hipEventCreateWithFlags(&c->guard_ev, hipEventDisableTiming));
    }
    HIP_TRY(c, hipMemcpyAsync(c->guard_host, total + kTotalGuardSeen, kGuardSeenSlots * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->guard_ev, c->stream));
    c->guard_ev_pending = true;
  }
  return end_record(c, stats, n_batches, record, R);
}

namespace {

// adanerf_render_masked's own buffers: bit words, list and count for a frame of R rays; staging for a listed batch of n rays
int ensure_mask_buffers(adanerf_ctx* c, int R, int n) {
  const size_t words = (static_cast<size_t>(R) + 31) / 32;
  if (c->mask_bits.bytes < words * sizeof(uint32_t) || c->ray_list.bytes < static_cast<size_t>(R) * sizeof(int32_t) || !c->ray_list_count.p || n > c->stage_cap) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // a masked call in flight may still use the smaller ones
    n = std::max(n, c->stage_cap);
    const size_t S = static_cast<size_t>(n);
    int rc;
    if ((rc = dev_alloc(c, &c->mask_bits, std::max(words, size_t(4)) * sizeof(uint32_t)))) return rc;
    if ((rc = dev_alloc(c, &c->ray_list, static_cast<size_t>(std::max(R, 1)) * sizeof(int32_t)))) return rc;
    if ((rc = dev_alloc(c, &c->ray_list_count, 64))) return rc;
    if ((rc = dev_alloc(c, &c->stage_rgba8, std::max(S, size_t(1)) * 4))) return rc;
    if ((rc = dev_alloc(c, &c->stage_rgb, std::max(S, size_t(1)) * 3 * sizeof(float)))) return rc;
    if ((rc = dev_alloc(c, &c->stage_aux, std::max(S, size_t(1)) * 3 * sizeof(float)))) return rc;
    c->stage_cap = n;
  }
  return ADANERF_OK;
}

}  // namespace

int adanerf_render_masked(adanerf_ctx* c, const uint8_t* d_mask, uint32_t values, void* d_rgba8, float* d_rgb, adanerf_stats* stats, int32_t* n_rendered) {
  if (!c) return ADANERF_EINVAL;
  if (!d_mask) return fail(c, ADANERF_EINVAL, "adanerf_render_masked: NULL mask");
  if (!d_rgba8 && !d_rgb) return fail(c, ADANERF_EINVAL, "adanerf_render_masked: both colour outputs NULL");
  if (values == 0) return fail(c, ADANERF_EINVAL, "adanerf_render_masked: values == 0 selects no mask byte");
  const int R = c->ms.info.rays_local, B = c->ms.info.batch_rays, N = c->ms.info.num_samples;
  const auto refuse = [&](const char* why) { return fail(c, ADANERF_EUNSUPPORTED, std::string("adanerf_render_masked: ") + why); };
  if (c->ms.coarse_fine) return refuse("the coarse / fine sampler has no ray list");
  if (c->ms.info.sampler_mode == ADANERF_SAMPLER_PDF) return refuse("the PDF sampler has no ray list");
  if (c->generic0) return refuse("run-time-shaped sampling networks have no ray list (the 8 x 256 network only)");
  if (c->sampling_mode != ADANERF_SAMPLING_SPLIT_FP16 && c->sampling_mode != ADANERF_SAMPLING_GUARDED)
    return refuse("sampling modes fp16 and fp32 have no ray list (split_fp16 or guarded only)");
  if (!(c->ms.info.threshold > 0.f)) return refuse("a dense context (threshold 0) has no fused selection");
  if (!use_pair_select(c, N) || (c->opt.flags & ADANERF_FLAG_KEEP_ORACLE))
    return refuse("the ray list needs the fused selection (N <= 16, neither ADANERF_FLAG_KEEP_ORACLE nor ADANERF_FLAG_WAVE_SELECT)");
  if (has_budget_map(c)) return refuse("a budget map is installed: its maps are indexed by frame position (remove it first)");
  if (has_sample_cap(c)) return refuse("a sample cap is installed: its threshold depends on which rays share a batch (adanerf_set_sample_cap(ctx, 0) removes it)");
  if (c->ms.rg.world != 1) return refuse("whole frames only (shard_world must be 1)");
  BIND(c);
  if (n_rendered) *n_rendered = 0;
  if (R <= 0) return ADANERF_OK;
  int rc = ensure_mask_buffers(c, R, 0);
  if (rc) return rc;
  // mask -> bit words -> ascending list + count (refine_list_kernel without an audit: the set bits, in order), then M comes back once
  const int n_words = (R + 31) / 32, n_halves = 2 * n_words;
  int32_t* ids = reinterpret_cast<int32_t*>(c->ray_list.p);
  int32_t* count = reinterpret_cast<int32_t*>(c->ray_list_count.p);
  hipLaunchKernelGGL(mask_bits_kernel, dim3((n_halves + 255) / 256), dim3(256), 0, c->stream, d_mask, R, values,
                     (reinterpret_cast<uintptr_t>(d_mask) & 15) == 0 ? 1 : 0, n_halves, reinterpret_cast<uint16_t*>(c->mask_bits.p));
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(refine_list_kernel, dim3((n_words + 255) / 256), dim3(256), 0, c->stream, reinterpret_cast<const uint32_t*>(c->mask_bits.p), n_words, R, 0, 0, 0,
                     0, ids, count);
  HIP_TRY(c, hipGetLastError());
  int32_t M = 0;
  HIP_TRY(c, hipMemcpyAsync(&M, count, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (M < 0 || M > R) return fail(c, ADANERF_EDEVICE, "adanerf_render_masked: the list count is outside 0..rays_local");
  if (n_rendered) *n_rendered = M;
  const int chunk = std::min(M, B), n_batches = M > 0 ? (M + B - 1) / B : 0;
  if (M > 0) {
    if ((rc = ensure_batch_buffers(c, chunk, N))) return rc;
    if ((rc = ensure_mask_buffers(c, R, chunk))) return rc;
    // a guarded context renders the list as the split engine: the count of re-evaluated rays goes to 0 in stream order (only a guarded
    // frame writes it), as under a budget map; guard_frame, the band and the monitor's running values stay
    if (c->sampling_mode == ADANERF_SAMPLING_GUARDED)
      HIP_TRY(c, hipMemsetAsync(reinterpret_cast<int32_t*>(c->total.p) + kTotalRefined, 0, sizeof(int32_t), c->stream));
  }
  bool record = false;
  if ((rc = begin_record(c, stats, n_batches, &record))) return rc;
  const bool want_depth = c->aux_depth || c->aux_disp, want_acc = c->aux_acc || c->aux_disp;
  float* aux = reinterpret_cast<float*>(c->stage_aux.p);
  for (int b = 0; b < n_batches; ++b) {
    const int at = b * B, n = std::min(B, M - at);
    const RayList list{ids + at, count};      // *count = M >= n: the kernel's own bound is n
    const BatchOut out{d_rgb ? reinterpret_cast<float*>(c->stage_rgb.p) : nullptr, d_rgba8 ? c->stage_rgba8.p : nullptr, want_depth ? aux : nullptr,
                       want_acc ? aux + c->stage_cap : nullptr, c->aux_disp ? aux + 2 * static_cast<size_t>(c->stage_cap) : nullptr};
    if ((rc = render_batch(c, 0, n, &list, out, record))) return rc;
    MaskScatter s{};
    s.list = list.ids;
    s.rgba8 = static_cast<const uint32_t*>(out.rgba8);
    s.rgb = out.rgb;
    s.depth = out.depth;
    s.acc = out.acc;
    s.disp = out.disp;
    s.o_rgba8 = static_cast<uint32_t*>(d_rgba8);
    s.o_rgb = d_rgb;
    s.o_depth = c->aux_depth;
    s.o_acc = c->aux_acc;
    s.o_disp = c->aux_disp;
    hipLaunchKernelGGL(mask_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, s, n);
    HIP_TRY(c, hipGetLastError());
  }
  return end_record(c, stats, n_batches, record, M);
}

int adanerf_set_aux_outputs(adanerf_ctx* c, float* d_depth_map, float* d_acc_map) {
  BIND(c);
  c->aux_depth = d_depth_map;
  c->aux_acc = d_acc_map;
  return ADANERF_OK;
}

int adanerf_set_disp_output(adanerf_ctx* c, float* d_disp_map) {
  BIND(c);
  c->aux_disp = d_disp_map;
  return ADANERF_OK;
}

int adanerf_set_budget_map(adanerf_ctx* c, const uint8_t* d_n_map, const float* d_thr_map) {
  BIND(c);
  if (d_n_map || d_thr_map) {
    if (c->ms.coarse_fine || c->ms.info.sampler_mode != ADANERF_SAMPLER_ADAPTIVE)
      return fail(c, ADANERF_EUNSUPPORTED, "per-ray budgets trim the adaptive selection: this model's sampler has none");
    if (c->ms.info.dense) return fail(c, ADANERF_EUNSUPPORTED, "threshold 0 (dense) keeps every bin: there is no selection to trim");
  }
  // a guarded context renders as the split engine while a map is installed: the per-frame count of re-evaluated rays goes back to 0 in
  // stream order (only a guarded frame writes it), as in reset_guard_band
  if (c->sampling_mode == ADANERF_SAMPLING_GUARDED && (d_n_map || d_thr_map) && !has_budget_map(c) && c->total.p)
    HIP_TRY(c, hipMemsetAsync(reinterpret_cast<int32_t*>(c->total.p) + kTotalRefined, 0, sizeof(int32_t), c->stream));
  c->budget_n = d_n_map;
  c->budget_thr = d_thr_map;
  return ADANERF_OK;
}

int adanerf_foveate(adanerf_ctx* c, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* n, const float* thr,
                    uint8_t* d_n_map, float* d_thr_map) {
  if (!c) return ADANERF_EINVAL;
  if (!std::isfinite(gaze_x) || !std::isfinite(gaze_y)) return fail(c, ADANERF_EINVAL, "adanerf_foveate: the gaze must be finite");
  if (n_rings < 0 || n_rings > kFoveaMaxRings) return fail(c, ADANERF_EINVAL, "adanerf_foveate: n_rings must be in 0.." + std::to_string(kFoveaMaxRings));
  if ((n_rings > 0 && !radius_px) || !n || !thr) return fail(c, ADANERF_EINVAL, "adanerf_foveate: NULL array");
  FoveaParams f{};
  for (int k = 0; k < n_rings; ++k) {
    if (radius_px[k] < 0 || (k > 0 && radius_px[k] <= radius_px[k - 1]))
      return fail(c, ADANERF_EINVAL, "adanerf_foveate: radii must be >= 0 and strictly ascending");
    const uint64_t d = 2ull * static_cast<uint64_t>(radius_px[k]);
    f.r2x4[k] = d * d;
  }
  for (int k = 0; k <= n_rings; ++k) {
    if (n[k] < 0 || n[k] > 255) return fail(c, ADANERF_EINVAL, "adanerf_foveate: every n must be in 0..255");
    if (std::isnan(thr[k])) return fail(c, ADANERF_EINVAL, "adanerf_foveate: a threshold is not a number");
    f.n[k] = static_cast<uint8_t>(n[k]);
    f.thr[k] = thr[k];
  }
  for (int k = n_rings; k < kFoveaMaxRings; ++k) {      // the slots behind the rings in use contain nothing and carry the outside entry
    f.r2x4[k] = ~0ull;
    f.n[k + 1] = f.n[n_rings];
    f.thr[k + 1] = f.thr[n_rings];
  }
  // twice the gaze, to the nearest integer (ties to even); beyond +-2^31 half-pixels every pixel of any frame is equally far outside
  auto half_px = [](float g) { return static_cast<int64_t>(std::lrintf(std::min(std::max(2.0f * g, -2147483648.0f), 2147483648.0f))); };
  f.gx2 = half_px(gaze_x);
  f.gy2 = half_px(gaze_y);
  BIND(c);
  const int R = c->ms.info.rays_local;
  if (R <= 0 || (!d_n_map && !d_thr_map)) return ADANERF_OK;
  hipLaunchKernelGGL(foveate_kernel, dim3((R + 255) / 256), dim3(256), 0, c->stream, c->ms.rg, f, R, d_n_map, d_thr_map);
  HIP_RETURN(c, hipGetLastError());
}

int adanerf_compact_budget(adanerf_ctx* c, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr, const uint8_t* d_n_map,
                           const float* d_thr_map, int32_t* d_off, int32_t* d_cnt, uint32_t* d_key, float* d_w, int32_t* d_total) {
  BIND(c);
  if (!d_oracle || !d_off || !d_cnt || !d_key || !d_w || !d_total) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0 || n_max < 1 || n_max > kBins || !(thr > 0.f)) return fail(c, ADANERF_EINVAL, "n_rays/n_max/thr out of range (thr must be > 0: the dense mode selects nothing)");
  if (static_cast<int64_t>(n_rays) >= (1ll << 25)) return fail(c, ADANERF_EINVAL, "n_rays must be < 2^25 per batch");
  if (static_cast<int64_t>(n_rays) * n_max > 0x7fffffffll) return fail(c, ADANERF_EINVAL, "n_rays * n_max exceeds 2^31 - 1");
  if (int rc = ensure_compact_scratch(c, n_rays, n_max)) return rc;
  const BudgetMaps bm{d_n_map, d_thr_map, 0};
  return launch_compact(c, d_oracle, n_rays, n_max, thr, d_off, d_cnt, d_key, d_w, d_total, &bm);
}

int adanerf_set_depth_limit(adanerf_ctx* c, const float* d_limit_zc) {
  if (!c) return ADANERF_EINVAL;
  if (d_limit_zc) {
    if (c->ms.coarse_fine || c->ms.info.sampler_mode != ADANERF_SAMPLER_ADAPTIVE)
      return fail(c, ADANERF_EUNSUPPORTED, "adanerf_set_depth_limit: a depth limit trims the adaptive selection: this model's sampler has none");
    if (c->ms.info.use_ndc) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_set_depth_limit: the samples of a useNDC model live in NDC space, not along the camera's viewing axis");
    if (c->ms.info.dense) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_set_depth_limit: threshold 0 (dense) keeps every bin with implicit keys: there is no selection to trim");
    if (reinterpret_cast<uintptr_t>(d_limit_zc) & 3) return fail(c, ADANERF_EINVAL, "adanerf_set_depth_limit: the map must be 4-byte aligned");
  }
  c->depth_limit = d_limit_zc;
  return ADANERF_OK;
}

int adanerf_compact_depth_limit(adanerf_ctx* c, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr, const float* d_rays,
                                const float* d_limit_zc, const float pos[3], const float rot[9], int32_t* d_off, int32_t* d_cnt, uint32_t* d_key,
                                float* d_w, int32_t* d_total) {
  BIND(c);
  if (!d_oracle || !d_rays || !d_limit_zc || !pos || !rot || !d_off || !d_cnt || !d_key || !d_w || !d_total) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0 || n_max < 1 || n_max > kBins || !(thr > 0.f)) return fail(c, ADANERF_EINVAL, "n_rays/n_max/thr out of range (thr must be > 0: the dense mode selects nothing)");
  if (static_cast<int64_t>(n_rays) >= (1ll << 25)) return fail(c, ADANERF_EINVAL, "n_rays must be < 2^25 per batch");
  if (static_cast<int64_t>(n_rays) * n_max > 0x7fffffffll) return fail(c, ADANERF_EINVAL, "n_rays * n_max exceeds 2^31 - 1");
  if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_limit_zc) & 3))
    return fail(c, ADANERF_EINVAL, "d_rays must be 16-byte aligned, d_limit_zc 4-byte aligned");
  if (!c->ms.sp.ztab) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_compact_depth_limit: this context has no depth table");
  if (int rc = ensure_compact_scratch(c, n_rays, n_max)) return rc;
  const DepthLimit dl{d_limit_zc, 0, nullptr, d_rays, c->ms.sp.ztab, depth_pose(pos, rot)};
  return launch_compact(c, d_oracle, n_rays, n_max, thr, d_off, d_cnt, d_key, d_w, d_total, nullptr, &dl);
}

int adanerf_set_sample_cap(adanerf_ctx* c, float mean_samples_per_ray) {
  BIND(c);
  const float cap = mean_samples_per_ray;
  if (cap != 0.f && !(std::isfinite(cap) && cap >= 1.f))
    return fail(c, ADANERF_EINVAL, "adanerf_set_sample_cap: the cap must be 0 (off) or a finite mean of at least 1 sample per ray");
  if (cap != 0.f) {
    if (c->ms.coarse_fine || c->ms.info.sampler_mode != ADANERF_SAMPLER_ADAPTIVE)
      return fail(c, ADANERF_EUNSUPPORTED, "adanerf_set_sample_cap: a cap trims the adaptive selection: this model's sampler has none");
    if (c->ms.info.dense) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_set_sample_cap: threshold 0 (dense) keeps every bin: there is no selection to trim");
  }
  // a guarded context renders as the split engine while a cap is installed: the per-frame count of re-evaluated rays goes back to 0 in
  // stream order (only a guarded frame writes it), as in adanerf_set_budget_map
  if (c->sampling_mode == ADANERF_SAMPLING_GUARDED && cap != 0.f && !has_sample_cap(c) && c->total.p)
    HIP_TRY(c, hipMemsetAsync(reinterpret_cast<int32_t*>(c->total.p) + kTotalRefined, 0, sizeof(int32_t), c->stream));
  c->sample_cap = cap == 0.f ? 0.f : cap;
  return ADANERF_OK;
}

int adanerf_sample_cap_report(adanerf_ctx* c, adanerf_cap_report* out) {
  BIND(c);
  if (!out) return fail(c, ADANERF_EINVAL, "adanerf_sample_cap_report: out == NULL");
  CapRecord r{};
  r.thr_max = -INFINITY;
  if (c->cap_record.p && c->cap_record_live) {
    HIP_TRY(c, hipMemcpyAsync(&r, c->cap_record.p, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  out->threshold_max = r.thr_max;
  out->batches_trimmed = r.batches_trimmed;
  out->samples_selected = r.selected;
  out->samples_kept = r.kept;
  return ADANERF_OK;
}

int adanerf_compact_cap(adanerf_ctx* c, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr, const uint8_t* d_n_map, const float* d_thr_map,
                        const float* d_rays, const float* d_limit_zc, const float pos[3], const float rot[9], int64_t cap_total, int32_t* d_off,
                        int32_t* d_cnt, uint32_t* d_key, float* d_w, int32_t* d_total, float* d_tstar) {
  BIND(c);
  if (!d_oracle || !d_off || !d_cnt || !d_key || !d_w || !d_total || !d_tstar) return fail(c, ADANERF_EINVAL, "NULL buffer");
  if (n_rays < 0 || n_max < 1 || n_max > kBins || !(thr > 0.f)) return fail(c, ADANERF_EINVAL, "n_rays/n_max/thr out of range (thr must be > 0: the dense mode selects nothing)");
  if (static_cast<int64_t>(n_rays) >= (1ll << 25)) return fail(c, ADANERF_EINVAL, "n_rays must be < 2^25 per batch");
  if (static_cast<int64_t>(n_rays) * n_max > 0x7fffffffll) return fail(c, ADANERF_EINVAL, "n_rays * n_max exceeds 2^31 - 1");
  if (cap_total < n_rays) return fail(c, ADANERF_EINVAL, "adanerf_compact_cap: cap_total must be at least n_rays (every non-empty row keeps one entry)");
  if (d_limit_zc) {
    if (!d_rays || !pos || !rot) return fail(c, ADANERF_EINVAL, "adanerf_compact_cap: a depth limit needs d_rays, pos and rot");
    if ((reinterpret_cast<uintptr_t>(d_rays) & 15) || (reinterpret_cast<uintptr_t>(d_limit_zc) & 3))
      return fail(c, ADANERF_EINVAL, "d_rays must be 16-byte aligned, d_limit_zc 4-byte aligned");
    if (!c->ms.sp.ztab) return fail(c, ADANERF_EUNSUPPORTED, "adanerf_compact_cap: this context has no depth table");
  }
  if (int rc = ensure_compact_scratch(c, n_rays, n_max)) return rc;
  if (int rc = ensure_cap_buffers(c, n_rays)) return rc;
  c->cap_record_live = true;
  const BudgetMaps bm{d_n_map, d_thr_map, 0};
  const DepthLimit dl = d_limit_zc ? DepthLimit{d_limit_zc, 0, nullptr, d_rays, c->ms.sp.ztab, depth_pose(pos, rot)} : DepthLimit{};
  hipLaunchKernelGGL(cap_reset_kernel, dim3(1), dim3(1), 0, c->stream, reinterpret_cast<CapRecord*>(c->cap_record.p));      // -inf for n_rays == 0 too
  HIP_TRY(c, hipGetLastError());
  if (int rc = launch_compact(c, d_oracle, n_rays, n_max, thr, d_off, d_cnt, d_key, d_w, d_total, (d_n_map || d_thr_map) ? &bm : nullptr,
                              d_limit_zc ? &dl : nullptr, &cap_total))
    return rc;
  HIP_RETURN(c, hipMemcpyAsync(d_tstar, c->cap_record.p, sizeof(float), hipMemcpyDeviceToDevice, c->stream));
}

int adanerf_set_stream(adanerf_ctx* c, void* hip_stream) {
  BIND(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
  return ADANERF_OK;
}

int adanerf_set_profiling(adanerf_ctx* c, int32_t enabled) {
  BIND(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->profiling = enabled != 0;
  reset_record(c);
  return ADANERF_OK;
}

int adanerf_collect_stats(adanerf_ctx* c, adanerf_stats* stats, int32_t* frames) {
  if (!c || !stats) return ADANERF_EINVAL;
  BIND(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int rc = sum_stats(c, stats)) return rc;
  stats->rays = c->ms.info.rays_local;
  if (frames) *frames = c->prof_frames;
  reset_record(c);
  return ADANERF_OK;
}

int adanerf_assemble_strips(adanerf_ctx* c, const void* d_gathered, void* d_image) {
  BIND(c);
  if (!d_gathered || !d_image) return fail(c, ADANERF_EINVAL, "NULL buffer");
  const int n = c->ms.info.width * c->ms.info.height;
  hipLaunchKernelGGL(assemble_strips_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, reinterpret_cast<const uchar4*>(d_gathered),
                     reinterpret_cast<uchar4*>(d_image), c->ms.info.width, c->ms.info.height, c->ms.rg.strip_rows, c->ms.rg.world, c->ms.info.rays_local_max);
  HIP_RETURN(c, hipGetLastError());
}

int adanerf_gather_to(adanerf_ctx* dst, void* d_dst, adanerf_ctx* src, const void* d_src, size_t bytes) {
  if (!dst || !src) return ADANERF_EINVAL;
  if (!d_dst || !d_src) return fail(dst, ADANERF_EINVAL, "NULL buffer");
  if (bytes == 0) return ADANERF_OK;
  adanerf_ctx* c = src;
  BIND(src);
  if (src->device != dst->device) {
    if (dst->device < 64 && !((src->peer_tried >> dst->device) & 1)) {
      src->peer_tried |= 1ull << dst->device;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, src->device, dst->device) == hipSuccess && can)
        (void)hipDeviceEnablePeerAccess(dst->device, 0);      // direct xGMI stores; "already enabled" is fine
      (void)hipGetLastError();                                // without peer access the copy is staged by the runtime
    }
    HIP_TRY(c, hipMemcpyPeerAsync(d_dst, dst->device, d_src, src->device, bytes, src->stream));
  } else {
    HIP_TRY(c, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, src->stream));
  }
  if (src == dst || src->stream == dst->stream) return ADANERF_OK;
  if (!src->peer_event) HIP_TRY(c, hipEventCreateWithFlags(&src->peer_event, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(src->peer_event, src->stream));
  c = dst;
  BIND(dst);
  HIP_RETURN(c, hipStreamWaitEvent(dst->stream, src->peer_event, 0));
}

int adanerf_probe_mfma(adanerf_ctx* c, int32_t operands, int32_t f16, float target_ms, float* tflops, float* clock_mhz) {
  BIND(c);
  if (operands < 0 || operands > 3 || !(target_ms > 0.f) || target_ms > 5000.f || !tflops || !clock_mhz)
    return fail(c, ADANERF_EINVAL, "operands must be 0..3, target_ms in (0, 5000], outputs non-NULL");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  double tf = 0, mhz = 0;
  HIP_TRY(c, probe_mfma_rate(operands, f16 != 0, target_ms, c->ms.info.compute_units, c->stream, &tf, &mhz));
  *tflops = static_cast<float>(tf);
  *clock_mhz = static_cast<float>(mhz);
  return ADANERF_OK;
}

int adanerf_malloc(adanerf_ctx* c, size_t bytes, void** d_out) {
  if (!c || !d_out) return ADANERF_EINVAL;
  BIND(c);
  HIP_RETURN(c, hipMalloc(d_out, bytes ? bytes : 1));
}
int adanerf_free(adanerf_ctx* c, void* d_ptr) {
  BIND(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_RETURN(c, hipFree(d_ptr));
}
int adanerf_memcpy_h2d(adanerf_ctx* c, void* d_dst, const void* src, size_t bytes) {
  BIND(c);
  HIP_TRY(c, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_RETURN(c, hipStreamSynchronize(c->stream));
}
int adanerf_memcpy_d2h(adanerf_ctx* c, void* dst, const void* d_src, size_t bytes) {
  BIND(c);
  HIP_TRY(c, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_RETURN(c, hipStreamSynchronize(c->stream));
}

int adanerf_get_buffer(adanerf_ctx* c, int32_t which, void** d_out, size_t* bytes_out) {
  if (!c || !d_out) return ADANERF_EINVAL;
  DevBuf* b = nullptr;
  switch (which) {
    case ADANERF_BUF_RAYS: b = &c->rays; break;
    case ADANERF_BUF_ORACLE: b = &c->oracle; break;
    case ADANERF_BUF_RAY_OFFSETS: b = &c->ray_offsets; break;
    case ADANERF_BUF_RAY_COUNTS: b = &c->ray_counts; break;
    case ADANERF_BUF_SAMPLE_KEY: b = &c->sample_key; break;
    case ADANERF_BUF_SAMPLE_W: b = &c->sample_w; break;
    case ADANERF_BUF_RAW: b = &c->raw; break;
    case ADANERF_BUF_TOTAL: b = &c->total; break;
    case ADANERF_BUF_SAMPLE_Z: b = &c->sample_z; break;
    case ADANERF_BUF_RAW_COARSE: b = &c->raw_coarse; break;
    case ADANERF_BUF_RAY_LIST: b = &c->ray_list; break;
    case ADANERF_BUF_RAY_LIST_COUNT: b = &c->ray_list_count; break;
    default: return fail(c, ADANERF_EINVAL, "unknown buffer id");
  }
  *d_out = b->p;
  if (bytes_out) *bytes_out = b->bytes;
  return ADANERF_OK;
}

}  // extern "C"
