// The context behind the C ABI (include/adanerf_hip.h) and what a launching unit needs to work on one: the owner of a device allocation, the
// error helpers (defined once, in adanerf_hip.hip) and the three macros around them.  Declarations only; for the .hip units alone.
#pragma once
#include "../../include/adanerf_hip.h"

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "k_common.hip.hpp"      // NetParams
#include "launch.hpp"
#include "model_setup.hpp"       // and through it format.hpp, pack.hpp, params.hpp

namespace adanerf {

// A device allocation and its owner: move-only, freed with it.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { return std::swap(p, o.p), std::swap(bytes, o.bytes), *this; }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

struct PackedDev {
  DevBuf w, b;
  NetParams params{};
};

int fail(adanerf_ctx* c, int code, const std::string& msg);      // `code`, with msg as the context's last error (the creating thread's, without one)
int hip_rc(adanerf_ctx* c, hipError_t e, const char* what);      // ADANERF_EDEVICE and the message "<what>: <HIP's error string>" unless e is hipSuccess
int dev_alloc(adanerf_ctx* c, DevBuf* b, size_t bytes);          // at least `bytes` behind b; a failed growth leaves the buffer usable

// Scratch of the image-space stages (stages.hip): grown on demand by the stage that needs it, freed with the context, touched by no one else.
struct StageScratch {
  DevBuf flip_tab, flip_partial, flip_mean;   // adanerf_flip: filter tables of the last pixels-per-degree value, per-tile sums, the mean
  double flip_ppd = 0.0;                      // what flip_tab holds (0: nothing yet)
  FlipParams flip_params{};
  bool flip_lds_raised = false;               // flip_kernel may use more than 64 KB of dynamic LDS
  DevBuf zbuf;                                // adanerf_reproject: [width*height] uint64 z-buffer; adanerf_reproject_pair: two of them, one behind the other
  DevBuf gather_surface;                      // adanerf_reproject_gather: [width*height] float4 (surface point, source camera depth)
  DevBuf count;                               // the one int32 a stage counts in (stages.hip stage_count)
  DevBuf upsample_zp;                         // adanerf_temporal_upsample / _resolve_sparse: [width*height] fp32 depths at the previous pose
};

}  // namespace adanerf

struct adanerf_ctx {
  adanerf_options opt{};
  adanerf::ModelSetup ms;             // what the model directory and the options say (model_setup.hpp); info, rg and sp move on from there
  std::string err;
  hipStream_t stream = nullptr;       // stream in use
  hipStream_t own_stream = nullptr;   // the context's own stream
  adanerf::GridCache grids;           // resident workgroups of every persistent kernel launched so far
  std::vector<hipEvent_t> events;     // pool; 5 per batch
  size_t events_used = 0;
  bool profiling = false;
  int prof_frames = 0;
  std::vector<int32_t*> pinned_totals;   // one pinned int32 per recorded batch
  // always-on monitor of the guarded selection (ADANERF_SAMPLING_GUARDED): the device's running {largest difference seen, violations,
  // largest pair error seen, audit mismatches, audited rays} copied to pinned memory after every frame and looked at before the next
  // one -- a violated band (or a failed audit) widens it (poll_guard)
  int32_t* guard_host = nullptr;
  hipEvent_t guard_ev = nullptr;
  bool guard_ev_pending = false;
  int guard_viol_seen = 0;
  int guard_mism_seen = 0;
  bool guard_ev_stale = false;           // the copy in flight was taken under another (N, threshold): it must not widen the band in force
  int guard_widened = 0;
  uint32_t guard_frame = 0;              // frames rendered in guarded mode: the audit's rotating phase
  int debug_guard = 0;                   // $ADANERF_DEBUG_GUARD at create (measurement knobs, bit 0: no whole-row monitor; bits 1 / 2: which plain-fp16 sampling kernel)
  std::string model_dir;
  uint64_t model0_hash = 0;              // FNV-1a 64 of model0.onnx: key of the calibration record
  adanerf_stats folded{};                // profiling record folded out of a full event pool (see adanerf_render)

  adanerf::NetTopology topo0, topo1;       // read off the ONNX initializers
  bool generic0 = false, generic1 = false;   // not the 8 x 256 (/ skip 4) topology or not a 10-4 (2-2) encoding: the run-time-shaped fp32 kernels (k_generic_f32.hip.hpp)
  int enc0 = adanerf::kEnc10_4, enc1 = adanerf::kEnc10_4;      // slot layout of the two networks' encodings (launch_f32.hpp)
  adanerf::GenericTopo gen0{}, gen1{};
  adanerf::DevBuf rsi_z;                   // [ray_samples] world depths of the raySampleInput points

  adanerf::PackedDev net0;                 // sampling net, fp32 fragments (exact engine)
  adanerf::PackedDev net0_split;           // sampling net, fp16 hi/lo' fragment pairs (split-precision engine)
  adanerf::PackedDev net0_f16;             // sampling net, plain fp16 fragments (ADANERF_SAMPLING_FP16, packed on first use)
  adanerf::TensorMap net0_host;
  int sampling_mode = 0;          // ADANERF_SAMPLING_*
  adanerf::DevBuf overflow;                // int32 counter: rays whose oracle values came out non-finite
  adanerf::PackedDev net1[3];              // shading net per precision (packed lazily)
  adanerf::TensorMap net1_host;
  adanerf::DevBuf ztab;                    // [2][128]: the sampler's bin centres, the dense mode's depths (depth_table); ms.sp.ztab is the one in force
  // vanilla NeRF (ADANERF_SAMPLER_COARSE_FINE): model0.onnx is a NeRF net as well, evaluated at n_coarse uniform depths
  adanerf::PackedDev netc[3];              // coarse net per precision (packed lazily)
  adanerf::NetTopology topoc;
  bool genericc = false;
  adanerf::GenericTopo genc{};
  adanerf::ShadeParams spc{};              // its sample positions: uniform depth table, rayMarchNormalization[0]
  adanerf::DevBuf ztab_coarse, raw_coarse, key_coarse;

  // per-batch buffers
  int cap_rays = 0, cap_nmax = 0;
  adanerf::DevBuf rays, oracle, ray_offsets, ray_counts, selbin, selw, block_total, block_offset, total;
  adanerf::DevBuf sample_key, sample_w, raw, sample_z;
  adanerf::DevBuf guard_mask, refine_list, guard_probe;   // ADANERF_SAMPLING_GUARDED: undecided bit per ray (one word per 32), ids of the
                                                          // rays to re-evaluate, first-pass top value of each undecided ray (monitor)
  float guard_eps = 0.f;             // the band in raw-output units; 0: not calibrated yet
  float guard_eps_pair = 0.f;        // bound on the error of a (kept - candidate) difference, raw-output units; 0: 2 x guard_eps
  int guard_audit_period = 0;        // 0: no audit; else a power of two <= 32
  int device = 0;                 // HIP device ordinal this context lives on
  float* aux_depth = nullptr;        // adanerf_set_aux_outputs: caller-owned [rays_local] buffers filled by adanerf_render
  float* aux_acc = nullptr;
  float* aux_disp = nullptr;         // adanerf_set_disp_output
  const uint8_t* budget_n = nullptr;  // adanerf_set_budget_map: caller-owned [rays_local] per-ray N / threshold, read by the trim kernels of every render
  const float* budget_thr = nullptr;
  const float* depth_limit = nullptr; // adanerf_set_depth_limit: caller-owned [rays_local] camera-space depths, read by the depth trim of every render
  float sample_cap = 0.f;             // adanerf_set_sample_cap: mean samples per ray a batch may shade, 0: no cap
  adanerf::DevBuf cap_state;          // k_cap.hip.hpp: CapState + the histograms of the three radix levels (zeroed per batch)
  adanerf::DevBuf cap_record;         // CapRecord: t* and totals of the last batch, running figures of the last frame
  bool cap_record_live = false;       // the record describes the last render (false: that render's cap could not trim and launched nothing)
  adanerf::DevBuf cap_map;            // [batch] the threshold map the unchanged trim kernels read t* from
  adanerf::DevBuf disp_scratch;      // [2, batch] depth / accumulation of the batch when the caller asked for disparity only
  adanerf::StageScratch stages;      // what the image-space stages (stages.hip) keep between calls
  // adanerf_render_masked: the mask as bit words, the ascending ray list and its count (for the frame), staged pixels of one listed batch
  // (rgba8 [cap], rgb [cap,3], depth / acc / disp [3,cap]); grown on demand
  adanerf::DevBuf mask_bits, ray_list, ray_list_count, stage_rgba8, stage_rgb, stage_aux;
  int stage_cap = 0;
  float px_dx = 0.f, px_dy = 0.f;    // adanerf_set_pixel_offset: kept here, not in ms.rg (calibrate_guard and adanerf_set_frame_size derive from / rewrite that)
  hipEvent_t peer_event = nullptr;   // adanerf_gather_to: orders the destination stream behind the copy
  uint64_t peer_tried = 0;           // bit d: peer access to device d has been requested once
};

#define HIP_TRY(ctx, call) do { if (int rc_ = adanerf::hip_rc(ctx, (call), #call)) return rc_; } while (0)
#define HIP_RETURN(ctx, call) return adanerf::hip_rc(ctx, (call), #call)
// Every entry point that touches the device first makes the context's device current: one host thread may drive
// several contexts on different GPUs (adanerf_amd/host --gpus N), and a launch on another device's stream fails.
#define BIND(ctx) do { if (!(ctx)) return ADANERF_EINVAL; HIP_TRY(ctx, hipSetDevice((ctx)->device)); } while (0)
