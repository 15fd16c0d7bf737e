/*
 * adanerf_hip.h -- C ABI of libadanerf_hip.so, the MI355X (gfx950) AdaNeRF inference renderer.
 *
 * Drop-in boundary: these entry points are what the reference viewer's host pipeline binds in
 * place of its CUDA launchers + TensorRT contexts.  Reference interface replaced (paths relative
 * to /root/reference/adanerf_real_time_viewer):
 *
 *   adanerf_create / adanerf_destroy     NeuralRenderer::init (src/neuralrenderer.cpp:59-139):
 *                                        Config::load (src/config.cpp:270-344), Encoding::load,
 *                                        RayMarchFromPoses::create (src/featureset.cpp:67-140),
 *                                        ImageGenerator::load/initEngine (src/imagegenerator.cpp:84-226)
 *   adanerf_set_camera                   Camera::UpdateFeatureRot/getPosition (src/camera.cpp:143-201)
 *   adanerf_set_selection                numRaymarchSamples / adaptiveSamplingThreshold: members of RayMarchFromPoses, handed to
 *                                        updateRayMarchFromPosesAdaptive on every call (src/featureset.cpp:80,153)
 *   adanerf_set_frame_size               Settings::width / height (src/settings.cpp:20-33), fixed for the life of the viewer's NeuralRenderer
 *   adanerf_set_pixel_offset             none: the ray table is fixed to pixel centres (src/util/raygeneration.py:10-26 of the reference's
 *                                        PyTorch tree); with adanerf_accumulate / adanerf_resolve_mean this is supersampling in time
 *   adanerf_present                      the blit from the render buffer to the window (src/interoprenderbuffer.cpp:87);
 *                                        ADANERF_PRESENT_AREA replaces its nearest decimation by an exact area filter
 *   adanerf_reproject                    none: the viewer presents the frame it rendered (src/neuralrenderer.cpp:146-182 ->
 *                                        src/interoprenderbuffer.cpp:87); this stage sits in front of that step
 *   adanerf_reproject_gather             none, as adanerf_reproject: the same warp as a gather, without cracks
 *   adanerf_reproject_pair               none, as adanerf_reproject: two rendered frames warped to a pose between them
 *   adanerf_temporal_resolve             none: the viewer shows each frame as rendered, without a history (src/neuralrenderer.cpp:146-182 ->
 *                                        src/interoprenderbuffer.cpp:87); temporal anti-aliasing between the render and that step
 *   adanerf_temporal_upsample            none: the viewer blits the frame it rendered (src/interoprenderbuffer.cpp:87), at whatever size it
 *                                        was rendered; this stage rebuilds a frame of s x the render size over s^2 jittered renders
 *   adanerf_render                       ImageGenerator::inference, 2-context adaptive branch
 *                                        (src/imagegenerator.cpp:282-394) as called from
 *                                        NeuralRenderer::render (src/neuralrenderer.cpp:146-182)
 *   adanerf_render_masked                none: ImageGenerator::inference always runs every ray of the frame; this renders the rays a mask
 *                                        selects (the holes of adanerf_reproject, the rejected pixels of the temporal stages)
 *   adanerf_ray_features                 updateSpherePosDirBatchedUnrolledEnc
 *                                        (include/cuda/adanerf_cuda_kernels.cuh:41-45)
 *   adanerf_sample_mlp                   contexts[0]->executeV2 (src/imagegenerator.cpp:308-312)
 *   adanerf_compact                      updateRayMarchFromPosesAdaptive, selection half
 *                                        (include/cuda/adanerf_cuda_kernels.cuh:52-58; kernels
 *                                        src/cuda/adaptive_cuda_kernels.cu:229-607)
 *   adanerf_shade_features               updateRayMarchFromPosesAdaptive, feature half
 *                                        (rayMarchFromPosesAdaptive[NDC], adaptive_cuda_kernels.cu:609-739)
 *   adanerf_shade_mlp                    contexts[1]->executeV2 (src/imagegenerator.cpp:336-344)
 *   adanerf_composite                    copyResultRaymarchAdaptiveMultDepth
 *                                        (include/cuda/adanerf_cuda_kernels.cuh:30-32)
 *   adanerf_flip                         generate_flip_data (src/evaluate.py:120-145 of the reference's PyTorch tree) over
 *                                        FLIP.compute_flip (src/util/flip_loss.py:61-105)
 *
 * Numerics follow the reference's PyTorch path (src/evaluate.py over nerf_raymarch_common.py /
 * features.py / models.py) wherever it disagrees with the viewer.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ADANERF_E* code on failure; the message is
 *     available from adanerf_last_error().  Nothing throws or aborts across this boundary.
 *   - one context = one device = one non-default HIP stream.  A context is not thread-safe;
 *     distinct contexts are independent.
 *   - pointers named d_* are DEVICE pointers on the context's device; all others are host.
 *   - the library owns every buffer behind the context; the caller owns output buffers it passes.
 *   - calls enqueue on the context's stream; adanerf_sync() (or stats != NULL) waits.
 */
#ifndef ADANERF_HIP_H
#define ADANERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADANERF_ABI_VERSION 4   /* 2: adanerf_info.view_cell_size, .num_samples_coarse appended
                                   3: ADANERF_SAMPLING_GUARDED, adanerf_options.guard_eps, adanerf_stats.rays_refined (carved out of
                                      reserved words), adanerf_info.guard_eps APPENDED (adanerf_info grew by 4 bytes)
                                   4: audited guard band: adanerf_options.guard_eps_pair / .guard_audit_period (carved out of the
                                      reserved words: size unchanged); adanerf_info and adanerf_stats GROW (guard fields + reserved
                                      words for later versions); adanerf_compact_guarded / adanerf_calibrate_guard take more
                                      arguments.  adanerf_get_info / adanerf_render write the whole struct: a caller checks
                                      adanerf_abi_version() == ADANERF_ABI_VERSION (and may compare adanerf_struct_sizes with its
                                      own sizeof) once after loading the library -- there is no per-call size argument */

enum {
  ADANERF_OK = 0,
  ADANERF_EINVAL = -1,    /* bad argument */
  ADANERF_EIO = -2,       /* model directory / file format problem */
  ADANERF_EDEVICE = -3,   /* HIP runtime error */
  ADANERF_EUNSUPPORTED = -4 /* config outside the supported north-star path */
};

/* arithmetic of the sampling MLP (its outputs drive the bit-exact sample selection) */
enum {
  ADANERF_SAMPLING_SPLIT_FP16 = 0, /* default: x = hi + 2^-11 lo' (two fp16), 3 x v_mfma_f32_32x32x16_f16 per term,
                                      fp32 accumulate; 22-bit operands, measured error <= fp32 sgemm's */
  ADANERF_SAMPLING_FP32 = 1,       /* v_mfma_f32_32x32x2_f32: bitwise an fp32 fma chain */
  ADANERF_SAMPLING_FP16 = 2,       /* opt-in speed mode: plain fp16 operands, one MFMA per term, fp32 accumulate -- what the
                                      reference viewer's TensorRT engine does (imagegenerator.cpp:155-156).  Raw outputs
                                      are then within ~3e-3 of fp32 and the selected bins differ from the fp32 PyTorch
                                      path on 0.3-1.5 % of rays (tools/probes/sampling_agreement.py); 3x faster. */
  ADANERF_SAMPLING_GUARDED = 3     /* two-precision selection with the results of ADANERF_SAMPLING_SPLIT_FP16: every ray goes
                                      through the plain-fp16 engine; a ray whose selection could change under a perturbation
                                      of guard_eps of its raw outputs (a value within the band around the threshold, a
                                      not-kept value closer than guard_eps_pair to the N-th largest, a tie, a non-finite value) is
                                      re-evaluated by the split-precision engine, which overwrites its row.  Selections are
                                      those of the split engine as long as |fp16 output - split output| <= guard_eps and the
                                      error of a (kept - candidate) difference <= guard_eps_pair hold.  Both assumptions are
                                      MEASURED on every re-evaluated ray (whole row: adanerf_stats.guard_max_seen /
                                      .guard_pair_seen / .guard_violations) and the OUTCOME is audited: every frame a rotating
                                      1 / guard_audit_period of ALL rays -- the ones the band declared decided included -- goes
                                      through the split engine as well and its selection is compared with the one in place
                                      (adanerf_stats.guard_audited / .guard_audit_mismatch); a violated bound or a mismatch widens
                                      the band for the frames that follow.  adanerf_stats.rays_refined counts the re-evaluated
                                      rays.  Applies where the selection is fused into the sampling kernel (adaptive sampler,
                                      N <= 16, threshold > 0, 8 x 256 net); everywhere else this mode runs the split-precision
                                      engine alone. */
};
/* Sampling nets of another topology / encoding layout (run-time-shaped kernels): ADANERF_SAMPLING_FP32 runs the exact fp32
 * kernel, every other mode the split-precision one (same arithmetic as ADANERF_SAMPLING_SPLIT_FP16; no plain-fp16 pass);
 * with raySampleInput always the fp32 kernel.  Sampling nets wider than 256 run the fp32 kernel in every mode (its wide form).
 *
 * Operand range of the 16-bit sampling engines (tests/range_networks.py states the rule per layer, tests/test_gpu_sampling_ranges.py holds
 * the kernels to it bit for bit): an operand x -- an encoded input, a ReLU output, a weight -- is hi = fp16(x), lo' = fp16((x - hi) 2^11),
 * both conversions round to nearest even and keep fp16 subnormals; a layer computes fma(Whi xlo' + Wlo' xhi, 2^-11, bias + Whi xhi) in
 * fp32 (plain fp16: bias + fp16(W) fp16(x)).  So a value is carried to 22 bits down to 2^-14 and with an absolute step of 2^-35 below
 * (lo' subnormal): |x| <= 2^-36 is 0, and so is a weight with |w| <= 2^-36.
 *   Activations: x >= 65520 converts to inf; the row of that ray is then non-finite in every column and the ray counts in
 *   adanerf_stats.sampling_overflow.  Every x <= 65520 - 2^-7 stays finite.  The one fp32 value between, nextafter(65520, 0), is carried
 *   as hi = 65504, lo' = 32768 (a tie, to even) -- the value 65520 -- and overflows at the next hidden layer that reads it with weight 1
 *   (split engine; plain fp16 rounds it to 65504).  A NaN stays a NaN through every ReLU.
 *   Weights: adanerf_create refuses (ADANERF_EUNSUPPORTED) a sampling net with a weight |w| >= 65520 or NaN in every mode but
 *   ADANERF_SAMPLING_FP32, where the network runs on the fp32 kernel: packed as +-inf, such a weight times a negative operand is -inf,
 *   which ReLU turns into a finite 0 whatever the bias -- a wrong row nobody would count.  (Nets that run the fp32 kernel in every
 *   mode -- raySampleInput, width above 256 -- are not refused.)  Biases are fp32 in every engine.
 *   ADANERF_SAMPLING_FP32 has no range below fp32's own and never counts.  Its ReLU is fmaxf: a NaN activation becomes 0 there. */

/* sample placement (config.ini rayMarchSampler[1]) */
enum {
  ADANERF_SAMPLER_ADAPTIVE = 0, /* FromClassifiedDepthAdaptive[NoDepthRange]: AdaNeRF top-N / threshold selection */
  ADANERF_SAMPLER_PDF = 1,      /* FromClassifiedDepth: DONeRF inverse-CDF sampling of sigmoid(oracle), fixed N samples
                                   per ray, classic sigma/delta compositing */
  ADANERF_SAMPLER_COARSE_FINE = 2 /* inFeatures [RayMarchFromPoses, RayMarchFromCoarse]: vanilla NeRF.  model0.onnx is a NeRF net
                                   too; numRaymarchSamples = [Nc, Nf]: Nc uniform depths, Nf more from the coarse weights,
                                   Nc + Nf samples through model1, classic compositing */
};

/* arithmetic of the shading MLP's MFMA path */
enum {
  ADANERF_PREC_BF16 = 0,  /* v_mfma_f32_32x32x16_bf16, fp32 accumulate */
  ADANERF_PREC_FP16 = 1,  /* v_mfma_f32_32x32x16_f16,  fp32 accumulate */
  ADANERF_PREC_FP32 = 2   /* v_mfma_f32_32x32x2_f32 (exact fp32; parity mode) */
};

/* adanerf_options.flags */
enum {
  ADANERF_FLAG_KEEP_ORACLE = 1, /* adanerf_render writes the raw oracle values [batch,128] to ADANERF_BUF_ORACLE and selects from
                                   there in a separate launch (debug / the reference's data flow); by default the selection runs
                                   in the sampling kernel's epilogue and that buffer is not written */
  ADANERF_FLAG_WAVE_SELECT = 2, /* selection by the wave-per-ray kernel (the only one for numRaymarchSamples > 16) even where the
                                   lane-pair selection applies; implies the separate launch */
  ADANERF_FLAG_NO_GUARD_CACHE = 4, /* ADANERF_SAMPLING_GUARDED: neither read nor write the calibration record next to the model
                                   (adanerf_guard_calibration_file); the band is measured at the first guarded frame */
  ADANERF_FLAG_GUARD_AUDIT_FILL = 8 /* ADANERF_SAMPLING_GUARDED (both shipped hosts set it): audit only as many decided rays per frame
                                   as the last, partly filled round of the refinement pass has room for (its grid x 128 rays per
                                   round; the undecided rays fix the number of rounds), so that the audit does not cost a round of
                                   its own (the 800 x 800 frame: 8 rounds instead of 9; an 80 000-ray share of it: 1 instead of 2)
                                   -- unless that room is less than a quarter of the frame's 1 / period quota, in which case it does
                                   take one more round.  The audited window moves through the frame's audit candidates from cycle
                                   to cycle, so every ray is audited at least once in 4 x period frames
                                   (adanerf_stats.guard_audited counts).  Without the flag every frame audits its full quota. */
};

typedef struct adanerf_ctx adanerf_ctx;

typedef struct adanerf_options {
  int32_t width;            /* image width  (Settings::width,  -s w h) */
  int32_t height;           /* image height (Settings::height)         */
  int32_t batch_rays;       /* <=0: whole frame; else min(batch_rays, rays) like Settings::batch_size (-bs) */
  int32_t device_id;        /* HIP device ordinal */
  int32_t precision;        /* ADANERF_PREC_* for the shading MLP */
  int32_t num_samples;      /* >0 overrides numRaymarchSamples from config.ini */
  float   threshold;        /* >=0 overrides adaptiveSamplingThreshold; <0 keeps config value */
  int32_t shard_rank;       /* image-strip shard of this context (multi-GPU); 0 */
  int32_t shard_world;      /* number of shards; 1 */
  int32_t strip_rows;       /* rows per strip for round-robin strip sharding; <=0 -> 8 */
  int32_t sampling_mode;    /* ADANERF_SAMPLING_* */
  int32_t flags;            /* ADANERF_FLAG_* (0 = defaults) */
  float   guard_eps;        /* ADANERF_SAMPLING_GUARDED: the band, in units of the raw network outputs; <= 0 -> the model's
                               calibration record if there is a current one, else calibrated for the loaded model at the first
                               guarded frame (adanerf_calibrate_guard, ADANERF_GUARD_CALIB_POSES poses) and recorded */
  float   guard_eps_pair;   /* ... the bound on the error of a (kept - candidate) difference; <= 0 -> calibrated like guard_eps when
                               that is, else 2 x guard_eps (what the bound on single values implies) */
  int32_t guard_audit_period; /* ... audit 1 / period of all rays per frame: 0 -> ADANERF_GUARD_AUDIT_PERIOD, < 0 -> no audit,
                               else a power of two <= 32 */
  int32_t reserved[1];
} adanerf_options;

/* Band of the guarded selection when calibration is impossible (non-finite outputs): about 2x the largest difference between
 * the plain-fp16 and the split-precision engine measured on the shipped networks (4.7e-3). */
#define ADANERF_GUARD_EPS_DEFAULT 1.0e-2f
/* The calibrated band is ADANERF_GUARD_CALIB_MARGIN x the largest difference found on the calibration rays, at least
 * ADANERF_GUARD_EPS_MIN. */
#define ADANERF_GUARD_CALIB_MARGIN 2.0f
#define ADANERF_GUARD_EPS_MIN 1.0e-3f
#define ADANERF_GUARD_CALIB_POSES 64     /* poses of the automatic calibration (x 4096 rays each) */
#define ADANERF_GUARD_AUDIT_PERIOD 16    /* default audit rate: every ray is audited once in 16 frames */

/* adanerf_info.guard_calib_source */
enum {
  ADANERF_GUARD_FROM_NONE = 0,        /* not calibrated yet */
  ADANERF_GUARD_FROM_OPTIONS = 1,     /* adanerf_options.guard_eps */
  ADANERF_GUARD_FROM_RECORD = 2,      /* the calibration record next to the model (adanerf_guard_calibration_file) */
  ADANERF_GUARD_FROM_CALIBRATION = 3, /* measured by this context (and recorded, if the directory is writable) */
  ADANERF_GUARD_FROM_MONITOR = 4      /* widened after a frame that violated a bound or failed the audit */
};

typedef struct adanerf_info {
  int32_t abi_version;
  int32_t width, height;
  int32_t rays_local;       /* rays rendered by this context (all of w*h when shard_world==1) */
  int32_t rays_local_max;   /* max over shards (gather payload size in rays) */
  int32_t batch_rays;
  int32_t n_in0, n_in1;     /* sampling / shading net input widths (90/90, or 30/90 for 2-2 NDC oracle) */
  int32_t num_samples;      /* N */
  float   threshold;
  int32_t dense;            /* threshold == 0: all 128 bins, no selection */
  int32_t use_ndc;
  int32_t precision;        /* the shading engine that runs: options.precision (every topology / encoding has a 16-bit and an
                               fp32 form since ABI 3) */
  int32_t compute_units;
  float   fov, focal;
  float   view_cell_center[3];
  float   view_cell_radius;
  float   depth_range[2];
  float   max_depth;
  int32_t sampler_mode;     /* ADANERF_SAMPLER_* (from rayMarchSampler[1]) */
  float   view_cell_size[3];/* dataset_info.txt view_cell_size (the viewer's camera speed: max(size / 2), camera.cpp:47) */
  int32_t num_samples_coarse; /* ADANERF_SAMPLER_COARSE_FINE: Nc (num_samples is then Nc + Nf); else 0 */
  float   guard_eps;          /* ADANERF_SAMPLING_GUARDED: the band in use (0 until it has been calibrated) */
  float   guard_eps_pair;     /* ... the bound on (kept - candidate) differences in use */
  int32_t guard_audit_period; /* ... 0: no audit */
  int32_t guard_calib_source; /* ... ADANERF_GUARD_FROM_* */
  int32_t guard_calib_poses;  /* ... poses behind a calibrated band (record or own calibration), else 0 */
  int32_t reserved[8];
} adanerf_info;

/* per-frame statistics: the fields the reference logs every 100 frames
 * (src/imagegenerator.cpp:379-393): Inference 1/2, fc1, fc2, rm, avg samples ppx */
typedef struct adanerf_stats {
  int64_t total_samples;      /* S summed over batches */
  int32_t rays;               /* rays rendered */
  int32_t batches;
  float   ms_total;           /* first launch -> last kernel end, HIP events on the context's stream */
  float   ms_sample_mlp;      /* ray gen + oracle PE + sampling MLP  ("fc1" + "Inference 1") */
  float   ms_compact;         /* selection + scan + expand           ("fc2", selection half) */
  float   ms_shade_mlp;       /* fused PE + shading MLP              ("fc2" feature half + "Inference 2") */
  float   ms_composite;       /* compositing                          ("rm") */
  int32_t shade_launches;     /* kernel launches behind ms_shade_mlp  */
  int32_t sample_launches;    /* kernel launches behind ms_sample_mlp */
  int32_t sampling_overflow;  /* rays (since create) whose oracle values were non-finite: an activation left the
                                 fp16 range of the split-precision engine -> use ADANERF_SAMPLING_FP32 */
  int32_t rays_refined;       /* ADANERF_SAMPLING_GUARDED: rays re-evaluated by the split-precision engine, summed like
                                 total_samples */
  float   guard_max_seen;     /* ... largest |fp16 - split| raw output seen since create, over ALL 128 outputs of every
                                 re-evaluated ray (undecided or audited): the assumption behind guard_eps, measured every frame */
  int32_t guard_violations;   /* ... re-evaluated rays (since create) where a measured error exceeded its bound: if this is
                                 not 0 the band was too narrow for this model; the library widens it for the frames that
                                 follow (guard_widened), frames before that may hold rays selected by the fp16 engine */
  int32_t guard_widened;      /* ... times (since create) the library widened the band after a frame reported violations or an audit
                                 mismatch: every later frame runs with ADANERF_GUARD_CALIB_MARGIN x the largest errors seen
                                 (adanerf_info.guard_eps / .guard_eps_pair are the bounds in force) */
  float   guard_pair_seen;    /* ... largest error of a (kept - candidate) difference seen since create (the assumption behind
                                 guard_eps_pair; 0 where the sampler transforms its values) */
  int32_t guard_audited;      /* ... rays (since create) that pass 1 had DECIDED and the audit re-evaluated anyway */
  int32_t guard_audit_mismatch; /* ... of those, rays whose exact selection differs from the one pass 1 left in place: must be 0
                                 while no bound is violated; not 0 -> the band is widened (guard_widened) */
  int32_t reserved[5];
} adanerf_stats;

/* ---- lifecycle ---------------------------------------------------------------------------- */

/* model_dir holds config.ini, dataset_info.txt, model0.onnx, model1.onnx (the format written by the
 * reference's src/export.py).  A trailing path separator is optional. */
int adanerf_create(const char* model_dir, const adanerf_options* opt, adanerf_ctx** out);
int adanerf_destroy(adanerf_ctx* ctx);
int adanerf_get_info(const adanerf_ctx* ctx, adanerf_info* info);
/* message of the last failing call on ctx; ctx == NULL reads the thread's last create() failure */
const char* adanerf_last_error(const adanerf_ctx* ctx);
/* ADANERF_ABI_VERSION the library was built with, and sizeof(adanerf_options / adanerf_info / adanerf_stats) as it sees them:
 * the handshake a binding does once after dlopen (structs are written whole, see ADANERF_ABI_VERSION). */
int adanerf_abi_version(void);
int adanerf_struct_sizes(int32_t sizes_out[3]);

/* ---- per frame ---------------------------------------------------------------------------- */

/* pos: camera position (world).  rot_c2w: row-major 3x3 camera-to-world rotation; camera looks
 * along -z, +y up (the convention of src/util/raygeneration.py:24-25).
 * ADANERF_PREC_BF16 contexts: the shading network's layers are scaled for sample positions the scene can produce with the camera in or
 * near its view cell (adanerf_create refuses a scene beyond that range).  A pose so far outside the cell that positions could leave the range
 * returns ADANERF_EUNSUPPORTED and leaves the previous camera in place -- render such poses with an fp16 / fp32 context.  NDC scenes
 * (useNDC) assume rays inside the frustum of the recorded cameras (positions in the NDC cube); that is not checked per pose. */
int adanerf_set_camera(adanerf_ctx* ctx, const float pos[3], const float rot_c2w[9]);

/* The sample budget N and the selection threshold of a live context: the quality / speed dial of an AdaNeRF network, which is trained
 * once and rendered at any budget.  num_samples <= 0 keeps the N in force, threshold < 0 the threshold in force (the convention of
 * adanerf_options).  The resulting pair is validated by the code adanerf_create runs on options.num_samples / .threshold, with its
 * error codes and messages (threshold 0 is the dense mode and needs num_samples == 128); a NaN threshold is ADANERF_EINVAL.  Afterwards
 * the context is what a new context created with these two options would be: same frames, same buffers, same adanerf_info
 * (num_samples / threshold / dense).  On failure nothing has changed.
 *   ADANERF_SAMPLER_PDF / _COARSE_FINE: adanerf_create ignores options.threshold for these samplers, so a threshold >= 0 returns
 *   ADANERF_EUNSUPPORTED; num_samples is the N (coarse/fine: Nf) that options.num_samples overrides.
 *   Ordering is that of adanerf_set_camera: the adanerf_render / adanerf_render_oracle calls issued afterwards see the new pair, frames
 *   already enqueued keep theirs (both values reach the kernels by value).  Device memory is allocated only when N exceeds the largest N
 *   the context has held, never released before adanerf_destroy, and the stream is synchronised only then (before the smaller buffers
 *   are freed); adanerf_render never allocates for it.  The adanerf_stats counters documented as "since create" keep counting.
 *   ADANERF_SAMPLING_GUARDED: the band belongs to (model, N, threshold).  A change leaves the context where a new guarded context is
 *   before its first guarded frame -- bounds from options.guard_eps if given, else from the new pair's calibration record
 *   (adanerf_guard_calibration_file names it), else calibrated at the next guarded frame; adanerf_info.guard_calib_source and the audit's
 *   phase start over; a band widened under the old pair is not carried along.  A call that changes neither value leaves all of this
 *   alone.  Outside the fused selection's domain (N > 16, threshold 0, or while a budget map is installed: adanerf_set_budget_map) the mode
 *   runs the split-precision engine alone, as after create.  Threshold 0 is refused (ADANERF_EUNSUPPORTED) while a budget map is installed. */
int adanerf_set_selection(adanerf_ctx* ctx, int32_t num_samples, float threshold);

/* The frame size of a live context: the third dial of a real-time viewer beside N and the threshold (a window resize, a dynamic-resolution
 * step, a resolution-against-quality table).  Replaces Settings::width / height (src/settings.cpp:20-33), which are fixed for the life of
 * the viewer's NeuralRenderer.  width <= 0 keeps the width in force, height <= 0 the height in force (the convention of
 * adanerf_set_selection).  The resulting size is validated by the code adanerf_create runs on options.width / .height, with its error codes
 * and messages (width * height < 2^25, batch_rays * num_samples <= 2^31 - 1).  Afterwards the context is what a new context created with
 * the original options and this size would be: the same frames byte for byte, the same adanerf_info -- width, height, rays_local,
 * rays_local_max, batch_rays, focal and everything else.  batch_rays is derived again from the options.batch_rays the caller asked for
 * at create, not from the clamped adanerf_info.batch_rays; shard_rank / shard_world / strip_rows stay and are applied to the new height.
 * On failure nothing has changed.  The model, the packed networks, N, the threshold and the camera in force stay.
 *   Ordering is that of adanerf_set_camera: the calls issued afterwards see the new size, frames already enqueued keep theirs (the ray
 *   generator's constants reach the kernels by value).  Buffer capacities follow the largest batch_rays x N the context has held: device
 *   memory is allocated (new buffers first, then the old ones freed) only when the batch exceeds that, never released before
 *   adanerf_destroy, and the stream is synchronised only then; a shrink allocates nothing, a call that changes neither value touches
 *   nothing, and adanerf_render never allocates for it.
 *   The caller-owned per-ray buffers of adanerf_set_aux_outputs / adanerf_set_disp_output / adanerf_set_budget_map /
 *   adanerf_set_depth_limit were sized for the old rays_local: a call that CHANGES rays_local resets all six to NULL (set them again for the new size); a call that does not change it
 *   leaves them.
 *   ADANERF_SAMPLING_GUARDED: the band belongs to (model, N, threshold) and its calibration runs on its own 64 x 64 rays, so the bounds,
 *   their source and pose count in adanerf_info stay; the audit's phase and fill cycle start over (frames do not depend on either). */
int adanerf_set_frame_size(adanerf_ctx* ctx, int32_t width, int32_t height);

/* Sub-pixel ray offsets: the ray of pixel (x, y) passes through image point (x + 0.5 + dx, y + 0.5 + dy) -- positive dx towards higher
 * columns, positive dy towards higher rows -- where the ray table of src/util/raygeneration.py:10-26 fixes it to the pixel centre.  A host
 * that renders several frames at the offsets of adanerf_host_subpixel_grid and averages them (adanerf_accumulate, adanerf_resolve_mean)
 * gets an anti-aliased still: what an evaluator wants against anti-aliased ground truth, a viewer while the camera rests.
 *   dx, dy: finite, |dx| <= 1 and |dy| <= 1; anything else, a NaN included, returns ADANERF_EINVAL with nothing changed.  (0, 0) is the
 *   state after adanerf_create: every frame is then byte for byte what it is without this entry point.
 *   Definition, exact: the kernels keep computing vx = start_x + x_pp * col, vy = start_y + y_pp * row (float64).  With an offset in force
 *   the ray generator handed to a launch carries start_x' = start_x + x_pp * (double)dx and start_y' = start_y + y_pp * (double)dy, each two
 *   rounded float64 operations (multiply, then add; never fused); a component equal to 0 leaves that start value's bits untouched.
 *   Ordering is that of adanerf_set_camera: renders issued afterwards see the offset, frames already enqueued keep theirs (the ray
 *   generator's constants reach the kernels by value).  The offset is in pixels and survives adanerf_set_frame_size: it is applied to the
 *   new pixel pitch.
 *   Honoured by adanerf_render, adanerf_render_oracle, adanerf_ray_features, adanerf_sample_mlp and adanerf_sample_uniform.  Ignored,
 *   deliberately, by adanerf_calibrate_guard (its own 64 x 64 rays: the band must not depend on a jitter), adanerf_reproject (it splats
 *   through pixel centres), adanerf_foveate and adanerf_assemble_strips (both index whole pixels).
 *   Sharded contexts, useNDC models, the PDF and coarse/fine samplers, guarded sampling and budget maps need nothing special: the offset
 *   moves the ray inside its pixel, and the maps of adanerf_set_budget_map / adanerf_set_aux_outputs stay indexed by pixel. */
int adanerf_set_pixel_offset(adanerf_ctx* ctx, float dx, float dy);
/* out[0] = dx, out[1] = dy of the offset in force. */
int adanerf_get_pixel_offset(const adanerf_ctx* ctx, float out[2]);

/* Renders this context's rays.  d_rgba8_out: [rays_local] uchar4 (A=255), row-major over the shard's
 * rows -- for shard_world==1 that is the whole image, pixel (x,y) at y*w+x.  d_rgb_f32_out: optional
 * [rays_local,3] fp32 unclamped colour (parity output).  Either may be NULL.  stats != NULL makes
 * the call synchronous and fills the per-stage timings. */
int adanerf_render(adanerf_ctx* ctx, void* d_rgba8_out, float* d_rgb_f32_out, adanerf_stats* stats);

/* Renders only the pixels a mask selects: what a host needs to re-render the disocclusion holes of adanerf_reproject, the rejected pixels
 * of the temporal stages, or any region of interest, at a cost that follows the number of selected pixels.
 *   d_mask       [rays_local] uint8, device memory, caller-owned, indexed as d_rgba8_out is; read, never written
 *   values       pixel p is rendered iff mask[p] < 32 and bit mask[p] of `values` is set.  The mask bytes of adanerf_reproject (0 hole,
 *                1 source, 2 filled) and of adanerf_temporal_resolve / _upsample select directly: values = 1 the holes (the rejected
 *                pixels), values = 5 everything without a source pixel of its own.
 *   d_rgba8_out / d_rgb_f32_out   as adanerf_render's; either may be NULL, not both
 *   stats        NULL or the record of the M rendered rays (rays = M, total_samples = the sum of their counts); makes the call's tail
 *                synchronous as adanerf_render's does
 *   n_rendered   host pointer or NULL: M
 * Contract: every rendered pixel carries, in the colour outputs and in the maps of adanerf_set_aux_outputs / adanerf_set_disp_output, the
 * bytes adanerf_render would write there with the same context state (camera, selection, frame size, pixel offset -- all honoured);
 * every other element of every output keeps the bytes it had.  It holds because every stage is position-invariant per ray, as batched
 * and guarded frames already are byte for byte what unbatched and unguarded ones are.
 * Mechanism: the mask becomes bit words and those an ascending list of ray ids with its count (two launches; deterministic: the same
 * list on every call); M is read back once (4 bytes and one stream synchronisation, as adanerf_reproject's hole count -- the call is
 * never fully asynchronous); the split-precision sampling kernel then generates the listed rays as a dense batch of M, selection,
 * shading and compositing run unchanged on it into context-owned staging buffers, and one launch scatters the pixels.  M above
 * adanerf_info.batch_rays is walked in chunks of batch_rays; M = 0 launches nothing after the list.  Ordering is that of
 * adanerf_set_camera.  ADANERF_BUF_RAY_LIST / _RAY_LIST_COUNT hold the list afterwards; the batch buffers describe the last chunk.
 * A context with ADANERF_SAMPLING_GUARDED renders this call as the split-precision engine (exact, what the guarded frame equals): no
 * first pass and no audit; the band, the audit's phase and the monitor's counters are untouched and rays_refined of the call is 0, as
 * under a budget map.
 * ADANERF_EINVAL, with nothing written: a NULL mask; both colour outputs NULL; values == 0.
 * ADANERF_EUNSUPPORTED, with nothing written and a message naming the reason -- refused, not done by this entry point: the sampling modes
 * ADANERF_SAMPLING_FP16 and _FP32; run-time-shaped sampling networks (anything but 8 x 256 with a 10-4 / 2-2 encoding); a dense
 * context (threshold 0), N above 16, ADANERF_FLAG_KEEP_ORACLE or ADANERF_FLAG_WAVE_SELECT (no fused selection); ADANERF_SAMPLER_PDF and
 * _COARSE_FINE; an installed budget map (its maps are indexed by frame position and would have to be gathered); a shard of a frame
 * (shard_world != 1).  Also not done: re-rendering inside the temporal hosts (extra samples where a full frame exists: a policy for a
 * host to set), and launches sized on the device that would spare the 4-byte read-back. */
int adanerf_render_masked(adanerf_ctx* ctx, const uint8_t* d_mask, uint32_t values, void* d_rgba8_out, float* d_rgb_f32_out,
                          adanerf_stats* stats, int32_t* n_rendered);

/* Secondary outputs of the compositing step (reference: adaptive_raw2outputs / nerf_raw2outputs return them next to the
 * colour, src/nerf_raymarch_common.py:137-139 and :60-62; the viewer has no counterpart): until reset with NULLs, every
 * adanerf_render also fills
 *   d_depth_map [rays_local] fp32   sum_k w_k z_k, z = world depth of the sample as the sampler placed it (NDC depth for
 *                                   useNDC models).  The reference's NeRFOutputDepth is this value under NDC and
 *                                   depth_transform.from_world(.) of it otherwise (src/features.py:571-577); its disp_map:
 *                                   adanerf_set_disp_output
 *   d_acc_map   [rays_local] fp32   sum_k w_k (accumulated opacity)
 * with w_k the compositing weight of sample k (after accumulationMult).  Either may be NULL.  Caller-owned buffers; an
 * adanerf_set_frame_size that changes rays_local resets them to NULL (as it does the maps of adanerf_set_budget_map). */
int adanerf_set_aux_outputs(adanerf_ctx* ctx, float* d_depth_map, float* d_acc_map);

/* The third secondary output of the reference's compositing (disp_map, src/nerf_raymarch_common.py:61 and :138):
 * d_disp_map [rays_local] fp32 = 1 / max(1e-10, depth_map / acc_map), filled by every adanerf_render until reset with NULL
 * (independent of adanerf_set_aux_outputs; a ray with acc_map == 0 gives NaN exactly as the reference's 0 / 0 does). */
int adanerf_set_disp_output(adanerf_ctx* ctx, float* d_disp_map);

/* Per-ray sample budgets: the budget dial of adanerf_set_selection per pixel -- full quality where the viewer looks, fewer samples in the
 * periphery, a cheaper border under dynamic resolution, a caller-made importance mask.
 *   d_n_map   [rays_local] uint8   N of the ray; 0 or a value above the context's N: the context's N
 *   d_thr_map [rays_local] fp32    threshold of the ray; a value not above the context's threshold (a NaN too): the context's threshold
 * both indexed by local ray as d_rgba8_out is, caller-owned, device memory.  Either may be NULL (that half follows the context); both NULL
 * turns the feature off.  The N and the threshold in force are the cap and the floor, evaluated per render, so adanerf_set_selection needs
 * no special case; device data is never "invalid".  Ray r then carries exactly the selection a context with (n_r, thr_r) makes for it:
 * the selection rule keeps a prefix of one order (values descending, lower bin first), so it is a trim of the row the context's own
 * selection wrote -- one small kernel between the selection and the compaction; shading and compositing consume counts and offsets and do
 * not change.  After a render adanerf_stats.total_samples and ADANERF_BUF_RAY_COUNTS / _RAY_OFFSETS / _SAMPLE_KEY / _SAMPLE_W / _TOTAL
 * describe the trimmed selection.
 *   Ordering is that of adanerf_set_camera; the maps are read by the renders issued afterwards at the time their kernels run, so a caller
 *   may rewrite them on the context's stream between frames.  adanerf_set_frame_size resets both to NULL when it changes rays_local.
 *   ADANERF_EUNSUPPORTED, with nothing changed: a context with threshold 0 (dense), ADANERF_SAMPLER_PDF / _COARSE_FINE.  While a map is
 *   installed adanerf_set_selection refuses threshold 0.
 *   ADANERF_SAMPLING_GUARDED: unrefined rays hold the fp16 engine's values, and a trim by them would not be the exact selection, so while a
 *   map is installed the context renders as an ADANERF_SAMPLING_SPLIT_FP16 context: no first pass, no audit, rays_refined 0.  The band,
 *   its source and the audit's phase are left untouched; removing the map resumes guarded rendering. */
int adanerf_set_budget_map(adanerf_ctx* ctx, const uint8_t* d_n_map, const float* d_thr_map);

/* Fills budget maps for this context's local rays from a gaze point (pixels; pixel (x, y) has its centre at (x + 0.5, y + 0.5)) and
 * n_rings concentric rings, in integers: gx2 = lrintf(2 gaze_x), gy2 alike (each clamped to +-2^31);
 * q = (2 x + 1 - gx2)^2 + (2 y + 1 - gy2)^2; ring k contains the pixel iff q <= 4 radius_px[k]^2; the pixel gets (n[k], thr[k]) of the
 * first ring that contains it, else entry n_rings ("outside").  Host arrays: radius_px[n_rings] whole pixels, strictly ascending;
 * n[n_rings + 1] in 0..255; thr[n_rings + 1].  A gaze outside the image, zero rings and rings larger than the image are all legal.
 * d_n_map [rays_local] uint8 / d_thr_map [rays_local] fp32: device buffers, either may be NULL.  Runs on the context's stream; it only
 * fills buffers, installing them is adanerf_set_budget_map.  ADANERF_EINVAL, with nothing written: a NaN / infinite gaze, n_rings outside
 * 0..8, radii negative or not strictly ascending, an n outside 0..255, a NaN thr. */
int adanerf_foveate(adanerf_ctx* ctx, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* n,
                    const float* thr, uint8_t* d_n_map, float* d_thr_map);

/* Hybrid rendering: the neural scene next to rasterised geometry (controllers, hands, avatars, UI panels, a cockpit).  Every ray stops
 * at the depth the rasteriser reports for its pixel; the samples in front of it are composited, the samples at or behind it are never
 * shaded, and adanerf_blend_behind lets the rasterised colour through with the transmittance that is left.  Painting the geometry over
 * a finished frame by comparing against depth_map / acc_map is wrong wherever the scene is semi-transparent in front of the geometry,
 * and pays for every sample nobody sees.
 *   d_limit_zc [rays_local] fp32, device memory, caller-owned, indexed as d_rgba8_out is; NULL turns the feature off.  The value is a
 *   camera-space depth, the distance along the camera's viewing axis: the zc adanerf_reproject writes to d_dst_depth and
 *   adanerf_temporal_resolve to d_out_depth, what adanerf_host_sphere_zc computes; a GL host linearises its depth buffer first
 *   (INTEGRATION.md).
 *   Ordering is that of adanerf_set_camera; the map is read by the renders issued afterwards at the time their kernels run, so a caller may
 *   rewrite it on the context's stream between frames.  adanerf_set_frame_size resets it to NULL when it changes rays_local.
 * Rule (every operation a single rounded fp32 operation in this order; the same inputs give the same bits): entry k of ray r's selected
 * row has bin b; z = ztab[b], the context's depth table (adanerf_host_depth_table); (o, d) = the ray's record in ADANERF_BUF_RAYS (it comes
 * out of the sampling kernel, so the pixel offset in force is honoured); P_i = o_i + d_i z (a product, then a sum); q_i = P_i - pos_i;
 * zc = -((R[2] q_0 + R[5] q_1) + R[8] q_2), pos and R = rot_c2w the pose in force (step 2 of adanerf_temporal_resolve).  The entry is
 * dropped iff zc >= L_r.  So: a NaN limit keeps the whole row and so does +inf (against finite zc); a NaN zc is kept; equality drops; no
 * entry is kept "as a fallback", and a row may become empty.  Survivors stay in ascending bin order with their weights untouched.
 * Mechanism: one small kernel (a thread per ray, rows rewritten in place, the segment totals recomputed by integer sums in a fixed order,
 * no atomics) after the selection -- fused, pair or wave -- and the budget trim, if any, and before the compaction.  With both maps
 * installed ray r carries the budget selection at (n_r, thr_r) with the entries at or behind the limit removed.  Without a limit nothing
 * new is launched: every frame is byte for byte what it was.  Shading and compositing consume counts and offsets and do not change; every
 * shading kernel bounds its tiles by the device total and both compositing kernels loop k < count, so an empty row is legal:
 * d_ray_counts is 0..n_max under a limit, and an empty ray composites to rgb 0, RGBA8 (0, 0, 0, 255), depth_map 0, acc_map 0, disp_map NaN.
 * After a render adanerf_stats.total_samples and ADANERF_BUF_RAY_COUNTS / _RAY_OFFSETS / _SAMPLE_KEY / _SAMPLE_W / _TOTAL describe the
 * trimmed selection.  Measured at 800 x 800, N 8, threshold 0.2 (profiles/depth_limit_measured.md): the trim kernel 11.3 us, and a frame
 * with a quarter / half of its pixels behind a sphere 0.83 / 0.66 of the unlimited frame's time.
 *   ADANERF_SAMPLING_GUARDED needs no special case: the rule reads bins, never values, and guarded bins are exact; the band, the audit and
 *   the monitor are untouched.  Shards: the map is indexed by local ray, as the budget maps are.  adanerf_render_masked works with a limit
 *   installed (the listed ray i reads L[list[i]]): each rendered pixel gets the bytes adanerf_render would write.
 * ADANERF_EUNSUPPORTED, with nothing changed: a dense context (threshold 0: keys are implicit there); ADANERF_SAMPLER_PDF and
 * _COARSE_FINE; a useNDC model (its samples live in NDC space).  While a limit is installed adanerf_set_selection refuses threshold 0.
 * ADANERF_EINVAL: a map that is not 4-byte aligned.
 * What it does not do: NDC models; dense, PDF and coarse/fine contexts; selecting the top N among the visible bins only (the rule trims
 * the selection the context made: a ray whose N best bins all lie behind the surface comes out empty); limits inside the temporal and
 * reprojection stages (their depth is the volume's own); an evaluator mode. */
int adanerf_set_depth_limit(adanerf_ctx* ctx, const float* d_limit_zc);

/* A hard upper bound on the samples a batch may shade: the guarantee "this frame will not cost more than X" that no other dial gives.
 * Frame time is shading time and shading time is linear in the selected samples, whose number follows the view; every other dial
 * (adanerf_set_selection, budget maps, depth limits, the frame size) fixes the inputs of the selection and takes whatever total comes out.
 * The cap is enforced on the device in the same frame, with no read-back, by raising the threshold -- AdaNeRF's own quality knob -- by
 * exactly as much as the bound needs.
 *   mean_samples_per_ray   0 turns the cap off.  Otherwise finite and >= 1, else ADANERF_EINVAL.  A batch of n rays may shade
 *                          C = (int64) floor((double) mean_samples_per_ray * n) samples (>= n: every non-empty row keeps one entry).
 *                          A cap at or above the context's N cannot trim and launches nothing.
 * Rule (exact, in integers on the values' bits), per batch, after the selection -- fused, pair or wave --, the budget trim and the depth
 * limit, immediately before the compaction: row r has c_r entries (0..N; 0 only under a depth limit) with kept values v_rk.  For a
 * threshold t, kept_r(t) = 0 if c_r == 0, else max(1, #{k < c_r : v_rk >= t}) -- an fp32 >=, so a NaN never passes and -0 equals +0;
 * T(t) = sum_r kept_r(t); T_now = sum_r c_r.  If T_now <= C nothing is written: rows, counts and segment totals keep their bytes.
 * Otherwise t* is the smallest non-NaN value present in the batch's rows with T(t*) <= C (-0 taken as +0; +inf if no present value
 * satisfies it: T(+inf) <= n <= C unless a row holds +inf more than once -- such a row keeps every +inf, the one way past C), and every row with more than one entry is trimmed as the budget trim trims a row at (N, t*): the
 * entries with v >= t* survive, the first of the order (value descending, lower bin first) alone if none does; survivors stay in
 * ascending bin order with their values untouched.  Ties at t* make T jump: the rule takes the smallest t that fits, so the result may lie
 * well under C, never above it.  t* >= the context's threshold always.  Trims compose (the kept set of a row is a prefix of one order):
 * with a budget map installed ray r ends with the selection at (n_r, max(thr_r, t*)).
 * Contract: a capped batch is byte for byte the batch the same context renders with no cap and a threshold map filled with t*
 * (adanerf_set_budget_map(ctx, NULL, map)): counts, offsets, keys, kept values, total and image.
 * Mechanism: an exact radix selection of t* over the order-preserving 32-bit keys of the values, 11 + 11 + 10 bits in three passes over the
 * rows; per pass two integer histograms (entries, row maxima: T(t) = entries >= t + non-empty rows - rows whose maximum is >= t), privatised in
 * LDS and flushed with integer atomic adds -- integer sums do not depend on their order, so the same inputs give the same bits; no
 * floating-point atomic -- and a one-workgroup digit search.  Every pass is its own launch, ordered by the stream; t*, T_now and the new
 * total stay in a context-owned device record; the scratch is context-owned, grown on demand and freed by adanerf_destroy.  t* then goes
 * into a context-owned threshold map and the unchanged budget-trim kernels run.  When a batch fits, the later passes return at once.
 * Without a cap nothing new is launched: every frame is byte for byte what it was.  After a render adanerf_stats.total_samples and
 * ADANERF_BUF_RAY_COUNTS / _RAY_OFFSETS / _SAMPLE_KEY / _SAMPLE_W / _TOTAL describe the trimmed selection.
 *   Ordering is that of adanerf_set_camera.  The cap is a scalar, not a per-ray buffer: it survives adanerf_set_selection and
 *   adanerf_set_frame_size.  While a cap is installed adanerf_set_selection refuses threshold 0.
 *   Shards and batches (options.batch_rays): each batch is capped on its own rays, so the bound holds per batch and therefore per frame
 *   (sum of floor(cap * n_b) <= cap * rays_local); t* may differ between batches.
 *   ADANERF_SAMPLING_GUARDED: as under a budget map, the context renders as an ADANERF_SAMPLING_SPLIT_FP16 context while a cap is installed
 *   (the trim reads values, and unrefined rays hold fp16 values): no first pass, no audit, rays_refined 0.  The band, the audit's phase and
 *   the monitor are left untouched; removing the cap resumes guarded rendering.
 * ADANERF_EUNSUPPORTED, with nothing changed: a context with threshold 0 (dense); ADANERF_SAMPLER_PDF and _COARSE_FINE.
 * What it does not do: adanerf_render_masked returns ADANERF_EUNSUPPORTED while a cap is installed (its byte-identity contract with
 * adanerf_render cannot hold when t* depends on which rays are in the batch); one cap across the batches of a frame; spreading the cut by
 * anything other than one threshold per batch; a closed-loop frame-time controller (a few host lines on top of this). */
int adanerf_set_sample_cap(adanerf_ctx* ctx, float mean_samples_per_ray);

/* What the cap did to the last adanerf_render (synchronises the context's stream once):
 *   threshold_max      largest t* over the frame's batches; -inf when no batch was trimmed
 *   batches_trimmed    batches whose T_now exceeded their C
 *   samples_selected   sum of T_now over the batches the cap examined (0 when the cap is at or above N: nothing is launched)
 *   samples_kept       sum of their totals afterwards: <= sum of C */
typedef struct adanerf_cap_report {
  float threshold_max;
  int32_t batches_trimmed;
  int64_t samples_selected;
  int64_t samples_kept;
} adanerf_cap_report;
int adanerf_sample_cap_report(adanerf_ctx* ctx, adanerf_cap_report* out);

/* The second half of hybrid rendering: per pixel t = 1 - acc (one fp32 subtraction); !(t > 0) gives t = 0 (a NaN too); t > 1 gives t = 1;
 * t == 0: out = rgb, the bits copied (a NaN in the behind image cannot leak); otherwise out_c = rgb_c + t * behind_c, a product, then a
 * sum, each rounded to fp32.
 *   d_rgb [n,3] fp32 / d_acc [n] fp32: d_rgb_f32_out and the acc_map of a render under a depth limit; d_behind_rgb [n,3] fp32: the
 *   rasterised colour (anything where the limit is +inf: acc decides what shows)
 *   d_out_rgb [n,3] fp32 or NULL, may be d_rgb itself; d_out_rgba8 [n] uchar4 or NULL, adanerf_resolve_mean's byte contract
 * One launch on the context's stream, no host synchronisation; independent of the context's frame size (as adanerf_accumulate is);
 * n == 0 does nothing.  Measured: 5.4 us for 640 000 pixels with the RGBA8 output (profiles/depth_limit_measured.md).
 * ADANERF_EINVAL, with nothing written: a NULL input; both outputs NULL; n < 0 or n * 3 beyond 2^31 - 1; a pointer that is not 4-byte
 * aligned; an output overlapping an input (only d_out_rgb == d_rgb is legal) or the other output. */
int adanerf_blend_behind(adanerf_ctx* ctx, const float* d_rgb, const float* d_acc, const float* d_behind_rgb, int32_t n, float* d_out_rgb,
                         void* d_out_rgba8);

/* Foveated ray density: the second half of foveation.  adanerf_foveate lowers the samples per ray away from the gaze; this lowers the
 * rays.  The mask below is dense at the gaze and thins to every 2nd, 4th or 8th pixel per axis outside it, adanerf_render_masked(d_mask, 1,
 * ..) renders exactly its lattice, and adanerf_fill_density rebuilds the pixels in between.
 *   radius_px[n_rings]  adanerf_foveate's rules: whole pixels, strictly ascending, n_rings in 0..8
 *   stride[n_rings + 1] each 1, 2, 4 or 8, never decreasing from one entry to the next; the last entry applies outside every ring
 *   d_mask              [height*width] uint8, device memory, at the context's current frame size, indexed as d_rgba8_out is
 * One launch on the context's stream, no host synchronisation.  Definition, in integers only:
 *   ring      adanerf_foveate's rule unchanged: gx2 = lrintf(2 gaze_x), gy2 alike, clamped as there; q = (2 x + 1 - gx2)^2 + (2 y + 1 - gy2)^2;
 *             ring k contains the pixel iff q <= 4 radius_px[k]^2; s(x, y) = stride[k] of the first ring that contains it, else stride[n_rings]
 *   rendered  pixel (x, y) iff some level L of 1, 2, 4, 8 passes all of: L divides x; L divides y; s(nx, ny) <= L, where (nx, ny) is the
 *             pixel of the box [max(x - L + 1, 0), min(x + L - 1, w - 1)] x [max(y - L + 1, 0), min(y + L - 1, h - 1)] whose centre lies
 *             nearest the gaze: per axis the integer c of the interval that minimises |2 c + 1 - gx2|, the lower c on a tie.  Strides never
 *             decrease outward, so that pixel carries the smallest stride of the box.
 *   byte      0 for a rendered pixel; every other pixel gets its own stride s(x, y), which is 2, 4 or 8
 * A pixel on the lattice of its own ring passes at L = s (the box contains it); beyond that every lattice point of stride L is rendered as
 * soon as any pixel within L - 1 of it per axis belongs to a ring of stride L or finer, also a point that sits in a coarser ring.  That
 * closes the pattern at ring borders: every corner adanerf_fill_density reads is a rendered pixel, for any gaze, radii and frame size.
 * At 800 x 800 with radii 120 / 300 and strides 1 / 2 / 4 the mask renders 127 399 of 640 000 pixels (19.9 %).
 * ADANERF_EINVAL, with nothing written: a NULL mask or array; a gaze that is not finite; n_rings outside 0..8; radii negative or not
 * strictly ascending; a stride outside {1, 2, 4, 8} or a decreasing one.
 * ADANERF_EUNSUPPORTED, with nothing written: shard_world != 1 (the reconstruction needs a pixel's neighbours; adanerf_render_masked
 * refuses shards too). */
int adanerf_foveate_density(adanerf_ctx* ctx, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride,
                            uint8_t* d_mask);

/* The reconstruction: one launch on the context's stream, a gather, in place.
 *   d_mask [height*width] uint8; d_rgb [height*width,3] fp32, required; d_depth_map / d_acc_map [height*width] fp32 and d_rgba8
 *   [height*width] uchar4, each may be NULL.  width and height are arguments, independent of the context's frame size (as
 *   adanerf_present's are).
 * Per pixel (x, y) with mask byte s:
 *   s not in {2, 4, 8}: nothing of the pixel is touched, in any image (0 is a rendered pixel; any other value is free for a caller's marks)
 *   otherwise the corners are x0 = x & ~(s - 1); x1 = x0 + s, but x1 = x0 if x == x0 or x0 + s >= width; y alike; the used corners are the
 *   distinct ones among (x0 | x1, y0 | y1).  A used corner whose mask byte is not 0: the pixel is left untouched and counted in
 *   *unfilled_out -- 0 with a mask of adanerf_foveate_density; with any other mask the result is still deterministic, because a thread
 *   reads only pixels of byte 0 and no thread writes those.
 *   fx = (float)(x - x0) / (float)s, fy alike (both exact); per channel top = c00 + fx (c01 - c00), bot = c10 + fx (c11 - c10),
 *   out = top + fy (bot - top), c01 the corner at (x1, y0), c10 at (x0, y1): each step a subtraction, a product and a sum, each rounded
 *   to fp32 and never fused.  On an axis where the two taps are the same pixel that step is skipped and the value's bits are copied (an
 *   infinity does not turn into a NaN that way).
 *   d_depth_map and d_acc_map get the same interpolation (both are sums over the samples and so linear in the weights); d_rgba8 of a
 *   filled pixel is adanerf_resolve_mean's byte contract applied to `out`.
 * unfilled_out: the 4-byte counter shared with adanerf_reproject; with a non-NULL pointer the call is synchronous, with NULL the images
 * are complete after adanerf_sync().  Measured at 800 x 800 with radii 120 / 300 and strides 1 / 2 / 4
 * (profiles/foveated_density_measured.md): the mask kernel 7 us, the fill kernel 12.5 us with the RGBA8 image, the whole frame -- masked
 * render and fill -- 1.12 ms where adanerf_render takes 4.91 ms.
 * ADANERF_EINVAL, with nothing written: a NULL mask or d_rgb; a side outside 1..16384; an fp32 or uchar4 pointer that is not 4-byte
 * aligned; images that overlap one another or the mask.
 * What it does not do: combine with budget maps (the hosts refuse the pair: a ray's budget would have to be reconstructed too); an
 * edge-aware or depth-aware filter (the blend is bilinear across depth edges); anything specific to useNDC models (their depth_map is
 * interpolated as a number like any other); sizing launches on the device (the ray count of the masked render is read back once per frame,
 * as adanerf_render_masked does). */
int adanerf_fill_density(adanerf_ctx* ctx, const uint8_t* d_mask, int32_t width, int32_t height, float* d_rgb, float* d_depth_map,
                         float* d_acc_map, void* d_rgba8, int32_t* unfilled_out);

/* The lattice with a phase: the two calls above are phase (0, 0) of these and write the same bytes.  phase_x, phase_y in 0..7.
 *   lattice   pixel (x, y) lies on the lattice of level L iff ((x - phase_x) & (L - 1)) == 0 and ((y - phase_y) & (L - 1)) == 0 (two's
 *             complement: the residue of x - phase_x mod L, also where the difference is negative).  The rest of the rule -- the ring
 *             test, the box of L - 1 around the point clipped to the frame, its pixel nearest the gaze having stride <= L -- is unchanged.
 *   cell      of a pixel with byte s: m = (x - phase_x) & (s - 1), x0 = x - m, x1 = x0 + s.  Two taps iff m != 0, x0 >= 0 and x1 < width,
 *             with fx = (float)m / (float)s; otherwise one tap: x0 if m == 0, else x0 if x0 >= 0, else x1 if x1 < width.  If neither
 *             exists (a frame narrower than the stride) the pixel is left untouched and counted in *unfilled_out.  y alike.  The used
 *             corners are the distinct ones among the taps; the blend is adanerf_fill_density's.
 * A corner lies within s - 1 of every pixel that uses it (m <= s - 1; x1 - x = s - m <= s - 1 where m != 0), so the closure above holds for
 * every phase: every corner the fill uses is a rendered pixel.
 * adanerf_host_density_phase gives the phase of frame k; over its 64 phases every pixel of a frame is rendered at least once, and a pixel
 * whose ring has stride L at least once in any L^2 consecutive frames.
 * ADANERF_EINVAL / ADANERF_EUNSUPPORTED, with nothing written: what the unphased calls refuse; a phase outside 0..7. */
int adanerf_foveate_density_phased(adanerf_ctx* ctx, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px, const int32_t* stride,
                                   int32_t phase_x, int32_t phase_y, uint8_t* d_mask);
int adanerf_fill_density_phased(adanerf_ctx* ctx, const uint8_t* d_mask, int32_t width, int32_t height, int32_t phase_x, int32_t phase_y,
                                float* d_rgb, float* d_depth_map, float* d_acc_map, void* d_rgba8, int32_t* unfilled_out);

/* De-interleaves the gathered shard payloads ([shard_world][rays_local_max] uchar4, rank-major)
 * into the full row-major image [h*w] uchar4. */
int adanerf_assemble_strips(adanerf_ctx* ctx, const void* d_gathered, void* d_image_out);

/* Single-process multi-GPU exchange (the counterpart of the RCCL gather for a host that owns all N contexts, e.g. the
 * `adanerf` CLI with --gpus N): copies `bytes` from d_src (a buffer of src's device, produced on src's stream) to d_dst
 * on dst's device -- hipMemcpyPeerAsync over xGMI, peer access enabled on first use -- ordered behind src's stream, and
 * makes dst's stream wait for it.  No host synchronisation.  src == dst or same device: a device-to-device copy. */
int adanerf_gather_to(adanerf_ctx* dst, void* d_dst, adanerf_ctx* src, const void* d_src, size_t bytes);

int adanerf_sync(adanerf_ctx* ctx);

/* Makes the context enqueue on a caller-owned HIP stream (hipStream_t, e.g. PyTorch's current stream)
 * instead of its own; NULL restores the context's stream.  The caller keeps the stream alive. */
int adanerf_set_stream(adanerf_ctx* ctx, void* hip_stream);

/* Asynchronous per-stage timing: with profiling on, every adanerf_render() records HIP events on the
 * context's stream without synchronising; adanerf_collect_stats() synchronises once and returns the
 * SUM over all frames rendered since the previous collect (stats->batches counts batches,
 * shade_launches / sample_launches the kernel launches behind the summed durations). */
int adanerf_set_profiling(adanerf_ctx* ctx, int32_t enabled);
int adanerf_collect_stats(adanerf_ctx* ctx, adanerf_stats* stats, int32_t* frames);

/* ---- stage-level entry points (mirror the reference launchers; used by the parity tests) ---- */

/* Oracle-net input features [n_rays, n_in0] fp32 = [PE(dir/|dir|) | PE(p)] and the per-ray record
 * d_rays_out [n_rays, 8] fp32 = (origin.xyz, 0, dir.xyz, 0) handed to the shading stage (sphere-exit
 * point and un-normalised world direction; NDC-space origin/direction when useNDC).  first_ray
 * indexes this context's local ray list.  Either output may be NULL. */
int adanerf_ray_features(adanerf_ctx* ctx, int32_t first_ray, int32_t n_rays,
                         float* d_features_out, float* d_rays_out);

/* Fused ray generation + PE + sampling MLP -> raw oracle values [n_rays,128] fp32 (+ ray records).  A model with
 * multiDepthFeatures = D < 128 fills bins D..127 with -1e30 ("absent": never selected). */
int adanerf_sample_mlp(adanerf_ctx* ctx, int32_t first_ray, int32_t n_rays,
                       float* d_oracle_out, float* d_rays_out);

/* Adaptive selection + deterministic compaction of arbitrary oracle values.
 *   d_oracle       [n_rays,128] fp32
 *   n_max, thr     N and threshold (thr > 0)
 *   d_ray_offsets  [n_rays] int32  exclusive prefix sum of counts (ray-major)
 *   d_ray_counts   [n_rays] int32  1..n_max
 *   d_sample_key   [>= n_rays*n_max] uint32  (local_ray << 7) | bin, ray-major, bins ascending
 *   d_sample_w     [>= n_rays*n_max] fp32    oracle value of the kept bin: the value the sampler ranked, i.e. AFTER the sigmoid
 *                                            (losses[0] = BCEWithLogitsLoss) or the softmax over the bins (CrossEntropyLoss[Weighted])
 *                                            of the context's model; the raw value of d_oracle under every other loss, and always
 *                                            in the dense mode (thr == 0 ranks nothing).  Under the two transforming losses it never
 *                                            reaches compositing: only NeRFWeightMultiplicationLoss multiplies by it (mult_mode is 0
 *                                            otherwise).  The softmax's last bits depend on the selection kernel.
 *   d_total        [1] int32       S
 * thr == 0 selects the dense mode (all 128 bins; n_max must be 128). */
int adanerf_compact(adanerf_ctx* ctx, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr,
                    int32_t* d_ray_offsets, int32_t* d_ray_counts, uint32_t* d_sample_key,
                    float* d_sample_w, int32_t* d_total);

/* The guarded two-precision selection (ADANERF_SAMPLING_GUARDED) on caller-provided values, for tests: selects from
 * d_oracle_approx [n_rays,128] with the guard band (eps, eps_pair <= 0 -> 2 eps), lists the undecided rays plus the rays audited at
 * (audit_period, audit_phase) (audit_period <= 0: none; audit_fill_cap > 0: only as many of them as fill the last round of
 * audit_fill_cap rays, the window chosen by audit_cycle -- ADANERF_FLAG_GUARD_AUDIT_FILL), re-selects the undecided ones from d_oracle_exact [n_rays,128], compares
 * the audited decided ones, then compacts.  If the two bounds hold on every row the outputs equal adanerf_compact(d_oracle_exact, ...)
 * except that d_sample_w holds the approximate values on the rays that were not re-selected.  d_refined [1] int32: how many rays
 * were looked at again.  d_monitor (may be NULL) [5] uint32, ADDED to / maximised into (the caller zeroes it): [0] float bits of
 * the largest |approx - exact| over the re-evaluated rows, [1] rows that exceeded a bound, [2] float bits of the largest
 * (kept - candidate) difference error, [3] audited rows whose approximate selection differs from the exact one, [4] audited rows.
 * n_max <= 16, thr > 0.
 * Under the context's sampler transform: eps always bounds the RAW values, |approx - exact| <= eps per entry of d_oracle_*; the rule runs
 * on the transformed values with the band e = eps (no transform), eps / 4 (sigmoid), 1.01 (exp(2 eps) - 1) x the approximate row's largest
 * probability (softmax), and the pair bound 2 e -- eps_pair is honoured without a transform only.  If the raw bound holds, counts, offsets,
 * total and keys are those of adanerf_compact(d_oracle_exact, ...) bit for bit under every transform; d_sample_w holds the transformed
 * exact values on the re-selected rays and the transformed approximate ones (within e of them) elsewhere; a row with a NaN or an infinity
 * is always re-selected.  The monitor reports in RAW units under every transform: [0] and the bound of [1] are raw differences against
 * eps; under a transform no pair bound is in use and [2] stays 0. */
int adanerf_compact_guarded(adanerf_ctx* ctx, const float* d_oracle_approx, const float* d_oracle_exact, int32_t n_rays,
                            int32_t n_max, float thr, float eps, float eps_pair, int32_t audit_period, int32_t audit_phase,
                            int32_t audit_fill_cap, int32_t audit_cycle, int32_t* d_ray_offsets, int32_t* d_ray_counts, uint32_t* d_sample_key, float* d_sample_w,
                            int32_t* d_total, int32_t* d_refined, uint32_t* d_monitor);

/* adanerf_compact with per-ray budgets, for tests: the selection at (n_max, thr), then the trim of ray r to d_n_map[r] / d_thr_map[r] (the
 * rules of adanerf_set_budget_map; either map may be NULL), then the compaction.  thr > 0.  Honours ADANERF_FLAG_WAVE_SELECT and
 * n_max > 16 as adanerf_compact does.  Outputs as adanerf_compact. */
int adanerf_compact_budget(adanerf_ctx* ctx, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr, const uint8_t* d_n_map,
                           const float* d_thr_map, int32_t* d_ray_offsets, int32_t* d_ray_counts, uint32_t* d_sample_key,
                           float* d_sample_w, int32_t* d_total);

/* adanerf_compact with a depth limit, for tests: the selection at (n_max, thr), then the trim of ray r to the entries with zc < d_limit_zc[r]
 * (the rule of adanerf_set_depth_limit, with d_rays [n_rays,8] the ray records -- 16-byte aligned --, pos / rot_c2w the pose, and the
 * context's depth table in force), then the compaction.  thr > 0.  Honours ADANERF_FLAG_WAVE_SELECT and n_max > 16 as adanerf_compact
 * does.  Outputs as adanerf_compact, with d_ray_counts 0..n_max. */
int adanerf_compact_depth_limit(adanerf_ctx* ctx, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr, const float* d_rays,
                                const float* d_limit_zc, const float pos[3], const float rot_c2w[9], int32_t* d_ray_offsets,
                                int32_t* d_ray_counts, uint32_t* d_sample_key, float* d_sample_w, int32_t* d_total);

/* adanerf_compact with a sample cap, for tests: the selection at (n_max, thr); the budget trim if d_n_map / d_thr_map is given (either or both
 * may be NULL); the depth trim if d_limit_zc is given (then d_rays, pos and rot_c2w as in adanerf_compact_depth_limit; all four may be NULL);
 * the cap of adanerf_set_sample_cap with C = cap_total (>= n_rays, else ADANERF_EINVAL); the compaction.  thr > 0.  Honours
 * ADANERF_FLAG_WAVE_SELECT and n_max > 16 as adanerf_compact does.  Outputs as adanerf_compact, plus d_tstar [1] fp32 device: the t* the
 * cap chose, -inf if nothing was trimmed. */
int adanerf_compact_cap(adanerf_ctx* ctx, const float* d_oracle, int32_t n_rays, int32_t n_max, float thr, const uint8_t* d_n_map,
                        const float* d_thr_map, const float* d_rays, const float* d_limit_zc, const float pos[3], const float rot_c2w[9],
                        int64_t cap_total, int32_t* d_ray_offsets, int32_t* d_ray_counts, uint32_t* d_sample_key, float* d_sample_w,
                        int32_t* d_total, float* d_tstar);

/* Calibrates the band of ADANERF_SAMPLING_GUARDED for the loaded model: n_poses cameras drawn inside the view cell
 * (positions uniform in 90 % of it, any orientation; seeded), 64 x 64 rays covering the field of view each, through both the
 * plain-fp16 and the split-precision sampling network; *max_diff = the largest |difference| over all raw outputs, *max_pair_diff
 * (may be NULL) = the largest error of a (kept - candidate) difference under the context's N and threshold with the single-value
 * bound that max_diff gives (0 where the sampler transforms its values).
 * set != 0 also installs max(ADANERF_GUARD_CALIB_MARGIN * max_diff, ADANERF_GUARD_EPS_MIN) and ADANERF_GUARD_CALIB_MARGIN *
 * max_pair_diff as the context's bounds -- what a context created with guard_eps <= 0 does by itself before its first guarded
 * frame (ADANERF_GUARD_CALIB_POSES poses, seed 1) unless the model directory holds a current calibration record of at least that
 * many poses -- and writes the record (see adanerf_guard_calibration_file; a record measured over more poses is left alone).
 * Synchronous.  8 x 256 sampling networks only. */
int adanerf_calibrate_guard(adanerf_ctx* ctx, int32_t n_poses, uint32_t seed, int32_t set, float* max_diff, float* max_pair_diff);

/* Path of the calibration record of this context's (model, N, threshold): <model_dir>/guard_band.n<N>.t<threshold bits>.cal, or
 * under $ADANERF_GUARD_CACHE_DIR/<model hash>/ when that variable is set (read-only model directories).  A text file (key = value):
 * hash of model0.onnx, the encoding, the sampler transform, the revision of the fp16 engine, poses, seed, the measured maxima.  Read
 * at the first guarded frame of a context created with guard_eps <= 0; a record of another model / engine revision is ignored
 * and overwritten.  Delete it to force a new measurement.  buf may be NULL to query the length (return value: bytes needed
 * including the terminator, or a negative ADANERF_E* code). */
int adanerf_guard_calibration_file(const adanerf_ctx* ctx, char* buf, size_t buf_bytes);

/* Explicit shading-net input features [n_samples, n_in1] fp32 = [PE(x^) | PE(dir)] (parity/debug;
 * the render path never materialises them). */
int adanerf_shade_features(adanerf_ctx* ctx, const float* d_rays, const uint32_t* d_sample_key,
                           int32_t n_samples, float* d_features_out);

/* Fused PE + shading MLP over compacted samples -> raw [rgb, alpha] fp32 [n_samples,4].
 * d_total (device int32) bounds the work without a host sync; max_samples bounds the launch.
 * precision: ADANERF_PREC_*, or -1 for the context's.
 * Positions: a sample whose (normalised) position o + d z is not finite in every component -- a NaN or an infinity in the ray record
 * or in the depth -- gets NaN in all four raw outputs, in every precision (the compositing stages then make the ray non-finite); every
 * other sample of the launch is unaffected.  ADANERF_PREC_BF16 runs a packing whose per-layer scaling is proved for |x_i| <= 4096 only
 * (what adanerf_create and adanerf_set_camera check for a bf16 context's own samples): a finite position beyond that also gets four
 * NaNs there, never a clamped value; fp16 and fp32 evaluate it like any other. */
int adanerf_shade_mlp(adanerf_ctx* ctx, const float* d_rays, const uint32_t* d_sample_key,
                      const int32_t* d_total, int32_t max_samples, int32_t precision, float* d_raw_out);

/* As adanerf_shade_mlp with an explicit world depth per sample (d_sample_z [S] fp32, may be NULL -> the bin
 * centre of sample_key's bin): the inverse-CDF sampler places samples anywhere inside a bin.  The depths are the caller's: one that
 * is NaN or infinite, or (ADANERF_PREC_BF16) takes the position beyond |x_i| <= 4096, gives that sample four NaNs as stated at
 * adanerf_shade_mlp -- also when the call names bf16 in a context created with another precision, where nothing checked the scene. */
int adanerf_shade_mlp_z(adanerf_ctx* ctx, const float* d_rays, const uint32_t* d_sample_key, const float* d_sample_z,
                        const int32_t* d_total, int32_t max_samples, int32_t precision, float* d_raw_out);

/* Debug view of the sampling network (reference: copyResultSamplingNetwork(output, surf, batch_size, batch_offset,
 * width, 128), include/cuda/adanerf_cuda_kernels.cuh:20-21 -> samplesToImage, src/cuda/base_cuda_kernels.cu:487-528;
 * the viewer's 'O' key, src/inputhandler.cpp:76): per ray the three bins with the largest raw outputs, largest
 * first (equal values: lower bin first), written as RGBA8 ((0.5 + bin) / 128 * 255, truncated; A = 255).
 * d_rgba8 [n_rays] uchar4. */
int adanerf_copy_result_sampling_network(adanerf_ctx* ctx, const float* d_oracle, int32_t n_rays, void* d_rgba8);

/* Whole-frame version of the above for this rank's rays (ImageGenerator::inference with render_oracle set,
 * src/imagegenerator.cpp:316-317): sampling MLP, then the view; the shading half is skipped. */
int adanerf_render_oracle(adanerf_ctx* ctx, void* d_rgba8);

/* DONeRF sampler (reference: updateRayMarchFromPoses / samplePDF, include/cuda/adanerf_cuda_kernels.cuh:47-52,
 * src/cuda/base_cuda_kernels.cu:296-372; PyTorch: FromClassifiedDepth + nerf_sample_pdf): n samples per ray by
 * inverting the CDF of sigmoid(oracle) + 1e-5 at u = k/(n+1).  Outputs as adanerf_compact plus d_sample_z
 * [n_rays*n] world depths; counts are all n; sample_w is zero-filled. */
int adanerf_sample_pdf(adanerf_ctx* ctx, const float* d_oracle, int32_t n_rays, int32_t n, int32_t* d_ray_offsets,
                       int32_t* d_ray_counts, uint32_t* d_sample_key, float* d_sample_w, float* d_sample_z,
                       int32_t* d_total);

/* Vanilla NeRF, coarse pass (reference: updateRayMarchCoarse, include/cuda/adanerf_cuda_kernels.cuh:60-66; PyTorch:
 * RayMarchFromPoses over LinearlySpacedZNearZFar, src/features.py:380-480, src/nerf_raymarch_common.py:295-331): rays of
 * [batch_offset, batch_offset + n_rays) from the camera position (d_rays [n,8]) and Nc samples per ray at the model's uniform
 * depth table (d_sample_key = ray << 7 | k, counts all Nc).  ADANERF_SAMPLER_COARSE_FINE contexts only. */
int adanerf_sample_uniform(adanerf_ctx* ctx, int32_t batch_offset, int32_t n_rays, float* d_rays, int32_t* d_ray_offsets,
                           int32_t* d_ray_counts, uint32_t* d_sample_key, int32_t* d_total);

/* The coarse network (model0.onnx, a NeRF net in this mode) on samples made by adanerf_sample_uniform: as adanerf_shade_mlp. */
int adanerf_shade_mlp_coarse(adanerf_ctx* ctx, const float* d_rays, const uint32_t* d_sample_key, const int32_t* d_total,
                             int32_t max_samples, int32_t precision, float* d_raw);

/* Vanilla NeRF, fine sampler (reference: updateRayMarchFromCoarse incl. nerf_raw_2_output_weights, adanerf_cuda_kernels.cuh:68-74,
 * src/cuda/coarse_cuda_kernels.cu:29-383; PyTorch: RayMarchFromCoarse.batch, src/features.py:640-672): the coarse raw outputs
 * [n_rays*Nc,4] -> nerf_raw2outputs weights -> nerf_sample_pdf over the interval mid-points with weights[1:-1], u =
 * linspace(0,1,Nf) -> merged with the coarse depths, ascending.  d_sample_z [n_rays*(Nc+Nf)] world depths for
 * adanerf_shade_mlp_z; counts are all Nc + Nf. */
int adanerf_sample_from_coarse(adanerf_ctx* ctx, const float* d_raw_coarse, const float* d_rays, int32_t n_rays, int32_t* d_ray_offsets,
                               int32_t* d_ray_counts, uint32_t* d_sample_key, float* d_sample_z, int32_t* d_total);

/* Classic NeRF compositing over a fixed n samples per ray (reference: copyResultRaymarch / nerf_raw_2_output,
 * adanerf_cuda_kernels.cuh:23-24; PyTorch nerf_raw2outputs): alpha = 1 - exp(-relu(raw.a) * dz * |dir|). */
int adanerf_composite_classic(adanerf_ctx* ctx, const float* d_raw, const float* d_sample_z, const float* d_rays,
                              int32_t n_rays, int32_t n, float* d_rgb_out, void* d_rgba8_out);

/* Per-ray front-to-back compositing: c = sigmoid(raw.rgb), a = sigmoid(raw.a) * w.  Ray r composites the d_ray_counts[r] samples
 * from d_ray_offsets[r] on; any layout is accepted (the compactor's ray-major one takes a staged fast path with the same result, bit
 * for bit).  Contract: in a context with num_samples > 32 one wave composites a ray and every lane holds two samples, so
 * d_ray_counts[r] must not exceed the context's num_samples (at most 128); samples beyond 128 are not read. */
int adanerf_composite(adanerf_ctx* ctx, const float* d_raw, const float* d_sample_w,
                      const int32_t* d_ray_offsets, const int32_t* d_ray_counts, int32_t n_rays,
                      float* d_rgb_out, void* d_rgba8_out);

/* adanerf_composite that also writes the secondary outputs of the step (src/nerf_raymarch_common.py:136-141): d_depth_out [n_rays]
 * fp32 = sum w z and d_acc_out [n_rays] fp32 = sum w over the ray's samples, w the weight the colour is formed with (under
 * accumulationMult = weights it carries the multiplier) and z the context's depth table at the bin of d_sample_key [S] (key & 127).
 * Either map may be NULL and is then not touched; with both NULL this is adanerf_composite.  The colours are those of adanerf_composite,
 * bit for bit.  d_sample_key may be NULL only in a dense context (threshold 0), where it means "bin = sample index & 127" (every ray
 * carries all 128 bins in order); NULL in any other context with a map requested returns ADANERF_EINVAL and writes nothing. */
int adanerf_composite_aux(adanerf_ctx* ctx, const float* d_raw, const float* d_sample_w, const int32_t* d_ray_offsets,
                          const int32_t* d_ray_counts, const uint32_t* d_sample_key, int32_t n_rays, float* d_rgb_out, void* d_rgba8_out,
                          float* d_depth_out, float* d_acc_out);

/* adanerf_composite_classic that also writes depth_map = sum w z (z = d_sample_z of the sample) and acc_map = sum w
 * (src/nerf_raymarch_common.py:60-62) into d_depth_out / d_acc_out [n_rays] fp32; either may be NULL and is then not touched. */
int adanerf_composite_classic_aux(adanerf_ctx* ctx, const float* d_raw, const float* d_sample_z, const float* d_rays, int32_t n_rays,
                                  int32_t n, float* d_rgb_out, void* d_rgba8_out, float* d_depth_out, float* d_acc_out);

/* disp_map of src/nerf_raymarch_common.py:61 / :138 from the two maps above: d_disp_out[i] = 1 / max(1e-10, d_depth[i] / d_acc[i]),
 * n fp32 values each, on the context's stream.  max is torch.max: the NaN of an empty ray (0 / 0) stays NaN.  n = 0 does nothing;
 * a NULL pointer or n < 0 returns ADANERF_EINVAL. */
int adanerf_disp_map(adanerf_ctx* ctx, const float* d_depth, const float* d_acc, int32_t n, float* d_disp_out);

/* ---- image metrics ---- */

/* FLIP (Andersson et al. 2020) between two images as the reference's evaluation computes it (src/evaluate.py:120-145 over
 * src/util/flip_loss.py:61-105): both images to YCxCz (sRGB clamped to [0, 1] first); colour pipeline = contrast-sensitivity filters
 * A / RG / BY (replicate padding) -> clamped linear RGB -> L*a*b* -> Hunt adjustment -> HyAB ^ 0.7 -> redistribute_errors (pc 0.4,
 * pt 0.95, cmax computed in fp64); feature pipeline = edge and point detectors on (Y + 16) / 116 in x and transposed;
 * map = dE_c ^ (1 - dE_f) per pixel (IEEE pow: 0 ^ 0 = 1), mean = its average.  The metric is symmetric in the two images.
 *   d_test_rgb, d_ref_rgb  [height*width,3] fp32, row-major, sRGB: the layout of adanerf_render's d_rgb_f32_out; values outside
 *                          [0, 1] are clamped as the reference clamps them, a NaN reaches every map pixel within the filter radius
 *                          and the mean
 *   width, height          of the two images; independent of the context's frame size; width * height <= 2^30
 *   pixels_per_degree      <= 0 selects the reference's 0.7 * (3840 / 0.7) * pi / 180 = 67.02; supported: 10 .. 140 (filter radii up to
 *                          19 / 18 pixels); anything else returns ADANERF_EINVAL -- a filter is never truncated
 *   d_error_map            [height*width] fp32 or NULL
 *   mean_out               host pointer or NULL; non-NULL makes the call synchronous, with NULL the map is complete after adanerf_sync()
 * Runs on the context's stream; filter tables and per-tile sums live in context-owned scratch, grown on demand and freed by
 * adanerf_destroy.  One fused kernel per 32 x 32 tile plus a fixed-order reduction (no floating-point atomics): the same inputs give the
 * same bits. */
int adanerf_flip(adanerf_ctx* ctx, const float* d_test_rgb, const float* d_ref_rgb, int32_t width, int32_t height,
                 float pixels_per_degree, float* d_error_map, float* mean_out);

/* adanerf_present flags */
enum {
  ADANERF_PRESENT_FLIP_Y = 1,  /* rows are written bottom-up: the reference's destination rectangle (GL's origin) and the BMP row order */
  ADANERF_PRESENT_NEAREST = 2, /* force the nearest filter */
  ADANERF_PRESENT_LINEAR = 4,  /* force the linear filter; together with _NEAREST: ADANERF_EINVAL */
  ADANERF_PRESENT_AREA = 8     /* the exact area (box) filter, below; together with _NEAREST or _LINEAR: ADANERF_EINVAL */
};

/* The frame at the window's size: the headless counterpart of the viewer's blit from its render buffer (-s W H) to the window (-ws W H),
 * src/interoprenderbuffer.cpp:87 -- linear filtering on both axes if dst_w > src_w, nearest otherwise, as there.  With
 * adanerf_set_frame_size this is dynamic resolution: a frame rendered at a reduced size reaches the caller at the window's size without
 * leaving the device.
 *   d_src_rgba8 [src_h*src_w] uchar4, d_dst_rgba8 [dst_h*dst_w] uchar4, both row-major and 4-byte aligned; every side in 1..16384; the
 *   two ranges must not overlap.  Independent of the context's frame size (as adanerf_flip); runs on the context's stream.
 *   flags: ADANERF_PRESENT_*; 0 gives a top-down image filtered by the rule above.
 * GL leaves the rounding of a linear blit to the implementation; this library defines it in integers (the same bits on every call).
 * Per axis, with D = 2 dst_w:  n = (2 x + 1) src_w - dst_w,  i0 = floor(n / D),  f = n - i0 D;  the taps are i0 and i0 + 1 clamped to the
 * edge, their weights D - f and f (samples at pixel centres: equal sizes give the identity); y alike with E = 2 dst_h.  Per channel,
 * alpha included, v = the sum of the four weighted taps and out = floor((2 v + D E) / (2 D E)).  Nearest takes pixel
 * min(floor((2 x + 1) src_w / D), src_w - 1).  A NULL pointer, a side outside 1..16384, both filter flags, an unknown flag, a pointer
 * that is not 4-byte aligned or overlapping ranges return ADANERF_EINVAL.
 *   ADANERF_PRESENT_AREA: supersampling in space.  The blit of src/interoprenderbuffer.cpp:87 decimates a frame rendered larger than the
 *   window (nearest); this filter averages it instead, exactly, for any pair of sizes.  Per axis, in units of 1 / dst_w of a source pixel:
 *   destination pixel x covers [x src_w, (x + 1) src_w), source pixel i covers [i dst_w, (i + 1) dst_w), the weight is the overlap
 *   wx(x, i) = max(0, min((i + 1) dst_w, (x + 1) src_w) - max(i dst_w, x src_w)); the contributing i run from floor(x src_w / dst_w) to
 *   floor(((x + 1) src_w - 1) / dst_w) and their weights sum to src_w; wy alike.  Per channel, alpha included, V = sum_j sum_i wy wx v,
 *   S = src_w src_h and out = floor((2 V + S) / (2 S)): rounded half up, in 64-bit integers.  Equal sizes give the identity, a constant
 *   image stays constant, an exact 2 x reduction is the half-up rounded mean of each 2 x 2 block; enlarging is legal (the definition covers
 *   it).  The filter needs src_w <= 8 dst_w and src_h <= 8 dst_h (at most 9 taps per axis), else ADANERF_EINVAL: reduce in two steps.
 *   _FLIP_Y combines with it as with the other filters.  Without the flag nothing changes: the default for dst_w <= src_w stays nearest. */
int adanerf_present(adanerf_ctx* ctx, const void* d_src_rgba8, int32_t src_w, int32_t src_h, void* d_dst_rgba8, int32_t dst_w,
                    int32_t dst_h, int32_t flags);

/* Supersampling in time: the running sum of the fp32 frames rendered at several sub-pixel offsets (adanerf_set_pixel_offset), and its
 * mean.  The viewer has no counterpart (one ray through each pixel centre, src/util/raygeneration.py:10-26).  Both run on the context's
 * stream without a host synchronisation and are independent of the context's frame size (as adanerf_present is); n_rays == 0 does nothing.
 *   adanerf_accumulate:   d_rgb_f32 [n_rays,3] is the d_rgb_f32_out of an adanerf_render, d_sum [n_rays,3] caller-owned.  first != 0:
 *                         sum = rgb; otherwise sum = sum + rgb, one rounded fp32 addition per value (a NaN propagates).
 *   adanerf_resolve_mean: m = sum / (float)frames, one IEEE fp32 division per value, frames in 1..65536.  d_rgb_f32_out [n_rays,3] or NULL
 *                         receives m and may be d_sum itself; d_rgba8_out [n_rays] uchar4 or NULL receives the viewer's output contract as
 *                         the compositing step writes it, (unsigned char)(fminf(fmaxf(m, 0), 1) * 255.0f) and A = 255 (a NaN becomes 0):
 *                         with frames == 1 the d_rgb_f32_out of a render resolves to that render's d_rgba8_out byte for byte.
 * ADANERF_EINVAL, with nothing written: a NULL d_rgb_f32 / d_sum, both outputs NULL; n_rays < 0 or n_rays * 3 beyond 2^31 - 1; frames
 * outside 1..65536; a pointer that is not 4-byte aligned; images that overlap without being identical (d_rgb_f32 and d_sum, d_sum and
 * d_rgb_f32_out), d_rgba8_out overlapping either fp32 image. */
int adanerf_accumulate(adanerf_ctx* ctx, const float* d_rgb_f32, int32_t n_rays, float* d_sum, int32_t first);
int adanerf_resolve_mean(adanerf_ctx* ctx, const float* d_sum, int32_t n_rays, int32_t frames, void* d_rgba8_out, float* d_rgb_f32_out);

/* Adaptive supersampling: the extra sub-pixel renders go only to the pixels that sit on an edge.  Three calls beside
 * adanerf_render_masked, which renders an arbitrary pixel set at a cost that follows its size:
 *
 * adanerf_contrast_mask -- which pixels of a rendered fp32 frame need more rays.  One launch on the context's stream; width and height are
 * arguments, independent of the context's frame size (as adanerf_present's are), sides in 1..16384.
 *   d_rgb    [height*width,3] fp32, interleaved, row-major: the d_rgb_f32_out of a render
 *   d_mask   [height*width] uint8, any alignment
 * Definition, exact:
 *   display value  v(p, ch) = fminf(fmaxf(d_rgb[3 p + ch], 0), 1), the clamp of adanerf_resolve_mean's byte contract: a NaN is 0, an
 *                  infinity is 0 or 1
 *   contrast       c(p, q) = max over ch of |v(p, ch) - v(q, ch)|, each difference one rounded fp32 subtraction
 *   flagged        p iff some q among its up to 8 neighbours inside the image has c(p, q) > threshold; the comparison is strict and in
 *                  fp32.  A 1 x 1 image flags nothing.  The relation is symmetric, so both sides of an edge are flagged and no dilation
 *                  pass is needed
 *   byte           d_mask[p] = 0 if flagged (render more), 1 otherwise: the convention of adanerf_reproject's holes and of the density
 *                  mask's 0, so adanerf_render_masked(ctx, d_mask, 1, ..) selects the flagged pixels directly
 *   n_flagged      a host pointer or NULL.  Given, it receives the number of 0 bytes, at the cost of one 4-byte read-back and one stream
 *                  synchronisation (as adanerf_reproject's hole count); NULL keeps the call asynchronous
 * With threshold 0 every pixel that differs from a neighbour at all is flagged; with 1 none is (no clamped difference exceeds 1).
 * ADANERF_EINVAL, with nothing written: a NULL d_rgb or d_mask; a side outside 1..16384; a threshold that is not finite or lies outside
 * [0, 1]; a d_rgb that is not 4-byte aligned; a d_mask that overlaps d_rgb.
 *
 * adanerf_accumulate_masked / adanerf_resolve_mean_masked -- adanerf_accumulate / adanerf_resolve_mean for the pixels a mask selects.
 * The selection is adanerf_render_masked's, word for word: pixel p iff d_mask[p] < 32 and bit d_mask[p] of `values` is set
 * (d_mask [n_rays] uint8).  A selected pixel gets exactly what the unmasked call computes: one rounded fp32 addition per value (or the
 * copy, first != 0); one IEEE division by (float)frames and the byte contract above.  Every element of every other pixel -- in d_sum,
 * d_rgb_f32_out and d_rgba8_out -- keeps its bytes and is not read.
 * ADANERF_EINVAL, with nothing written: everything the unmasked call refuses; a NULL mask; values == 0; a mask that overlaps an image
 * the call writes.
 *
 * The frame the hosts build from them (NeuralRenderer.render_supersampled_adaptive, --supersample S --supersample-contrast T): one render
 * at offset (0, 0) fills the output images (the centre frame); adanerf_contrast_mask runs on its fp32 colour; if any pixel is flagged, the
 * S * S offsets of adanerf_host_subpixel_grid(S, k) are walked in order, each adanerf_render_masked(values = 1) into a staging image and
 * adanerf_accumulate_masked into the sum (first at k = 0); adanerf_resolve_mean_masked then writes the mean of the flagged pixels over the
 * centre frame.  A flagged pixel carries, byte for byte, what the full S x S supersampling gives it; an unflagged pixel, byte for byte,
 * what adanerf_render gives it (which is why the centre frame is a render of its own and not the grid's offset 0).  The aux and
 * disparity maps are switched off for the masked passes, so they describe the centre frame whole.  Limits are adanerf_render_masked's.
 * What it does not do: a depth or opacity criterion in the rule; progressive refinement (detecting again after each pass); coupling to
 * adanerf_reproject or the temporal stages; launches sized on the device (the masked render reads its ray count back once per pass). */
int adanerf_contrast_mask(adanerf_ctx* ctx, const float* d_rgb, int32_t width, int32_t height, float threshold, uint8_t* d_mask,
                          int32_t* n_flagged);
int adanerf_accumulate_masked(adanerf_ctx* ctx, const float* d_rgb_f32, const uint8_t* d_mask, uint32_t values, int32_t n_rays,
                              float* d_sum, int32_t first);
int adanerf_resolve_mean_masked(adanerf_ctx* ctx, const float* d_sum, const uint8_t* d_mask, uint32_t values, int32_t n_rays,
                                int32_t frames, void* d_rgba8_out, float* d_rgb_f32_out);

/* adanerf_reproject flags */
enum { ADANERF_REPROJECT_FILL = 1 }; /* a destination pixel no source pixel lands in takes the farthest of its 8 neighbours' source pixels */

/* Depth reprojection (timewarp): the last rendered frame warped to the pose of the moment, for a host whose display rate or pose latency
 * must not follow the render rate (a head-tracked or 120 Hz host between two renders).  The viewer has no counterpart: NeuralRenderer::render
 * (src/neuralrenderer.cpp:146-182) hands the frame it rendered to the blit of src/interoprenderbuffer.cpp:87, and this stage sits in
 * front of that present step (adanerf_present may follow it).  Inputs are what one adanerf_render of this context wrote: the RGBA8 frame,
 * the depth_map and acc_map of adanerf_set_aux_outputs, and the pose it was rendered at.
 *   d_src_rgba8 [height*width] uchar4, d_src_depth_map / d_src_acc_map [height*width] fp32; src_pos / src_rot_c2w: the pose of that frame
 *   dst_pos / dst_rot_c2w   the pose to warp to (conventions of adanerf_set_camera; the camera in force is neither read nor changed)
 *   acc_min                 a source pixel with acc_map < acc_min has no surface ("far"); 0 is legal
 *   hole_rgba8              colour of a destination pixel nothing reaches: the pixel's four bytes as a little-endian word (R lowest)
 *   flags                   0 or ADANERF_REPROJECT_FILL
 *   d_dst_rgba8 [height*width] uchar4; d_dst_depth [height*width] fp32 or NULL; d_dst_mask [height*width] uint8 or NULL
 *   holes_out               host pointer or NULL: the number of pixels with mask 0; non-NULL makes the call synchronous (as mean_out of
 *                           adanerf_flip), with NULL the outputs are complete after adanerf_sync()
 * All images have the context's CURRENT frame size (the ray generator's constants belong to it) and are indexed as adanerf_render's
 * output is; the colour images are 4-byte aligned.  d_dst_depth may be d_src_depth_map; the two colour images must not overlap.
 * Definition (every operation a single rounded fp32 operation in this order; the same inputs give the same bits on every call):
 *   splat, source pixel i = row*width + col: (nds, p) = this context's ray of that pixel at the source pose; o = p, the view-cell sphere
 *   exit (ADANERF_SAMPLER_ADAPTIVE / _PDF), or src_pos (ADANERF_SAMPLER_COARSE_FINE) -- the origin in ADANERF_BUF_RAYS.  a = acc_map[i],
 *   t = depth_map[i] / a.  The pixel is far if !(a >= acc_min), if t is not finite or if !(t > 0) (NaNs are far).  q = (o + nds t) - dst_pos
 *   for a near pixel, q = nds for a far one (direction only: the sky follows the rotation alone).  v_k = (R[k] q_0 + R[3+k] q_1) + R[6+k] q_2
 *   with R = dst_rot_c2w (its transpose applied), zc = -v_2; dropped unless zc is finite and > 0.  u = (focal v_0) / zc + 0.5 width,
 *   vv = (focal (-v_1)) / zc + 0.5 height, focal = adanerf_info.focal (pixel pitch 1); dropped unless 0 <= u < width and 0 <= vv < height.
 *   The pixel lands in (floor(u), floor(vv)) with the key (bits(zc) << 32 | i), bits = 0x7F800000 (+inf) for a far pixel; the smallest key
 *   of a destination pixel wins (a 64-bit integer atomic minimum: nearest surface, lower source index on a tie; no floating-point atomics).
 *   resolve, destination pixel j: with a winner, its source pixel's colour, mask 1, depth = the winner's zc (+inf for a far winner).
 *   Without one and with ADANERF_REPROJECT_FILL: among the 8 neighbours' winners (never filled results) the LARGEST key -- the farthest
 *   surface, the usual choice behind a disocclusion -- gives colour and depth, mask 2.  Otherwise hole_rgba8, depth 0, mask 0.
 * What it does not do: a splat covers one pixel, so background can show through the cracks of a magnified foreground (a forward move);
 * view-dependent colour stays that of the source pose.  The holes are re-rendered by adanerf_render_masked(d_dst_mask, 1, d_dst_rgba8, ..)
 * with the camera at the destination pose (values 5: the filled pixels too).
 * Runs on the context's stream in three launches (clear, splat, resolve); the z-buffer and the hole count live in context-owned scratch,
 * grown on demand (the stream is synchronised only then), never shrunk, freed by adanerf_destroy; adanerf_render never allocates them.
 * ADANERF_EINVAL, with nothing written: a NULL source image, destination colour or pose; a pose entry that is not finite; acc_min NaN or
 * negative; an unknown flag; a colour image that is not 4-byte aligned; destination colour overlapping the source colour.
 * ADANERF_EUNSUPPORTED, with nothing written: a useNDC model (its depth_map is NDC depth); a context with shard_world != 1. */
int adanerf_reproject(adanerf_ctx* ctx, const void* d_src_rgba8, const float* d_src_depth_map, const float* d_src_acc_map,
                      const float src_pos[3], const float src_rot_c2w[9], const float dst_pos[3], const float dst_rot_c2w[9],
                      float acc_min, uint32_t hole_rgba8, int32_t flags, void* d_dst_rgba8, float* d_dst_depth, uint8_t* d_dst_mask,
                      int32_t* holes_out);

/* adanerf_reproject_gather flags */
enum { ADANERF_GATHER_GUESS = 1 }; /* a pixel whose iteration stayed inside the source frame but failed the consistency test keeps its gathered colour, mask 2 */

/* Gather reprojection: adanerf_reproject's warp done from the destination's side, with only the source frame's depth.  Each destination
 * pixel searches its own ray for the source surface by a fixed-point iteration -- guess a depth on the ray, look where that point lies in
 * the source frame, take the surface found there as the next guess -- so a pixel is a hole only where the source frame has nothing (a
 * disocclusion, the frame's border), never because no splat happened to land on it, and the colour is a bilinear tap of the fp32 frame.
 * adanerf_reproject is unchanged and stays every host's default.  Inputs are what one adanerf_render of this context wrote.
 *   d_src_rgb [height*width,3] fp32 (d_rgb_f32_out), d_src_depth_map / d_src_acc_map [height*width] fp32 (adanerf_set_aux_outputs);
 *                           src_pos / src_rot_c2w: the pose of that frame
 *   dst_pos / dst_rot_c2w   the pose to warp to (conventions of adanerf_set_camera; the camera in force is neither read nor changed)
 *   acc_min                 as adanerf_reproject's; depth_tol >= 0: relative tolerance of the consistency test; iterations in 1..8
 *   hole_rgba8              as adanerf_reproject's: the four bytes of a mask-0 pixel in d_dst_rgba8
 *   flags                   0 or ADANERF_GATHER_GUESS
 *   d_dst_rgb [height*width,3] fp32; d_dst_rgba8 [height*width] uchar4, d_dst_depth [height*width] fp32, d_dst_mask [height*width] uint8:
 *                           each may be NULL
 *   holes_out               host pointer or NULL: the number of pixels with mask 0; non-NULL makes the call synchronous (as holes_out of
 *                           adanerf_reproject), with NULL the outputs are complete after adanerf_sync()
 * All images have the context's CURRENT frame size and are indexed as adanerf_render's output is; fp32 and uchar4 images are 4-byte aligned;
 * no output may overlap a source image or another output.
 * Definition (every operation a single rounded fp32 operation in this order, over the float64 ray table; a gather: the same inputs give
 * the same bits on every call):
 *   1 source surface, source pixel i   (nds, p) = this context's ray of the pixel at the source pose through the pixel centre; o = p, or
 *               src_pos (ADANERF_SAMPLER_COARSE_FINE).  a = acc_map[i], t = depth_map[i] / a; near by adanerf_reproject's test (a >= acc_min,
 *               t finite, t > 0; NaNs are far).  near: S_i = o + nds t, q = S_i - src_pos, zs_i = -((R[2] q_0 + R[5] q_1) + R[8] q_2),
 *               R = src_rot_c2w.  far: no point, zs_i = +inf (a near pixel whose zs comes out +inf counts as far from here on).
 *   2 destination ray, destination pixel j   d = the nds of this context's ray of j at the destination pose through the pixel centre (the
 *               offset of adanerf_set_pixel_offset is ignored, as adanerf_reproject ignores it).
 *   3 iteration   tap_0 = j.  For k = 0 .. iterations - 1: if tap_k is near, s = ((S_x - dst_x) d_x + (S_y - dst_y) d_y) + (S_z - dst_z) d_z
 *               with S = S_tap_k; the pixel dies unless s is finite and > 0; P = dst_pos + d s, q = P - src_pos.  If tap_k is far, q = d
 *               (direction only: the sky follows the rotation alone).  v_k = (R[k] q_0 + R[3+k] q_1) + R[6+k] q_2 with R = src_rot_c2w,
 *               zc = -v_2, u = (focal v_0) / zc + 0.5 width, vv = (focal (-v_1)) / zc + 0.5 height; the pixel dies unless zc is finite
 *               and > 0, 0 <= u < width and 0 <= vv < height.  tap_k+1 = floor(vv) width + floor(u).  A dead pixel stays dead.
 *   4 consistency, against the last zc and the final tap   a near estimate (the last tap_k was near) is consistent iff the final tap is near
 *               and |zc - zs_tap| <= depth_tol * zc; a far estimate iff the final tap is far.
 *   5 result    the colour tap is adanerf_temporal_resolve's step 5 on d_src_rgb at the last (u, vv).  Alive and consistent: that colour,
 *               mask 1, depth = -((D[2] r_0 + D[5] r_1) + D[8] r_2) with r = P - dst_pos, D = dst_rot_c2w (+inf for a far estimate).
 *               Alive, not consistent, ADANERF_GATHER_GUESS: the same colour and depth, mask 2.  Everything else: fp32 (0, 0, 0), hole_rgba8,
 *               mask 0, depth 0.  d_dst_rgba8 of a mask 1 / 2 pixel follows adanerf_resolve_mean's byte contract.
 * The mask bytes mean to adanerf_render_masked what adanerf_reproject's mean: values 1 re-renders the holes, 5 the unverified pixels too.
 * What it does not do: a thin foreground object that the start guess (the same pixel) never sees can be missed; bilinear taps blend across
 * depth edges; view-dependent colour stays that of the source pose; the scene is static; no depth limit; no useNDC models, no shards.
 * A depth_tol below the relative depth step per pixel of a sloped surface cannot verify it (the iteration ends in a 2-cycle between two
 * taps).  And on a trained network's noisy depth it does not beat the splat (profiles/reproject_gather_measured.md, 800 x 800, 4 iterations,
 * depth_tol 0.05): not in PSNR as warped (19.99 against 20.09 dB), not in pixels left to re-render once the unverified ones count (32.9 %
 * both); it leaves fewer holes (11.1 against 14.0 %) but is 1.3 dB worse once those are re-rendered, at two thirds of the splat's time.
 * At 1920 x 1080 it is 0.3 dB better as warped.  The iteration follows the depth's noise: one iteration scores highest as warped.
 * Runs on the context's stream in two launches (source surfaces, warp); the surface table (16 bytes per pixel) lives in context-owned
 * scratch beside the hole count, grown on demand (the stream is synchronised only then), never shrunk, freed by adanerf_destroy;
 * adanerf_render never allocates for it.
 * ADANERF_EINVAL, with nothing written: a NULL source image, pose or d_dst_rgb; a pose entry that is not finite; acc_min or depth_tol NaN
 * or negative; iterations outside 1..8; an unknown flag; a misaligned fp32 or uchar4 pointer; an output overlapping a source image or
 * another output.
 * ADANERF_EUNSUPPORTED, with nothing written: a useNDC model (its depth_map is NDC depth); a context with shard_world != 1. */
int adanerf_reproject_gather(adanerf_ctx* ctx, const float* d_src_rgb, const float* d_src_depth_map, const float* d_src_acc_map,
                             const float src_pos[3], const float src_rot_c2w[9], const float dst_pos[3], const float dst_rot_c2w[9],
                             float acc_min, float depth_tol, int32_t iterations, uint32_t hole_rgba8, int32_t flags, float* d_dst_rgb,
                             void* d_dst_rgba8, float* d_dst_depth, uint8_t* d_dst_mask, int32_t* holes_out);

/* Two-source reprojection (bidirectional frame interpolation): two rendered frames A and B warped to a pose between them.  A disocclusion
 * is a region ONE source frame never saw, so no single-source warp can fill it with real data; a frame behind and a frame ahead uncover
 * each other's.  For a host that has the frame after the in-between pose already: one that replays a script, evaluates a pose list, or
 * shows its frames K calls late.  Inputs are what two adanerf_render calls of this context wrote.
 *   d_a_rgb / d_b_rgb [height*width,3] fp32 (d_rgb_f32_out), d_*_depth_map / d_*_acc_map [height*width] fp32 (adanerf_set_aux_outputs);
 *                           a_pos / a_rot_c2w, b_pos / b_rot_c2w: the pose of each render.  A and B may be the same buffers
 *   dst_pos / dst_rot_c2w   the pose to warp to (conventions of adanerf_set_camera; the camera in force is neither read nor changed)
 *   weight_b                in [0, 1]: the share of B where both sources see the same surface (adanerf_host_pair_weight)
 *   acc_min, hole_rgba8     as adanerf_reproject's; depth_tol >= 0: relative tolerance of the agreement test
 *   flags                   0 or ADANERF_REPROJECT_FILL
 *   d_dst_rgb [height*width,3] fp32; d_dst_rgba8 [height*width] uchar4, d_dst_depth [height*width] fp32, d_dst_mask and d_dst_source
 *                           [height*width] uint8: each of the four may be NULL
 *   holes_out               as adanerf_reproject's: the number of pixels with mask 0; non-NULL makes the call synchronous
 * All images have the context's CURRENT frame size and are indexed as adanerf_render's output is; fp32 and uchar4 images are 4-byte aligned;
 * no output may overlap a source image or another output.
 * Definition (every operation a single rounded fp32 operation in this order; the same inputs give the same bits on every call):
 *   splat, per source s in {A, B}: adanerf_reproject's splat verbatim on that source's maps and pose (the far test, the direction-only
 *               far pixels, v, zc, u, vv, the key bits(zc) << 32 | i under a 64-bit integer minimum), each source into its own z-buffer
 *               Z_s, bit for bit what adanerf_reproject builds for that source.
 *   resolve, destination pixel j: k_s = Z_s[j], z_s the float in its high word (+inf for a far winner), i_s its low word.
 *     both have a winner   they agree iff both are far, or both are near and |zA - zB| <= depth_tol * min(zA, zB) (a subtraction, fabs,
 *               fmin, a multiplication, a comparison).  Agreement: per channel c = cA + weight_b * (cB - cA) (a subtraction, a
 *               multiplication, an addition) with c_s the colour of source pixel i_s; depth the same expression on zA, zB, +inf when both
 *               are far; mask 1, source 3.  Disagreement (one far and one near winner too): the source with the smaller high word wins --
 *               in a static scene the nearer surface occludes the other in the destination view -- its colour and depth, mask 1, source 1
 *               (A) or 2 (B).
 *     one has a winner     that source's colour and depth, mask 1, source 1 or 2.
 *     neither, with ADANERF_REPROJECT_FILL   the candidates are the winners in the 8 neighbours of j in both z-buffers, up to 16 keys,
 *               never filled results; the LARGEST key (the farthest surface, as in adanerf_reproject) gives colour and depth; B's largest is
 *               taken iff it is larger than A's largest, so A wins on equal keys; mask 2, source 1 or 2.
 *     otherwise            fp32 (0, 0, 0), hole_rgba8, depth 0, mask 0, source 0.
 *   d_dst_rgba8 of a mask 1 / 2 pixel follows adanerf_resolve_mean's byte contract.
 * The mask bytes mean exactly what adanerf_reproject's mean (0 hole, 1 own source pixel, 2 neighbour-filled), so
 * adanerf_render_masked(d_dst_mask, 1 or 5, ..) works on the result unchanged; provenance is in d_dst_source for that reason.
 * What it does not do: the scene is static (a moving object is warped as if it stood still); view-dependent colour is a blend of the two
 * source poses'; a host that uses it lags K frames or knows its path in advance; a splat covers one pixel, as adanerf_reproject's; no
 * useNDC models, no shards.  Against the one-source warp on a trained network's depth (profiles/reproject_pair_measured.md: two renders a
 * tenth of the view cell apart, the two poses between them, 800 x 800): 0.5 % holes against 5.2 / 9.8 %, 25.3 / 25.5 dB against 20.3 / 19.6 dB
 * as shown, 26.0 / 26.1 against 21.7 / 22.1 dB with the holes re-rendered; one pair call takes 0.6 of the time of two adanerf_reproject calls.
 * Unlike the gather, it helps on that depth: its data is a second real frame, not a better search of the first.
 * Runs on the context's stream in three launches (one clear over both z-buffers and the hole count, one splat of both sources side by
 * side, one resolve); the second z-buffer lives in the context-owned scratch that holds adanerf_reproject's, grown on demand (the stream
 * is synchronised only then), never shrunk, freed by adanerf_destroy; adanerf_render never allocates it.
 * ADANERF_EINVAL, with nothing written: a NULL source image, pose or d_dst_rgb; a pose entry that is not finite; weight_b NaN or outside
 * [0, 1]; acc_min or depth_tol NaN or negative; an unknown flag; a misaligned fp32 or uchar4 pointer; an output overlapping a source image
 * or another output.
 * ADANERF_EUNSUPPORTED, with nothing written: a useNDC model (its depth_map is NDC depth); a context with shard_world != 1. */
int adanerf_reproject_pair(adanerf_ctx* ctx, const float* d_a_rgb, const float* d_a_depth_map, const float* d_a_acc_map, const float a_pos[3],
                           const float a_rot_c2w[9], const float* d_b_rgb, const float* d_b_depth_map, const float* d_b_acc_map,
                           const float b_pos[3], const float b_rot_c2w[9], const float dst_pos[3], const float dst_rot_c2w[9], float weight_b,
                           float acc_min, float depth_tol, uint32_t hole_rgba8, int32_t flags, float* d_dst_rgb, void* d_dst_rgba8,
                           float* d_dst_depth, uint8_t* d_dst_mask, uint8_t* d_dst_source, int32_t* holes_out);

/* adanerf_temporal_resolve flags */
enum { ADANERF_TEMPORAL_CLAMP = 1 }; /* the history colour is clamped to the min / max of the current colour over the pixel's 3 x 3 neighbourhood */

/* Temporal anti-aliasing: the stage a real-time host runs on every frame between adanerf_render and its present step.  A history image is
 * carried to the pose of the moment by the new frame's own depth, tested for disocclusion, clamped to what the new frame can justify and
 * blended with the new frame, which the host renders at the next sub-pixel offset of a small cycle (adanerf_set_pixel_offset,
 * adanerf_host_subpixel_grid): one render per displayed frame converges to the supersampled still while the camera rests and stays
 * anti-aliased while it moves.  The viewer has no counterpart: NeuralRenderer::render (src/neuralrenderer.cpp:146-182) hands each frame to
 * the blit of src/interoprenderbuffer.cpp:87 as rendered.
 *   d_cur_rgb [height*width,3] fp32, d_cur_depth_map / d_cur_acc_map [height*width] fp32: what one adanerf_render at cur_pos / cur_rot_c2w
 *                           wrote (d_rgb_f32_out and the maps of adanerf_set_aux_outputs)
 *   d_hist_rgb [height*width,3] fp32, d_hist_depth [height*width] fp32, d_hist_count [height*width] uint8: what the previous call wrote to
 *                           d_out_rgb / d_out_depth / d_out_count, at prev_pos / prev_rot_c2w.  Caller-owned: a host ping-pongs two sets.
 *                           d_hist_rgb NULL: no history (the first frame, a cut) -- every pixel is rejected and the previous pose is not
 *                           read (it may be NULL).  d_hist_depth NULL: no disocclusion test.  d_hist_count NULL: constant alpha.
 *   alpha                   weight of the new frame, in (0, 1]; depth_tol >= 0: relative depth tolerance of the disocclusion test;
 *                           acc_min >= 0: as adanerf_reproject's; flags: 0 or ADANERF_TEMPORAL_CLAMP
 *   d_out_rgb [height*width,3] fp32; d_out_depth, d_out_count, d_out_rgba8 ([height*width] uchar4), d_out_mask ([height*width] uint8):
 *                           each may be NULL
 *   rejected_out            host pointer or NULL: the number of pixels with mask 0; non-NULL makes the call synchronous (as holes_out of
 *                           adanerf_reproject), with NULL the outputs are complete after adanerf_sync()
 * All images have the context's CURRENT frame size and are indexed as adanerf_render's output is; fp32 and uchar4 images are 4-byte aligned.
 * Definition, per destination pixel j = (x, y) (every operation a single rounded fp32 operation in this order; a gather: the same inputs
 * give the same bits on every call):
 *   1 surface   (nds, p) = this context's ray of the pixel at the current pose through the pixel CENTRE (the offset of
 *               adanerf_set_pixel_offset is ignored, deliberately, as adanerf_reproject ignores it); o = p, or cur_pos
 *               (ADANERF_SAMPLER_COARSE_FINE).  a = acc_map[j], t = depth_map[j] / a; near by adanerf_reproject's test (a >= acc_min, t
 *               finite, t > 0; NaNs are far).
 *   2 own depth near: P = o + nds t, q = P - cur_pos, zc_cur = -((R[2] q_0 + R[5] q_1) + R[8] q_2), R = cur_rot_c2w; far: +inf.  Written to
 *               d_out_depth[j] whatever becomes of the history.
 *   3 previous camera   adanerf_reproject's splat arithmetic with dst = prev: q = P - prev_pos (near) or nds (far), v_k, zc, u, vv as there;
 *               rejected unless zc is finite and > 0, 0 <= u < width and 0 <= vv < height.  The nearest tap is floor(vv) * width + floor(u).
 *   4 disocclusion (d_hist_depth given)   hd = d_hist_depth[nearest tap]; a near pixel is accepted iff hd is finite and
 *               |zc - hd| <= depth_tol * zc, a far pixel iff hd == +inf.
 *   5 history colour   fx = u - 0.5, x0 = floor(fx), wx = fx - x0, taps x0 and x0 + 1 clamped to 0 .. width - 1; y alike.  Per channel
 *               top = c00 + wx (c01 - c00), bot = c10 + wx (c11 - c10), hst = top + wy (bot - top): a subtraction, a product, a sum each.
 *   6 clamp (ADANERF_TEMPORAL_CLAMP)   per channel lo / hi = the minimum / maximum of d_cur_rgb over the pixels of j's 3 x 3 neighbourhood
 *               that exist; a NaN is skipped (all NaN: lo = hi = NaN), -0 orders below +0.  hst = min(max(hst, lo), hi) by the same rules:
 *               a NaN bound leaves hst as it is, a NaN hst takes the bound.
 *   7 count     accepted: n' = min(d_hist_count[nearest tap] + 1, 255); rejected, or without d_hist_count: n' = 1.  d_out_count[j] = n'.
 *               a_eff = fmaxf(alpha, 1.0f / (float)n') with d_hist_count, alpha without: a running mean until 1 / n' falls below alpha.
 *   8 blend     accepted: out = hst + a_eff (cur - hst), mask 1; rejected: out = cur, the bits copied, mask 0.  d_out_rgba8 follows
 *               adanerf_resolve_mean's byte contract.
 * What it does not do: rejected pixels show the new frame's single jittered sample -- more samples for them are a host's choice
 * (adanerf_render_masked(d_out_mask, 1, ..) at further offsets; neither host does it); the current frame is not un-jittered; no variance
 * clipping; the scene is static.
 * Runs on the context's stream in one launch; its only context-owned scratch is the 4-byte counter it shares with adanerf_reproject (made
 * on first use, freed by adanerf_destroy); adanerf_render never allocates for it.
 * ADANERF_EINVAL, with nothing written: a NULL current image, map, current pose or d_out_rgb; a NULL previous pose with a history; a pose
 * entry that is read and not finite; alpha outside (0, 1] or NaN; depth_tol or acc_min negative or NaN; an unknown flag; a misaligned
 * pointer; d_out_rgb overlapping d_hist_rgb or d_cur_rgb, d_out_depth overlapping d_hist_depth, d_out_count overlapping d_hist_count.
 * ADANERF_EUNSUPPORTED, with nothing written: a useNDC model; a context with shard_world != 1. */
int adanerf_temporal_resolve(adanerf_ctx* ctx, const float* d_cur_rgb, const float* d_cur_depth_map, const float* d_cur_acc_map,
                             const float cur_pos[3], const float cur_rot_c2w[9], const float* d_hist_rgb, const float* d_hist_depth,
                             const uint8_t* d_hist_count, const float prev_pos[3], const float prev_rot_c2w[9], float alpha, float depth_tol,
                             float acc_min, int32_t flags, float* d_out_rgb, float* d_out_depth, uint8_t* d_out_count, void* d_out_rgba8,
                             uint8_t* d_out_mask, int32_t* rejected_out);

/* Temporal upsampling: the frame is rendered at the context's frame size w x h with a sub-pixel offset and resolved into a history of
 * W x H = s w x s h, s = scale in 1..4: s^2 times fewer rays per displayed frame, the full-resolution image rebuilt over the s^2 offsets
 * of adanerf_host_subpixel_grid(s, .).  adanerf_temporal_resolve with two sizes and a neighbourhood depth test; that entry point is
 * unchanged.  The viewer has no counterpart: it blits the frame it rendered (src/interoprenderbuffer.cpp:87).
 *   d_cur_rgb [h*w,3], d_cur_depth_map / d_cur_acc_map [h*w] fp32: what one adanerf_render at cur_pos / cur_rot_c2w wrote with the pixel
 *                           offset (cur_dx, cur_dy) in force; the offset is this call's argument and never read from the context
 *   d_hist_rgb [H*W,3] fp32, d_hist_depth [H*W] fp32, d_hist_count [H*W] uint8: what the previous call wrote, at prev_pos / prev_rot_c2w.
 *                           d_hist_rgb NULL: no history -- every pixel has mask 0 and the previous pose is not read.  d_hist_depth NULL:
 *                           no disocclusion test.  d_hist_count NULL: constant alpha.
 *   alpha, depth_tol, acc_min, flags, rejected_out: as adanerf_temporal_resolve's
 *   d_out_rgb [H*W,3] fp32; d_out_depth [H*W] fp32, d_out_count [H*W] uint8, d_out_rgba8 [H*W] uchar4, d_out_mask [H*W] uint8: each may be NULL
 * All images are row-major; fp32 and uchar4 images are 4-byte aligned.  G_lo is the context's ray generator with (cur_dx, cur_dy) applied
 * exactly as adanerf_set_pixel_offset defines, at the current pose; G_hi is the generator a context of this model has at frame size W x H,
 * at pixel centres and the current pose, focal_hi its focal length as fp32.  Definition (every operation a single rounded fp32 operation
 * in this order; a gather: the same inputs give the same bits on every call):
 * Pass A, per render pixel i = (x, y), only when d_hist_rgb and d_hist_depth are both given: (nds, p) = G_lo's ray of the pixel; o = p, or
 *   cur_pos (ADANERF_SAMPLER_COARSE_FINE).  a = acc[i], t = depth[i] / a; near by adanerf_reproject's test.  near: P = o + nds t,
 *   q = P - prev_pos, zp[i] = -((R[2] q_0 + R[5] q_1) + R[8] q_2), R = prev_rot_c2w.  Far, or a zp that is not finite: zp[i] = +inf.
 * Pass B, per output pixel J = (X, Y):
 *   1 sample    cx = ((float)X + 0.5f) / (float)s - cur_dx, ix = floor(cx) clamped to 0 .. w - 1; iy alike from cy; i = iy w + ix: the
 *               render pixel whose jittered sample lies nearest the output pixel's centre.  ex = (((float)ix + 0.5f) + cur_dx) (float)s -
 *               ((float)X + 0.5f), ey alike: the sample's distance from that centre in output pixels.  k = fmaxf(0, 1 - |ex|)
 *               fmaxf(0, 1 - |ey|); inside = |ex| <= 0.5 and |ey| <= 0.5; cur = d_cur_rgb[i].
 *   2 surface and own depth   (nds, p) = G_hi's ray of (X, Y); o as in pass A; a, t and near from render pixel i; P = o + nds t; zc_cur as
 *               adanerf_temporal_resolve's step 2 (+inf if far), written to d_out_depth[J] whatever becomes of the history.
 *   3 previous camera   adanerf_temporal_resolve's step 3 with W, H and focal_hi; tap = floor(vv) W + floor(u).
 *   4 disocclusion (d_hist_depth given)   hd = d_hist_depth[tap].  Over the pixels of i's 3 x 3 render-size neighbourhood that exist: zmin /
 *               zmax = the smallest / largest finite zp, any_far = some zp is +inf.  hd == +inf: accepted iff any_far.  hd finite: accepted
 *               iff a finite zp exists and zmin - depth_tol zmin <= hd <= zmax + depth_tol zmax (a product, then a difference / sum).  Any
 *               other hd: rejected.  The depths compared are those of one camera, so half a pixel of jitter between two renders of one
 *               pose rejects nothing that a neighbour's surface explains.
 *   5 history colour   four bilinear taps at W x H, as adanerf_temporal_resolve's step 5.
 *   6 clamp (ADANERF_TEMPORAL_CLAMP)   lo / hi = minimum / maximum of d_cur_rgb over i's 3 x 3 render-size neighbourhood, by the order rules
 *               of adanerf_temporal_resolve's step 6; hst = min(max(hst, lo), hi).
 *   7 count     with d_hist_count: hc = d_hist_count[tap], live = accepted and hc >= 1; live: n' = min(hc + inside, 255), a_eff =
 *               k fmaxf(alpha, 1.0f / (float)n'); not live: n' = inside.  Without: live = accepted, a_eff = k alpha, n' = live or inside.
 *               d_out_count[J] = n'; 0 marks a pixel that so far holds only a neighbour's sample as a placeholder.
 *   8 blend     live, k == 0: out = hst; live, k > 0: out = hst + a_eff (cur - hst); not live: out = cur, the bits copied.  mask 1: live; 2:
 *               accepted with hc == 0 (a placeholder replaced); 0: rejected, counted in rejected_out.  d_out_rgba8 follows
 *               adanerf_resolve_mean's byte contract.
 * With the offsets of adanerf_host_subpixel_grid(s, .) every output pixel has inside true in exactly one frame of the s^2 cycle, with
 * ex = ey = 0 to rounding: at rest from a cut, after s^2 calls every count is 1 and the image is the interleave of the s^2 renders.
 * What it does not do: rejected pixels show the nearest sample (their mask selects them for adanerf_render_masked on a context of the
 * output size; neither host does it); no variance clipping;
 * the scene is static; at s = 1 it is a temporal resolve with another depth test, not a replacement for adanerf_temporal_resolve.
 * Two launches on the context's stream.  Context-owned scratch: zp ([h*w] fp32, grown on demand as adanerf_reproject's z-buffer is) and the
 * counter shared with adanerf_reproject; both freed by adanerf_destroy; adanerf_render never allocates for them.
 * ADANERF_EINVAL, with nothing written: everything adanerf_temporal_resolve refuses; scale outside 1..4; W H >= 2^25; cur_dx / cur_dy not
 * finite or beyond +-1; d_out_rgb overlapping d_hist_rgb or d_cur_rgb, d_out_depth overlapping d_hist_depth, d_cur_depth_map or
 * d_cur_acc_map, d_out_count overlapping d_hist_count.
 * ADANERF_EUNSUPPORTED, with nothing written: a useNDC model; a context with shard_world != 1. */
int adanerf_temporal_upsample(adanerf_ctx* ctx, int32_t scale, const float* d_cur_rgb, const float* d_cur_depth_map, const float* d_cur_acc_map,
                              float cur_dx, float cur_dy, const float cur_pos[3], const float cur_rot_c2w[9], const float* d_hist_rgb,
                              const float* d_hist_depth, const uint8_t* d_hist_count, const float prev_pos[3], const float prev_rot_c2w[9],
                              float alpha, float depth_tol, float acc_min, int32_t flags, float* d_out_rgb, float* d_out_depth,
                              uint8_t* d_out_count, void* d_out_rgba8, uint8_t* d_out_mask, int32_t* rejected_out);

/* The temporal resolve of a foveated frame: adanerf_temporal_resolve told which pixels were rendered and which only reconstructed.
 * Rendered pixels refresh the history; reconstructed pixels keep the history they have and show the fill only where they have none.  With
 * the lattice moving through adanerf_host_density_phase's 64 phases the periphery converges on the full render while the camera rests,
 * at the price of the foveated frame; in motion every pixel is re-rendered at least once per s^2 frames of its ring.
 *   d_mask, phase_x, phase_y   the mask and phase of this frame.  d_cur_* are what adanerf_render_masked(d_mask, 1, ..) followed by
 *                              adanerf_fill_density_phased(d_mask, .., phase_x, phase_y, ..) left: dense colour, depth and acc at the
 *                              context's current frame size.  Byte 0: the pixel was rendered; 2, 4 or 8: reconstructed with that stride;
 *                              any other byte: the pixel is rejected -- out = cur with the bits copied, count 0, mask 0, no history read.
 *   every other argument, image shape, alignment rule and the meaning of rejected_out are adanerf_temporal_resolve's, except that
 *   d_hist_count is required whenever d_hist_rgb is given and d_out_count always: without a count a placeholder (count 0, a fill nobody
 *   rendered) could not be told from a sample.
 * Two launches on the context's stream; a gather: the same inputs give the same bits on every call.  Every operation below is one
 * rounded fp32 operation in the stated order, never fused.
 * Pass A (only with d_hist_rgb and d_hist_depth), over every pixel i: zp[i], the camera depth of i's surface at the previous pose --
 *   pass A of adanerf_temporal_upsample with G_lo the context's generator at pixel centres (the offset of adanerf_set_pixel_offset is
 *   ignored, as adanerf_temporal_resolve ignores it): +inf for a far pixel or a value that is not finite.  The scratch is the context's
 *   own, shared with adanerf_temporal_upsample and grown on demand.
 * Pass B, per pixel j:
 *   1-3  adanerf_temporal_resolve's steps unchanged: the surface from j's own depth and acc, zc_cur -> d_out_depth[j], the projection into
 *        the previous camera, the nearest tap.  A pixel that misses the previous frame is rejected.
 *   4    disocclusion (only with d_hist_depth): hd = d_hist_depth[tap] against a set Z of zp values.  Rendered pixel: the zp of j's 3 x 3
 *        neighbourhood that exists.  Reconstructed pixel: the zp of its used corners, the corners adanerf_fill_density_phased used (none
 *        on a frame narrower than the stride: Z is empty).  zmin / zmax the smallest / largest finite value of Z, any_far: some value is
 *        +inf.  The rule is step 4 of adanerf_temporal_upsample verbatim: hd == +inf: accepted iff any_far; hd finite: accepted iff a finite
 *        zp exists and zmin - tol zmin <= hd <= zmax + tol zmax; anything else rejected.  Why the corners: a filled depth is a blend of its
 *        corners' depths, so a history surface that any corner explains is not a disocclusion, and the 3 x 3 of a blend would reject every
 *        cell that straddles an edge.  The corners' mask bytes are not looked at.
 *   5    history colour hst: adanerf_temporal_resolve's four bilinear taps.
 *   6    clamp (ADANERF_TEMPORAL_CLAMP), rendered pixels only: hst to the minimum / maximum of the current (filled) colour over the 3 x 3
 *        neighbourhood, by adanerf_temporal_resolve's order rules.  A reconstructed pixel's own colour is an interpolation and no
 *        evidence against its history: not clamped.
 *   7    hc = d_hist_count[tap]; live = accepted and hc >= 1.  Count n': rendered and live min(hc + 1, 255), with a_eff = fmaxf(alpha,
 *        1.0f / (float)n'); rendered and not live 1; reconstructed and live hc; reconstructed and not live 0, a placeholder.
 *   8    rendered and live: out = hst + a_eff (cur - hst); reconstructed and live: out = hst; not live: out = cur, the bits copied.
 *        d_out_mask: 1 live; 2 accepted with hc == 0 (a placeholder replaced by a sample, or kept as the new fill); 0 rejected, counted in
 *        rejected_out.  d_out_rgba8 follows adanerf_resolve_mean's byte contract.
 * Without a history every pixel is rejected: rendered pixels start at count 1, reconstructed ones at 0.
 * Measured (profiles/foveated_temporal_measured.md): the call 58 us at 800 x 800 and 128 us at 1920 x 1080 with the history's depth tested
 * (adanerf_temporal_resolve on the same images: 52 us and 112 us), 33 us and 57 us without; the whole frame -- phased mask, masked render,
 * phased fill, this call -- 1.20 ms and 3.15 ms at rest where the fill-only frame takes 1.13 ms and 3.05 ms.  At rest the result reaches the
 * full render (above 90 dB) once every pixel has been rendered; on a moving camera it can score below the fill-only frame (same note).
 * ADANERF_EINVAL, with nothing written: everything adanerf_temporal_resolve refuses; a NULL mask; a phase outside 0..7; a history without
 * a count; a NULL d_out_count; the mask overlapping an output.  ADANERF_EUNSUPPORTED, with nothing written: useNDC models; shards.
 * What it does not do: sub-pixel jitter on top (the stage ignores the offset as its siblings do; a host may still set one); budget maps;
 * variance clipping; ageing out reconstructed history faster than alpha; re-rendering the rejected pixels (d_out_mask == 0 selects them
 * for adanerf_render_masked, but neither host does it); launches sized on the device; NDC models and shards. */
int adanerf_temporal_resolve_sparse(adanerf_ctx* ctx, const uint8_t* d_mask, int32_t phase_x, int32_t phase_y, const float* d_cur_rgb,
                                    const float* d_cur_depth_map, const float* d_cur_acc_map, const float cur_pos[3],
                                    const float cur_rot_c2w[9], const float* d_hist_rgb, const float* d_hist_depth,
                                    const uint8_t* d_hist_count, const float prev_pos[3], const float prev_rot_c2w[9], float alpha,
                                    float depth_tol, float acc_min, int32_t flags, float* d_out_rgb, float* d_out_depth,
                                    uint8_t* d_out_count, void* d_out_rgba8, uint8_t* d_out_mask, int32_t* rejected_out);

/* ---- measurement hook (bench.py's roofline) ---- */

/* What dense 16-bit MFMA rate does the context's device sustain on live operands, and at which clock?  Runs register-only loops of
 * v_mfma_f32_32x32x16_bf16 (f16 != 0: _f16) on every CU for about target_ms milliseconds -- two accumulator chains per wave, one wave
 * per SIMD, the shading kernel's form -- and returns the achieved TFLOP/s and the effective shader clock (MHz, s_memtime against
 * s_memrealtime).  operands: 0 all-zero bits, 1 constant small values, 2 random values that change with every MFMA, 3 as 2 with a
 * post-ReLU-like B operand (half of its elements 0, the rest positive).  The part runs to a power budget: the same stream reaches
 * ~2.4 GHz on zeros and ~1.7 GHz on random operands, so a kernel's fraction of the nominal 2.5 PFLOP/s and its fraction of what
 * the silicon sustains on its kind of data differ (profiles/r04_mfma_peak_operands_clock.log).  Synchronous; nothing else should
 * run on the device meanwhile. */
int adanerf_probe_mfma(adanerf_ctx* ctx, int32_t operands, int32_t f16, float target_ms, float* tflops, float* clock_mhz);

/* ---- device memory plumbing for callers without a HIP runtime of their own ---- */
int adanerf_malloc(adanerf_ctx* ctx, size_t bytes, void** d_out);
int adanerf_free(adanerf_ctx* ctx, void* d_ptr);
int adanerf_memcpy_h2d(adanerf_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int adanerf_memcpy_d2h(adanerf_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* Internal buffers of the last adanerf_render batch (device pointers, valid until the next call). */
enum {
  ADANERF_BUF_RAYS = 0,        /* [batch,8] fp32 */
  ADANERF_BUF_ORACLE = 1,      /* [batch,128] fp32 */
  ADANERF_BUF_RAY_OFFSETS = 2, /* [batch] int32 */
  ADANERF_BUF_RAY_COUNTS = 3,  /* [batch] int32; 0..N under adanerf_set_depth_limit */
  ADANERF_BUF_SAMPLE_KEY = 4,  /* [S] uint32; not written in dense mode (threshold 0): sample i is ray i >> 7, bin i & 127 */
  ADANERF_BUF_SAMPLE_W = 5,    /* [S] fp32; not written in dense mode: the kept values are ADANERF_BUF_ORACLE itself */
  ADANERF_BUF_RAW = 6,         /* [S,4] fp32 */
  ADANERF_BUF_TOTAL = 7,       /* [1] int32 */
  ADANERF_BUF_SAMPLE_Z = 8,    /* [S] fp32 (ADANERF_SAMPLER_PDF / _COARSE_FINE) */
  ADANERF_BUF_RAW_COARSE = 9,  /* [batch*Nc,4] fp32 (ADANERF_SAMPLER_COARSE_FINE) */
  ADANERF_BUF_RAY_LIST = 10,   /* [M] int32: the ascending ray ids of the last adanerf_render_masked (NULL before the first) */
  ADANERF_BUF_RAY_LIST_COUNT = 11 /* [1] int32: M of that call */
};
int adanerf_get_buffer(adanerf_ctx* ctx, int32_t which, void** d_out, size_t* bytes_out);

/* ---- host-only inspection (no device needed; used by the CPU test-suite) ---- */

/* Parses and validates config.ini / dataset_info.txt exactly as adanerf_create does and fills
 * `info` (compute_units = 0).  Fails with the same codes/messages as adanerf_create. */
int adanerf_host_parse_model(const char* model_dir, const adanerf_options* opt, adanerf_info* info);

/* Packs net 0 (sampling) or net 1 (shading) of model_dir into MFMA A-fragment order for
 * `precision` (ADANERF_PREC_*, or 3 = the sampling net's fp16 hi/lo' split pairs).  Two-call pattern: pass NULL outputs to query sizes.
 *   weights_out  packed 16-byte fragments        (*weights_bytes)
 *   bias_out     packed bias blocks, fp32        (*bias_floats)
 *   layer_out    per layer {w_off (16-B units), b_off (floats), slots per lane-half, 32-row tiles}
 *                as int32[4] each                (*n_layers); a sampling net with raySampleInput = A > 0 has one more
 *                record {w_off of layer 0's K-major block for the A extra points, A, slots per point, tiles}; a shading net in
 *                ADANERF_PREC_BF16 has one more record {alpha exponent, rgb exponent, 0, -1}: it is packed SCALED (every ReLU
 *                layer's weights and bias carry a power of two that keeps its activations <= 1, so the kernels' ReLU is a clamped
 *                conversion), and its alpha / rgb outputs x 2^exponent are the network's own.
 *                (precision 4, net 1 only: the bf16 blob without that scaling, for tests -- no kernel consumes it.)
 * The shading net packs in every precision for every topology.  A sampling net other than 8 x 256 with a 10-4 / 2-2 encoding
 * packs for ADANERF_PREC_FP32 (run-time-shaped fp32 kernel) and, without raySampleInput, as split pairs (3: run-time-shaped
 * split-precision kernel); the plain 16-bit precisions -- and the split pairs with raySampleInput -- return ADANERF_EIO with a message.
 * Hidden widths up to 512 pack (zero-padded); a net wider than 256 packs for ADANERF_PREC_FP32 in the wide form (16-row tiles: records
 * hold slots per lane group and 16-row tiles), a sampling net that wide for ADANERF_PREC_FP32 only, without raySampleInput. */
int adanerf_host_pack_weights(const char* model_dir, int32_t net, int32_t precision, void* weights_out,
                              size_t* weights_bytes, float* bias_out, size_t* bias_floats, int32_t* layer_out,
                              int32_t* n_layers);

/* 128-entry world-depth table the shading stage indexes by bin (and dense t-values) for model_dir. */
int adanerf_host_depth_table(const char* model_dir, const adanerf_options* opt, float* ztab128);


/* The regular s x s sub-pixel pattern both hosts and the evaluator feed to adanerf_set_pixel_offset: for k in 0..s*s-1, i = k % s,
 * j = k / s, *dx = (2 i + 1 - s) / (2 s), *dy alike from j, computed in double and cast to float.  s in 1..8, k in 0..s*s-1, non-NULL
 * outputs; anything else returns ADANERF_EINVAL.  s == 1 gives (0, 0); the offsets of a grid sum to 0 on either axis. */
int adanerf_host_subpixel_grid(int32_t s, int32_t k, float* dx, float* dy);

/* An occluder without a rasteriser, for both hosts and the tests: the camera-space depth (the zc of adanerf_set_depth_limit) of a sphere
 * for every pixel of a width x height frame with pixel pitch 1 and focal length `focal` (adanerf_info.focal), seen from pos / rot_c2w
 * (conventions of adanerf_set_camera).  zc_out [height*width] fp32, row-major; a pixel whose ray misses the sphere gets +inf.
 * Everything in float64, each step one rounded operation in this order, never fused; the cast to float comes last:
 *   e_i = center_i - pos_i;  c_k = (R[k] e_0 + R[3+k] e_1) + R[6+k] e_2 (the centre in camera space, R^T e);
 *   g = ((c_0 c_0 + c_1 c_1) + c_2 c_2) - radius radius
 *   pixel (x, y): vx = ((x + 0.5) - 0.5 width) / focal, vy = -(((y + 0.5) - 0.5 height) / focal), vz = -1 -- the inverse of adanerf_reproject's
 *   projection; a = (vx vx + vy vy) + 1;  b = (vx c_0 + vy c_1) - c_2;  disc = b b - a g
 *   disc >= 0: s = sqrt(disc), t0 = (b - s) / a, t1 = (b + s) / a; zc = t0 if t0 > 0, else t1 if t1 > 0 -- the smallest root t > 0 of
 *   |t v - c|^2 = radius^2, which is zc because vz = -1.  Otherwise (and with !(disc >= 0)) +inf.
 * ADANERF_EINVAL: a NULL pointer; a side outside 1..16384; a value that is not finite; radius <= 0; focal <= 0. */
int adanerf_host_sphere_zc(int32_t width, int32_t height, float focal, const float pos[3], const float rot_c2w[9], const float center[3],
                           float radius, float* zc_out);

/* The mask of adanerf_foveate_density computed on the host, for a width x height frame: the same rule compiled from the same text, byte
 * for byte what the device writes.  mask_out [height*width] uint8, row-major.
 * ADANERF_EINVAL, with nothing written: everything adanerf_foveate_density refuses; a side outside 1..16384. */
int adanerf_host_density_mask(int32_t width, int32_t height, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px,
                              const int32_t* stride, uint8_t* mask_out);

/* The mask of adanerf_foveate_density_phased computed on the host, compiled from the same text (csrc/density_rule.hpp).
 * ADANERF_EINVAL, with nothing written: everything adanerf_host_density_mask refuses; a phase outside 0..7. */
int adanerf_host_density_mask_phased(int32_t width, int32_t height, float gaze_x, float gaze_y, int32_t n_rings, const int32_t* radius_px,
                                     const int32_t* stride, int32_t phase_x, int32_t phase_y, uint8_t* mask_out);

/* The phase of frame k, a cycle of 64: k is taken mod 64 (a negative k too); d_i = (k >> 2 i) & 3 for i = 0, 1, 2; with bx = {0, 1, 1, 0}
 * and by = {0, 1, 0, 1}, phase_x = sum bx[d_i] << i and phase_y = sum by[d_i] << i.  k mod L^2 fixes (phase_x mod L, phase_y mod L) one to
 * one, so any L^2 consecutive frames put every residue pair mod L on the lattice exactly once, for L = 2, 4 and 8 at the same time.
 * ADANERF_EINVAL, with nothing written: a NULL output. */
int adanerf_host_density_phase(int32_t k, int32_t* phase_x, int32_t* phase_y);

/* The mask of adanerf_contrast_mask computed on the host: the same rule compiled from the same text (csrc/contrast_rule.hpp), byte for
 * byte what the device writes.  rgb [height*width,3] fp32 and mask [height*width] uint8 in host memory; n_flagged may be NULL.
 * ADANERF_EINVAL, with nothing written: everything adanerf_contrast_mask refuses. */
int adanerf_host_contrast_mask(const float* rgb, int32_t width, int32_t height, float threshold, uint8_t* mask, int32_t* n_flagged);

/* The weight_b of adanerf_reproject_pair both hosts use, so that they blend alike: the destination's distance from A over the sum of its
 * distances from A and from B.  In float64 from the fp32 positions, each step one rounded operation: e_i = dst_i - a_i,
 * dA = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2), dB alike from b; *weight_b = (float)(dA / (dA + dB)), and 0.5 when dA + dB == 0 (a pure
 * rotation weighs both frames alike).  dst == a gives 0, dst == b gives 1.
 * ADANERF_EINVAL, with nothing written: a NULL pointer; a position entry that is not finite. */
int adanerf_host_pair_weight(const float dst_pos[3], const float a_pos[3], const float b_pos[3], float* weight_b);

#ifdef __cplusplus
}
#endif
#endif /* ADANERF_HIP_H */
