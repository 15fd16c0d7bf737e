// Command-line settings of the headless `adanerf` host.  Same arguments and batch-size semantics as the
// reference viewer (adanerf_real_time_viewer/src/main.cpp:19-50, src/settings.cpp:15-47).
#pragma once
#include <string>
#include <vector>

class Settings {
 public:
  std::string model_path = "sample/";
  unsigned int width = 800, height = 800, total_size = 640000;
  unsigned int window_width = 800, window_height = 800;   // -ws: the size --write-window presents the frame at (default: the frame size)
  unsigned int batch_size = 640000;
  int batch_request = 0;        // what adanerf_options.batch_rays gets: -bs as given (not clamped to the first frame size, so that a
                                // "size" token re-derives the batch from it), -nb's share of the first frame, 0: the whole frame
  bool write_images = false;
  bool write_window = false;    // --write-window: also write the frame presented at the window size (out_window.bmp beside out.bmp)
  bool is_debug = false;        // -d: accepted, headless is always "debug" (no GL interop)
  // headless extras (not in the reference)
  int frames = 100;             // --frames: frames to render before exiting
  std::string precision = "bf16";
  std::string sampling;               // --sampling auto|guarded|split|fp32|fp16: arithmetic of the sampling network (ADANERF_SAMPLING_*; auto = the default rule measured on this workload at start-up); the
                                      // viewer itself has one (TensorRT kFP16 = "fp16"); "guarded" keeps the exact engine's selections while its
                                      // measured band holds.  Not given: split (exact by construction on every ray; DESIGN 1 has the rule)
  float yaw = -80.f, pitch = 0.f;   // Camera::init defaults (camera.cpp:90-91)
  int num_samples = 0;
  float threshold = -1.f;
  int gpus = 1;                 // --gpus N: one context per GPU in this process, strips exchanged with peer copies over xGMI
  bool same_device = false;     // --same-device: all N contexts on device 0 (exercises the N-GPU path on a 1-GPU box)
  int sub_shares = 0;           // --sub-shares P: every GPU renders its share of a frame as P concurrent sub-shares (contexts / streams);
                                // 0: 2 with --gpus N > 1 when the rows split evenly over 2 N, else 1
  std::string script;           // --script FILE: replay input events, one line per frame (inputhandler.h)
  bool log_camera = false;      // --log-camera: print position / yaw / pitch / view per frame
  bool dry_run = false;         // --dry-run: replay the script without a device (no rendering)
  // --fovea R:N:T[,R:N:T...],N:T: per-ray sample budgets around a gaze point (adanerf_foveate): up to 8 rings, radius in whole pixels
  // strictly ascending, each with the N (0..255, 0 = the context's) and threshold of the pixels inside it; the last entry is for the pixels
  // outside every ring.  The gaze starts at the frame centre (script token `gaze X Y` moves it).  Empty fovea_n: no foveation
  std::vector<int> fovea_radius, fovea_n;
  std::vector<float> fovea_thr;
  static bool parseFovea(const std::string& spec, std::vector<int>* radius, std::vector<int>* n, std::vector<float>* thr, std::string* err);
  // --fovea-density R:S[,R:S...],S: foveated ray density around the same gaze point (adanerf_foveate_density / adanerf_render_masked /
  // adanerf_fill_density): up to 8 rings, radius in whole pixels strictly ascending, each with the stride S (1, 2, 4 or 8: every S-th pixel per
  // axis is rendered, the rest rebuilt from them) of the pixels inside it, never decreasing outward; the last entry is the stride outside every
  // ring.  Empty density_stride: off
  std::vector<int> density_radius, density_stride;
  static bool parseFoveaDensity(const std::string& spec, std::vector<int>* radius, std::vector<int>* stride, std::string* err);
  // --fovea-temporal ALPHA (with --fovea-density): the lattice moves through the 64 phases of adanerf_host_density_phase and every frame is
  // resolved against a history that knows which pixels were rendered (adanerf_temporal_resolve_sparse, clamp on, depth tolerance 0.02);
  // ALPHA in (0, 1] the weight of a rendered pixel once its history is older than 1 / ALPHA samples.  0: off
  float fovea_temporal_alpha = 0.f;
  // --occluder cx,cy,cz,r[,R,G,B] (repeatable): hybrid rendering against sphere occluders -- the frame is rendered under the depth limit of
  // the spheres' camera-space depth (per-pixel minimum, adanerf_host_sphere_zc / adanerf_set_depth_limit) and the nearest sphere's flat colour
  // (0..1 per channel, default 0.5 grey) is let through with the transmittance left (adanerf_blend_behind).  Empty: off
  struct Occluder {
    float center[3], radius, rgb[3];
  };
  std::vector<Occluder> occluders;
  static bool parseOccluder(const std::string& spec, Occluder* out, std::string* err);
  std::string rerender;         // --rerender holes|unsourced (with --reproject K > 1): the warped frames' holes (or every pixel without a source pixel
                                // of its own) are rendered at the frame's camera (adanerf_render_masked); empty: they stay filled from neighbours
  int reproject = 1;            // --reproject K: of every K frames the first is rendered, the next K - 1 are that frame warped to their own camera
                                // (adanerf_reproject, fill on); 1: every frame is rendered
  int interpolate = 0;          // --interpolate K (K >= 2): frames are shown K calls late; of every K the first is rendered as a keyframe, the K - 1 before
                                // it come from the keyframe behind and the keyframe ahead (adanerf_reproject_pair, fill on); 0: off
  bool reproject_warp_set = false;      // --reproject-warp / --reproject-iterations / --reproject-tol was given (an error without --reproject K > 1)
  bool reproject_gather = false;        // --reproject-warp gather: the warped frames come from adanerf_reproject_gather; splat (the default): adanerf_reproject
  int reproject_iterations = 4;         // --reproject-iterations N (1..8) and --reproject-tol T (>= 0): the gather's two dials
  float reproject_tol = 0.05f;
  int supersample = 1;          // --supersample S (1..8): every shown frame is S x S renders at the offsets of adanerf_host_subpixel_grid, accumulated and
                                // resolved on the device (adanerf_set_pixel_offset / adanerf_accumulate / adanerf_resolve_mean); 1: one render per frame
  float sample_cap = 0.f;       // --sample-cap X: no frame shades more than X samples per ray on average (adanerf_set_sample_cap; script token `cap X`); 0: off
  float supersample_contrast = -1.f;   // --supersample-contrast T (0..1, with --supersample S >= 2): adaptive supersampling -- one render at the pixel centres, then
                                // the S x S renders only for the pixels a neighbour of which differs by more than T in some channel's display value
                                // (adanerf_contrast_mask / adanerf_render_masked / adanerf_accumulate_masked / adanerf_resolve_mean_masked); < 0: off
  float taa_alpha = 0.f;        // --taa ALPHA[:TOL]: temporal anti-aliasing (adanerf_temporal_resolve, clamp on): every frame is rendered at the next offset of
  float taa_tol = 0.02f;        // the --taa-grid cycle and blended with a history carried to its camera; ALPHA in (0, 1] the weight of the new frame, TOL >= 0
  int taa_grid = 2;             // the relative depth tolerance of the disocclusion test; --taa-grid S (1..8): the S x S cycle of adanerf_host_subpixel_grid.  0: off
  int taau_scale = 0;           // --taau S[:ALPHA[:TOL]]: temporal upsampling (adanerf_temporal_upsample, clamp on): -s W H stays the render size, every frame is
  float taau_alpha = 0.1f;      // rendered at the next offset of the S x S cycle and resolved into a history of S W x S H, which -w / --write-window write;
  float taau_tol = 0.02f;       // S in 1..4, ALPHA in (0, 1] (default 0.1), TOL >= 0 the relative tolerance of the neighbourhood depth test (default 0.02).  0: off
  std::string present_filter;   // --present-filter nearest|linear|area: filter of the -ws window image (adanerf_present); empty: the viewer's rule
  bool render_oracle = false;   // --oracle: the viewer's 'O' key (inputhandler.cpp:76), sampling-network debug view

  // returns false and fills err on a malformed command line
  bool init(int argc, char** argv, std::string* err);
  static const char* usage();
};
