// Headless NeuralRenderer: the viewer's init()/render() pair (include/neuralrenderer.h:53-55) over the
// C ABI of libadanerf_hip.so.  Owns the device framebuffer the viewer's BufferManager would own.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/adanerf_hip.h"
#include "camera.h"
#include "settings.h"

// The resolved frames a temporal stage blends with (--taa, --taau, --fovea-temporal; one of them at a time): two sets (rgb float [n*3],
// depth float [n], count uint8 [n]) that ping-pong, which one was written last and at which pose.
struct History {
  void* set[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  bool have = false;                 // set[side], pos and rot describe a resolved frame of the size in force
  int side = 0;
  float pos[3] = {0, 0, 0}, rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  struct Inputs {
    const float *rgb, *depth;        // the history, or null without one; depth null at rest too
    const uint8_t* count;
    const float *prev_pos, *prev_rot;
    float *out_rgb, *out_depth;      // the set the resolve writes
    uint8_t* out_count;
  };
  int out() const { return have ? 1 - side : 0; }
  // what a resolve at (pos, rot) reads and writes.  The camera has not moved since the history was written: nothing can have been
  // uncovered, so no disocclusion test (as renderer.py)
  Inputs inputs(const float at_pos[3], const float at_rot[9]) const {
    const bool at_rest = have && std::memcmp(pos, at_pos, sizeof(pos)) == 0 && std::memcmp(rot, at_rot, sizeof(rot)) == 0;
    void* const* h = set[side];
    void* const* o = set[out()];
    return {have ? static_cast<const float*>(h[0]) : nullptr, have && !at_rest ? static_cast<const float*>(h[1]) : nullptr,
            have ? static_cast<const uint8_t*>(h[2]) : nullptr, pos, rot, static_cast<float*>(o[0]), static_cast<float*>(o[1]), static_cast<uint8_t*>(o[2])};
  }
  void commit(const float at_pos[3], const float at_rot[9]) {      // after a successful resolve at (pos, rot)
    side = out();
    have = true;
    std::memcpy(pos, at_pos, sizeof(pos));
    std::memcpy(rot, at_rot, sizeof(rot));
  }
  void reset() { have = false; }     // the next frame is a first frame
};

class NeuralRenderer {
 public:
  NeuralRenderer(Settings& settings, Camera& camera) : settings(settings), camera(camera) {}
  ~NeuralRenderer();

  bool init();
  bool initHostOnly();               // --dry-run: parse the model directory on the host only (no device), for input replay
  bool render();                     // one frame; logs every 100 frames like imagegenerator.cpp:379-393
  void switchRenderOracle() { render_oracle = !render_oracle; }   // neuralrenderer.h: the 'O' key toggle
  bool renderingOracle() const { return render_oracle; }
  // sample budget N / selection threshold from the next frame on (n <= 0, thr < 0: keep); reaches every context in render()
  void setSelection(int n, float thr) {
    if (n > 0) want_samples = n;
    if (thr >= 0.f) want_threshold = thr;
    selection_pending = true;
  }
  bool pendingSelection(int* n, float* thr) const {      // what the next frame will ask of the library (0 / < 0: keep)
    *n = want_samples;
    *thr = want_threshold;
    return selection_pending;
  }
  // --sample-cap: the bound from the next frame on (script token "cap X", 0 removes it); reaches every context in render()
  void setSampleCap(float cap) {
    want_cap = cap;
    cap_pending = true;
  }
  bool pendingSampleCap(float* cap) const {      // what the next frame will ask of the library
    *cap = want_cap;
    return cap_pending;
  }
  // frame size from the next frame on ("size W H"); the window size stays.  Reaches every context in render()
  void setFrameSize(int w, int h) {
    want_width = w;
    want_height = h;
    size_pending = true;
  }
  bool pendingFrameSize(int* w, int* h) const {      // what the next frame will ask of the library
    *w = want_width;
    *h = want_height;
    return size_pending;
  }
  // --fovea / --fovea-density: the gaze point from the next frame on (script token "gaze X Y", pixels); the maps / the mask are filled again in render()
  void setGaze(float x, float y) {
    gaze_x = x;
    gaze_y = y;
    gaze_set = true;
    fovea_pending = true;
  }
  bool pendingGaze(float* x, float* y) const {      // what the next frame will ask of the library
    *x = gaze_x;
    *y = gaze_y;
    return fovea_pending;
  }
  // --taa / --taau: the next frame is shown as rendered and starts a new history (script token "cut"); without them nothing to drop
  void cutHistory() {      // --interpolate: both keyframes go too, the next frame is the first of a new sequence
    history.reset();
    ip_keys = 0;
  }
  bool applyFrameSize();             // a pending setFrameSize, now: render() calls it; --dry-run calls it in render()'s place (host only)
  int batchesPerFrame() const;       // ceil(rays / batch_rays)
  bool writeImageToFile();           // out.bmp in the model directory (neuralrenderer.cpp:184-222); --write-window: out_window.bmp too
  const adanerf_info& info() const { return info_; }
  const std::string& error() const { return err; }

 private:
  Settings& settings;
  Camera& camera;
  adanerf_ctx* ctx = nullptr;        // rank 0: display GPU, owns the frame
  std::vector<adanerf_ctx*> peers;   // ranks 1 .. N-1 (--gpus N), one per GPU, same process
  std::vector<adanerf_ctx*> contexts() const {      // rank 0, then the peers
    std::vector<adanerf_ctx*> all(1, ctx);
    all.insert(all.end(), peers.begin(), peers.end());
    return all;
  }
  template <class Set>
  bool applyToAll(Set set);          // set(context) on every context, then the source frame and the history are dropped: the change shows from this frame on
  std::vector<void*> d_payload;      // per rank: uchar4 [rays_local_max] on that rank's GPU
  void* d_gathered = nullptr;        // rank 0: uchar4 [N][rays_local_max]
  adanerf_info info_{};
  void* d_frame = nullptr;           // uchar4 [h*w]
  // --reproject K > 1: depth_map / acc_map of the last rendered frame (the context's aux outputs), its pose, the warped frame
  void* d_depth = nullptr;
  void* d_acc = nullptr;
  void* d_warp = nullptr;            // uchar4 [h*w]
  void* d_wmask = nullptr;           // --rerender: adanerf_reproject's mask of the warped frame, uint8 [h*w]
  void* d_src_rgb = nullptr;         // --reproject-warp gather: the rendered frame's fp32 colour, float [h*w*3]
  void* d_warp_rgb = nullptr;        // --reproject-warp gather: the gathered fp32 colour, float [h*w*3]
  const void* d_shown = nullptr;     // what the last frame presented: d_frame or d_warp (-w / --write-window write it)
  bool have_source = false;          // d_frame, d_depth, d_acc and src_* describe one rendered frame of the size and selection in force
  int since_render = 0;              // warped frames since it
  float src_pos[3] = {0, 0, 0}, src_rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  bool warp(const float rot[9]);     // this frame = the source frame at the camera of the moment
  // --interpolate K: two keyframes (uchar4 frame, fp32 colour, depth_map, acc_map, pose) that ping-pong, the ring of the last K cameras and
  // the interpolated frame (d_warp, d_warp_rgb, d_wmask)
  struct Keyframe {
    void* rgba = nullptr;
    void* rgb = nullptr;
    void* depth = nullptr;
    void* acc = nullptr;
    float pos[3], rot[9];
  };
  struct Pose {
    float pos[3], rot[9];
  };
  Keyframe ip_key[2];
  int ip_keys = 0;                   // keyframes held (0, 1 or 2) of the size and selection in force; dropped with the --reproject source
  int ip_newer = 0;                  // which of ip_key is B, the keyframe rendered last
  int ip_call = 0;                   // frames since the first keyframe of this sequence
  std::vector<Pose> ip_ring;         // the cameras of the last K frames: slot ip_call % K
  bool renderKeyframe(int into, adanerf_stats* st, const float rot[9]);
  bool interpolate(const float rot[9]);      // this frame of --interpolate K: a keyframe, or the frame between two at the camera of K frames ago
  void logInterval();                // the per-100-frame line of the single-context path
  long long s_rerendered = 0;        // --rerender: pixels rendered into the warped frames of the running interval
  long long s_holes = 0;             // holes of the warped frames / rendered and warped frames of the running interval
  int s_rendered = 0, s_warped = 0;
  // --supersample S > 1: the fp32 frame of one sub-pixel render and the running sum of a shown frame's S x S renders, float [h*w*3] each
  void* d_rgb = nullptr;
  void* d_sum = nullptr;
  bool renderSupersampled(adanerf_stats* st);   // S x S renders at the grid's offsets, accumulated and resolved into d_frame; *st: times summed, samples per render
  // --supersample-contrast T: d_rgb holds the centre frame's fp32 colour, d_stage (float [h*w*3]) one masked sub-pixel render, d_cmask (uint8
  // [h*w]) the contrast mask of the centre frame (0 = refined)
  void* d_stage = nullptr;
  void* d_cmask = nullptr;
  long long s_refined = 0;           // pixels refined in the running interval's frames
  bool renderSupersampledAdaptive(adanerf_stats* st);   // the centre frame into d_frame / d_rgb, then the S x S masked renders of its flagged pixels over it
  // --taa: depth_map / acc_map (d_depth, d_acc) and the fp32 frame (d_rgb) of this frame's render; the history, the place in the offset cycle
  History history;
  int taa_k = 0;
  long long s_rejected = 0;          // rejected pixels of the running interval's frames
  template <class Render>
  bool renderAtOffset(float dx, float dy, Render render);   // render() with the rays through (dx, dy) of their pixels; the offset goes back to (0, 0) whatever happened
  bool renderJittered(int S, adanerf_stats* st, float* dx, float* dy);   // one render into d_rgb at the next offset of the S x S cycle
  bool renderTemporal(adanerf_stats* st, const float rot[9]);   // one render at the cycle's next offset, resolved against the history into d_frame
  // --taau S: as --taa, with the two history sets and the shown frame d_up (uchar4) at S w x S h; the state above (history, taa_k,
  // s_rejected) is shared, the two being exclusive
  void* d_up = nullptr;
  bool renderUpsampled(adanerf_stats* st, const float rot[9]);   // one render at the cycle's next offset, resolved into the S w x S h history and d_up
  // --occluder: the limit (float [h*w]) and the colour behind it (float [h*w*3]) of the spheres at the pose and size they were last filled
  // for; the fp32 frame (d_rgb) and acc_map (d_acc) of this frame's render
  void* d_limit = nullptr;
  void* d_behind = nullptr;
  bool occ_have = false;             // d_limit / d_behind hold the spheres as seen from occ_pos / occ_rot at the size in force
  float occ_pos[3] = {0, 0, 0}, occ_rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  bool renderHybrid(adanerf_stats* st, const float rot[9]);   // the map refilled if the camera or the size moved, one render under it, blended into d_frame
  // --fovea-density: the mask of the gaze and the size in force (uint8 [h*w]; 0 = rendered, else the pixel's stride); the fp32 frame (d_rgb)
  // the lattice is rendered into and the pixels in between are rebuilt in, together with d_frame
  void* d_dmask = nullptr;
  long long s_density_rendered = 0;  // rays rendered in the running interval's frames
  bool applyFoveaDensity();          // the mask filled again: at start, after "gaze", after "size" (fovea_pending, shared with --fovea: the two are exclusive)
  bool renderFoveated(adanerf_stats* st);   // adanerf_render_masked over the lattice, adanerf_fill_density for the rest, into d_frame
  // --fovea-temporal: the frame number of the phase cycle; the aux maps (d_depth, d_acc), the history and the count are --taa's
  // (history, s_rejected: --fovea-density excludes --taa and --taau)
  int ft_k = 0;
  bool renderFoveatedTemporal(adanerf_stats* st, const float rot[9]);   // phased mask, masked render, phased fill, sparse resolve into d_frame
  void* d_window = nullptr;          // --write-window: uchar4 [window_height*window_width], the frame as adanerf_present shows it
  int world_ = 1, strip_rows_ = 8;   // share layout chosen at init; a live context keeps its strip height
  // a frame-sized device buffer of rank 0: its member, the bytes it needs under the settings and the size in force (0: not needed), and the
  // state that describes its contents and so resets when it is made again
  enum Resets { RESET_SOURCE = 1, RESET_HISTORY = 2, RESET_OCCLUDER = 4, RESET_FOVEA = 8 };
  struct FrameBuffer {
    void** p;
    size_t bytes;
    int resets;
  };
  std::vector<FrameBuffer> frameBuffers();
  bool allocFrameBuffers();          // every buffer of frameBuffers(), d_gathered and d_payload for the size in info_ (again after a size change)
  bool writeBmp(const std::string& name, const void* d_image, int w, int h);
  std::string err;
  bool render_oracle = false;
  bool selection_pending = false;    // setSelection since the last frame
  int want_samples = 0;
  float want_threshold = -1.f;
  bool applyFovea();                 // --fovea: maps of every context filled for the gaze and the size in force, and installed
  std::vector<void*> d_fovea_n, d_fovea_thr;   // per context (rank order): uint8 / float [rays_local] on that context's GPU
  bool fovea_pending = true;         // the maps are to be filled before the next frame: at start, after "gaze", after "size"
  bool gaze_set = false;             // a "gaze" token has moved it from the frame centre
  float gaze_x = 0.f, gaze_y = 0.f;
  bool cap_pending = false;          // setSampleCap since the last frame (init: --sample-cap)
  float want_cap = 0.f, cap_in_force = 0.f;
  float s_cap_thr = -1.f / 0.f;      // --sample-cap: largest threshold the cap chose, samples before / after it, over the running interval's frames
  long long s_cap_selected = 0, s_cap_kept = 0;
  bool size_pending = false;         // setFrameSize since the last frame
  int want_width = 0, want_height = 0;
  // 100-frame running sums
  int logging_interval = 100, sample_count = 0;
  double s_inference1 = 0, s_inference2 = 0, s_fc2 = 0, s_rm = 0, s_total = 0;
  int guard_widened_seen = 0;        // adanerf_stats.guard_widened already reported on the console
  long long s_num_total_samples = 0;
};
