// Built by tests/test_budget_cpu.py from the host's own sources (everything but main.cpp).  No device: the renderer is never initialised.
// Two modes:
//   <line> ...        feeds each argument to InputHandler::replay as one script line and prints "ok" or "bad", the gaze the renderer would
//                     fill its budget maps for before its next frame, and the frame size / selection the same line asked for
//   --fovea <spec>    runs Settings::init over `adanerf model --fovea <spec>` and prints the rings it stored, or the error
#include <cstdio>
#include <cstring>
#include <string>

#include "../adanerf_amd/host/camera.h"
#include "../adanerf_amd/host/inputhandler.h"
#include "../adanerf_amd/host/neuralrenderer.h"
#include "../adanerf_amd/host/settings.h"

int main(int argc, char** argv) {
  if (argc > 2 && std::strcmp(argv[1], "--fovea") == 0) {
    for (int i = 2; i < argc; ++i) {
      Settings s;
      std::string err;
      char prog[] = "adanerf", model[] = "model", flag[] = "--fovea";
      char* av[4] = {prog, model, flag, argv[i]};
      const bool ok = s.init(4, av, &err);
      std::printf("%s rings=%zu", ok ? "ok" : "bad", s.fovea_radius.size());
      for (size_t k = 0; ok && k < s.fovea_n.size(); ++k) {
        if (k < s.fovea_radius.size()) std::printf(" %d:%d:%.9g", s.fovea_radius[k], s.fovea_n[k], static_cast<double>(s.fovea_thr[k]));
        else std::printf(" %d:%.9g", s.fovea_n[k], static_cast<double>(s.fovea_thr[k]));
      }
      std::printf("\n");
    }
    return 0;
  }
  for (int i = 1; i < argc; ++i) {
    Settings settings;
    Camera camera;
    NeuralRenderer renderer(settings, camera);
    InputHandler input(renderer, camera);
    float gx = -1.f, gy = -1.f, thr = 0.f;
    renderer.pendingGaze(&gx, &gy);
    const bool at_start = gx == 0.f && gy == 0.f;      // no token yet: the centre of the frame, taken when the maps are filled
    const bool ok = input.replay(argv[i]);
    int w = 0, h = 0, n = 0;
    renderer.pendingGaze(&gx, &gy);
    const bool size_pending = renderer.pendingFrameSize(&w, &h);
    const bool sel_pending = renderer.pendingSelection(&n, &thr);
    std::printf("%s start=%d gx=%.9g gy=%.9g size_pending=%d w=%d h=%d sel_pending=%d n=%d\n", ok ? "ok" : "bad", at_start ? 1 : 0,
                static_cast<double>(gx), static_cast<double>(gy), size_pending ? 1 : 0, w, h, sel_pending ? 1 : 0, n);
  }
  return 0;
}
