// Built by tests/test_set_frame_size_cpu.py from the host's own sources (everything but main.cpp).  No device: the renderer is never
// initialised.  Two modes:
//   <line> ...            feeds each argument to InputHandler::replay as one script line and prints "ok" or "bad", the frame size the
//                         renderer would ask of the library before its next frame, the selection it would ask for and whether the line
//                         toggled the sampling-network view
//   --settings <argv> ... runs Settings::init over the rest of the command line and prints what it stored
#include <cstdio>
#include <cstring>
#include <string>

#include "../adanerf_amd/host/camera.h"
#include "../adanerf_amd/host/inputhandler.h"
#include "../adanerf_amd/host/neuralrenderer.h"
#include "../adanerf_amd/host/settings.h"

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--settings") == 0) {
    Settings s;
    std::string err;
    argv[1] = argv[0];
    const bool ok = s.init(argc - 1, argv + 1, &err);
    std::printf("%s size=%ux%u window=%ux%u write=%d write_window=%d batch=%u request=%d\n", ok ? "ok" : "bad", s.width, s.height, s.window_width,
                s.window_height, s.write_images ? 1 : 0, s.write_window ? 1 : 0, s.batch_size, s.batch_request);
    return 0;
  }
  for (int i = 1; i < argc; ++i) {
    Settings settings;
    Camera camera;
    NeuralRenderer renderer(settings, camera);
    InputHandler input(renderer, camera);
    const bool ok = input.replay(argv[i]);
    int w = 0, h = 0, n = 0;
    float thr = 0.f;
    const bool size_pending = renderer.pendingFrameSize(&w, &h);
    const bool sel_pending = renderer.pendingSelection(&n, &thr);
    std::printf("%s size_pending=%d w=%d h=%d sel_pending=%d n=%d oracle=%d\n", ok ? "ok" : "bad", size_pending ? 1 : 0, w, h, sel_pending ? 1 : 0, n,
                renderer.renderingOracle() ? 1 : 0);
  }
  return 0;
}
