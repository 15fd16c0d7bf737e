// Built by tests/test_set_selection_cpu.py from the host's own sources (everything but main.cpp): feeds each argument to
// InputHandler::replay as one script line and prints what came of it -- "ok" or "bad", the selection the renderer would ask of the
// library before its next frame, and whether the line toggled the sampling-network view.  No device: the renderer is never initialised.
#include <cstdio>

#include "../adanerf_amd/host/camera.h"
#include "../adanerf_amd/host/inputhandler.h"
#include "../adanerf_amd/host/neuralrenderer.h"
#include "../adanerf_amd/host/settings.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    Settings settings;
    Camera camera;
    NeuralRenderer renderer(settings, camera);
    InputHandler input(renderer, camera);
    const bool ok = input.replay(argv[i]);
    int n = 0;
    float thr = 0.f;
    const bool pending = renderer.pendingSelection(&n, &thr);
    std::printf("%s pending=%d n=%d thr=%.9g oracle=%d\n", ok ? "ok" : "bad", pending ? 1 : 0, n, static_cast<double>(thr), renderer.renderingOracle() ? 1 : 0);
  }
  return 0;
}
