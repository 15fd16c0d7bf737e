#include "inputhandler.h"

#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "neuralrenderer.h"

static unsigned char movement_char(Key k) {
  switch (k) {
    case Key::W: return 'w';
    case Key::A: return 'a';
    case Key::S: return 's';
    case Key::D: return 'd';
    case Key::Q: return 'q';
    case Key::E: return 'e';
    default: return 0;
  }
}

void InputHandler::keyDown(Key key) {
  if (const unsigned char c = movement_char(key)) camera.MovementKeyPressed(c);
}

void InputHandler::keyUp(Key key) {
  if (const unsigned char c = movement_char(key)) camera.MovementKeyReleased(c);
  else if (key == Key::ESCAPE) quit = true;                 // GL::platform::quit()
  else if (key == Key::O) renderer.switchRenderOracle();
}

void InputHandler::buttonDown(Button button, int x, int y) {
  if (button == Button::LEFT) mouse_left = true;
  last_x = x;
  last_y = y;
}

void InputHandler::buttonUp(Button button, int, int) {
  if (button == Button::LEFT) mouse_left = false;
}

void InputHandler::mouseMove(int x, int y) {
  if (mouse_left && (x != last_x || y != last_y)) camera.MouseDrag(static_cast<float>(x - last_x), static_cast<float>(y - last_y));
  last_x = x;
  last_y = y;
}

static bool key_of(const std::string& s, Key* k) {
  static const struct { const char* name; Key key; } names[] = {{"w", Key::W}, {"a", Key::A}, {"s", Key::S}, {"d", Key::D},
      {"q", Key::Q}, {"e", Key::E}, {"o", Key::O}, {"f", Key::F}, {"backspace", Key::BACKSPACE}, {"esc", Key::ESCAPE}};
  for (const auto& n : names)
    if (s == n.name) {
      *k = n.key;
      return true;
    }
  return false;
}

bool InputHandler::replay(const char* line) {
  std::istringstream in(line);
  std::string tok;
  while (in >> tok) {
    if (tok[0] == '#') break;
    if (tok == "b+" || tok == "b-" || tok == "m") {
      int x, y;
      if (!(in >> x >> y)) return false;
      if (tok == "b+") buttonDown(Button::LEFT, x, y);
      else if (tok == "b-") buttonUp(Button::LEFT, x, y);
      else mouseMove(x, y);
    } else if (tok == "n" || tok == "thr") {
      // one value, read whole: "n 8", "thr 0.15"; the library validates the pair when the frame is rendered
      std::string val;
      if (!(in >> val)) return false;
      char* end = nullptr;
      if (tok == "n") {
        const long n = std::strtol(val.c_str(), &end, 10);
        if (end == val.c_str() || *end != 0 || n < 1 || n > 1 << 20) return false;
        renderer.setSelection(static_cast<int>(n), -1.f);
      } else {
        const float t = std::strtof(val.c_str(), &end);
        if (end == val.c_str() || *end != 0 || !(t >= 0.f)) return false;
        renderer.setSelection(0, t);
      }
    } else if (tok == "gaze") {
      // two values, each read whole: "gaze 400.5 300"; pixels, may lie outside the frame
      float v[2];
      for (float& x : v) {
        std::string val;
        if (!(in >> val)) return false;
        char* end = nullptr;
        x = std::strtof(val.c_str(), &end);
        if (end == val.c_str() || *end != 0 || !(x - x == 0.f)) return false;      // finite
      }
      renderer.setGaze(v[0], v[1]);
    } else if (tok == "cap") {
      // one value, read whole: "cap 4.5"; 0 removes the cap; the library validates it when the frame is rendered
      std::string val;
      if (!(in >> val)) return false;
      char* end = nullptr;
      const float x = std::strtof(val.c_str(), &end);
      if (end == val.c_str() || *end != 0 || !(x == 0.f || (x >= 1.f && x - x == 0.f))) return false;
      renderer.setSampleCap(x);
    } else if (tok == "cut") {
      renderer.cutHistory();
    } else if (tok == "size") {
      // two values, each read whole: "size 400 300"; the library validates the size when the frame is rendered
      long v[2];
      for (long& x : v) {
        std::string val;
        if (!(in >> val)) return false;
        char* end = nullptr;
        x = std::strtol(val.c_str(), &end, 10);
        if (end == val.c_str() || *end != 0 || x < 1 || x > 1 << 16) return false;
      }
      renderer.setFrameSize(static_cast<int>(v[0]), static_cast<int>(v[1]));
    } else if ((tok[0] == '+' || tok[0] == '-') && tok.size() > 1) {
      Key k;
      if (!key_of(tok.substr(1), &k)) return false;
      if (tok[0] == '+') keyDown(k);
      else keyUp(k);
    } else {
      return false;
    }
  }
  return true;
}
