#include "settings.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

const char* Settings::usage() {
  return "Usage: adanerf [modelPath] [-s|--size W H] [-ws|--windowSize W H] [-bs|--batchSize N]\n"
         "               [-nb|--numberOfBatches N] [-w|--writeImages] [-d|--debug]\n"
         "               [--write-window]     also write the frame presented at the window size (-ws): out_window.bmp\n"
         "               [--frames N] [--precision bf16|fp16|fp32] [--sampling auto|guarded|split|fp32|fp16]\n"
         "               [--yaw DEG] [--pitch DEG]\n"
         "               [--samples N] [--threshold T] [--oracle]\n"
         "               [--sample-cap X]                   a hard bound on the samples of every frame: at most X per ray on average (X >= 1);\n"
         "                                                  the threshold is raised on the device by exactly as much as that needs\n"
         "               [--fovea R:N:T[,R:N:T...],N:T]     per-ray budgets: rings around the gaze (radius px : N : threshold), then the\n"
         "                                                  entry outside them; the gaze starts at the frame centre\n"
         "               [--fovea-density R:S[,R:S...],S]   foveated ray density: rings around the gaze (radius px : stride 1|2|4|8), then the\n"
         "                                                  stride outside them; every S-th pixel per axis is rendered, the rest rebuilt\n"
         "               [--fovea-temporal ALPHA]           with --fovea-density: the lattice moves through a 64-phase cycle and every frame is\n"
         "                                                  resolved against a history; rendered pixels refresh it with weight ALPHA in (0, 1],\n"
         "                                                  reconstructed pixels keep what they have\n"
         "               [--occluder cx,cy,cz,r[,R,G,B]]    hybrid rendering (repeatable): every ray stops at the nearest of these spheres and its\n"
         "                                                  flat colour (0..1, default 0.5 grey) shows through what the volume in front leaves\n"
         "               [--script FILE] [--log-camera] [--dry-run]     input replay: one line of events per frame\n"
         "                                                              (+w -w ... b+ x y  b- x y  m x y; n <int> / thr <float>:\n"
         "                                                              sample budget N / threshold from that frame on;\n"
         "                                                              size <W> <H>: frame size from that frame on, the window stays;\n"
         "                                                              gaze <X> <Y>: the --fovea / --fovea-density gaze, px;\n"
         "                                                              cap <X>: the --sample-cap bound from that frame on, cap 0 removes it;\n"
         "                                                              cut: --taa / --taau / --fovea-temporal start a new history with that frame)\n"
         "               [--reproject K]      of every K frames render the first and warp it to the camera of the next K - 1 (depth\n"
         "                                    reprojection, holes filled from their neighbours); -w / --write-window write what was shown\n"
         "               [--reproject-warp splat|gather]  with --reproject K: splat (default) scatters source pixels (adanerf_reproject); gather\n"
         "                                    iterates each shown pixel along its ray to the source surface (adanerf_reproject_gather: no cracks)\n"
         "               [--reproject-iterations N] [--reproject-tol T]   the gather's steps per pixel (1..8, default 4) and the relative depth\n"
         "                                    tolerance of its consistency test (default 0.05)\n"
         "               [--rerender holes|unsourced]     with --reproject K: render the warped frames' holes (unsourced: the pixels filled from a\n"
         "                                    neighbour, or gathered but unverified, too) at their own camera instead of leaving them\n"
         "               [--interpolate K]    show the same frames K frames late: of every K frames render the first as a keyframe and make the\n"
         "                                    K - 1 before it from the keyframe behind and the keyframe ahead (adanerf_reproject_pair, K >= 2);\n"
         "                                    --rerender applies to those frames\n"
         "               [--supersample S]    every shown frame is S x S renders (S in 1..8) at the offsets of a regular sub-pixel grid, summed and\n"
         "                                    averaged on the device (anti-aliasing in time); -w / --write-window write the resolved image\n"
         "               [--supersample-contrast T]   with --supersample S >= 2: one render at the pixel centres, then the S x S renders only for\n"
         "                                    the pixels a neighbour of which differs by more than T (0..1) in some channel (adaptive supersampling)\n"
         "               [--taa ALPHA[:TOL]]  temporal anti-aliasing: every frame is rendered at the next sub-pixel offset of a cycle and blended\n"
         "                                    (weight ALPHA in (0, 1]) with a history carried to its camera by its depth; a history pixel whose depth\n"
         "                                    is off by more than TOL (relative, default 0.02) is dropped; script token cut drops the history\n"
         "               [--taa-grid S]       the cycle of --taa: the S x S regular sub-pixel grid, S in 1..8 (default 2)\n"
         "               [--taau S[:ALPHA[:TOL]]]  temporal upsampling: -s W H stays the render size; every frame is rendered at the next offset of the\n"
         "                                    S x S sub-pixel cycle (S in 1..4) and resolved into a history of S W x S H (weight ALPHA in (0, 1], default\n"
         "                                    0.1; neighbourhood depth tolerance TOL, default 0.02); -w / --write-window write the S W x S H frame;\n"
         "                                    script tokens cut and size drop the history\n"
         "               [--present-filter nearest|linear|area]     filter of the -ws window image; default: linear if the window is wider than\n"
         "                                    the frame, else nearest (the viewer's blit); area: exact area filter, for a frame rendered larger\n"
         "               [--gpus N] [--same-device] [--sub-shares P]\n";
}

// R:N:T[,R:N:T...],N:T -- every field read whole; what adanerf_foveate would refuse is refused here, with the spec in the message
bool Settings::parseFovea(const std::string& spec, std::vector<int>* radius, std::vector<int>* n, std::vector<float>* thr, std::string* err) {
  auto bad = [&](const char* why) {
    *err = "--fovea " + spec + ": " + why + " (expected R:N:T[,R:N:T...],N:T)";
    return false;
  };
  radius->clear();
  n->clear();
  thr->clear();
  std::vector<std::string> parts(1);
  for (char ch : spec) {
    if (ch == ',') parts.emplace_back();
    else parts.back() += ch;
  }
  for (size_t k = 0; k < parts.size(); ++k) {
    std::vector<std::string> f(1);
    for (char ch : parts[k]) {
      if (ch == ':') f.emplace_back();
      else f.back() += ch;
    }
    const bool last = k + 1 == parts.size();
    if (f.size() != (last ? 2u : 3u)) return bad(last ? "the last entry must be N:T" : "a ring must be R:N:T");
    char* end = nullptr;
    for (size_t j = 0; j + 1 < f.size(); ++j) {
      const long v = std::strtol(f[j].c_str(), &end, 10);
      if (end == f[j].c_str() || *end != 0) return bad("not an integer");
      const bool is_radius = !last && j == 0;
      if (is_radius && (v < 0 || v > 0x7fffffffl || (!radius->empty() && v <= radius->back()))) return bad("radii must be >= 0 and strictly ascending");
      if (!is_radius && (v < 0 || v > 255)) return bad("N must be in 0..255");
      (is_radius ? radius : n)->push_back(static_cast<int>(v));
    }
    const float t = std::strtof(f.back().c_str(), &end);
    if (end == f.back().c_str() || *end != 0 || t != t) return bad("a threshold is not a number");
    thr->push_back(t);
  }
  if (radius->size() > 8) return bad("at most 8 rings");
  return true;
}

// R:S[,R:S...],S -- every field read whole; what adanerf_foveate_density would refuse is refused here, with the spec in the message
bool Settings::parseFoveaDensity(const std::string& spec, std::vector<int>* radius, std::vector<int>* stride, std::string* err) {
  auto bad = [&](const char* why) {
    *err = "--fovea-density " + spec + ": " + why + " (expected R:S[,R:S...],S)";
    return false;
  };
  radius->clear();
  stride->clear();
  std::vector<std::string> parts(1);
  for (char ch : spec) {
    if (ch == ',') parts.emplace_back();
    else parts.back() += ch;
  }
  for (size_t k = 0; k < parts.size(); ++k) {
    std::vector<std::string> f(1);
    for (char ch : parts[k]) {
      if (ch == ':') f.emplace_back();
      else f.back() += ch;
    }
    const bool last = k + 1 == parts.size();
    if (f.size() != (last ? 1u : 2u)) return bad(last ? "the last entry must be S" : "a ring must be R:S");
    for (size_t j = 0; j < f.size(); ++j) {
      char* end = nullptr;
      const long v = std::strtol(f[j].c_str(), &end, 10);
      if (end == f[j].c_str() || *end != 0) return bad("not an integer");
      const bool is_radius = !last && j == 0;
      if (is_radius && (v < 0 || v > 0x7fffffffl || (!radius->empty() && v <= radius->back()))) return bad("radii must be >= 0 and strictly ascending");
      if (!is_radius && v != 1 && v != 2 && v != 4 && v != 8) return bad("a stride must be 1, 2, 4 or 8");
      if (!is_radius && !stride->empty() && v < stride->back()) return bad("strides must not decrease outward");
      (is_radius ? radius : stride)->push_back(static_cast<int>(v));
    }
  }
  if (radius->size() > 8) return bad("at most 8 rings");
  return true;
}

// cx,cy,cz,r[,R,G,B] -- every field read whole; what adanerf_host_sphere_zc would refuse is refused here, with the spec in the message
bool Settings::parseOccluder(const std::string& spec, Occluder* out, std::string* err) {
  auto bad = [&](const char* why) {
    *err = "--occluder " + spec + ": " + why + " (expected cx,cy,cz,r[,R,G,B])";
    return false;
  };
  std::vector<std::string> f(1);
  for (char ch : spec) {
    if (ch == ',') f.emplace_back();
    else f.back() += ch;
  }
  if (f.size() != 4 && f.size() != 7) return bad("four or seven values");
  float v[7] = {0.f, 0.f, 0.f, 0.f, 0.5f, 0.5f, 0.5f};
  for (size_t k = 0; k < f.size(); ++k) {
    char* end = nullptr;
    v[k] = std::strtof(f[k].c_str(), &end);
    if (end == f[k].c_str() || *end != 0 || !std::isfinite(v[k])) return bad("not a finite number");
  }
  if (!(v[3] > 0.f)) return bad("the radius must be > 0");
  for (int k = 0; k < 3; ++k) {
    out->center[k] = v[k];
    out->rgb[k] = v[4 + k];
  }
  out->radius = v[3];
  return true;
}

bool Settings::init(int argc, char** argv, std::string* err) {
  bool bs_used = false, ws_used = false, model_set = false;
  int batch_arg = -1;
  unsigned int n_batches = 1;
  auto need = [&](int i, int n) {
    if (i + n >= argc) {
      *err = std::string("missing value after ") + argv[i];
      return false;
    }
    return true;
  };
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-s" || a == "--size") {
      if (!need(i, 2)) return false;
      width = static_cast<unsigned>(std::atoi(argv[i + 1]));
      height = static_cast<unsigned>(std::atoi(argv[i + 2]));
      i += 2;
    } else if (a == "-ws" || a == "--windowSize") {
      if (!need(i, 2)) return false;
      window_width = static_cast<unsigned>(std::atoi(argv[i + 1]));
      window_height = static_cast<unsigned>(std::atoi(argv[i + 2]));
      ws_used = true;
      i += 2;
    } else if (a == "-bs" || a == "--batchSize") {
      if (!need(i, 1)) return false;
      batch_arg = std::atoi(argv[++i]);
      bs_used = true;
    } else if (a == "-nb" || a == "--numberOfBatches") {
      if (!need(i, 1)) return false;
      n_batches = static_cast<unsigned>(std::max(1, std::atoi(argv[++i])));
    } else if (a == "-w" || a == "--writeImages") {
      write_images = true;
    } else if (a == "--write-window") {
      write_window = true;
    } else if (a == "-d" || a == "--debug") {
      is_debug = true;
    } else if (a == "--frames") {
      if (!need(i, 1)) return false;
      frames = std::atoi(argv[++i]);
    } else if (a == "--precision") {
      if (!need(i, 1)) return false;
      precision = argv[++i];
    } else if (a == "--sampling") {
      if (!need(i, 1)) return false;
      sampling = argv[++i];
      if (sampling != "auto" && sampling != "guarded" && sampling != "split" && sampling != "fp32" && sampling != "fp16") {
        *err = "--sampling must be auto, guarded, split, fp32 or fp16";
        return false;
      }
    } else if (a == "--yaw") {
      if (!need(i, 1)) return false;
      yaw = static_cast<float>(std::atof(argv[++i]));
    } else if (a == "--pitch") {
      if (!need(i, 1)) return false;
      pitch = static_cast<float>(std::atof(argv[++i]));
    } else if (a == "--samples") {
      if (!need(i, 1)) return false;
      num_samples = std::atoi(argv[++i]);
    } else if (a == "--threshold") {
      if (!need(i, 1)) return false;
      threshold = static_cast<float>(std::atof(argv[++i]));
    } else if (a == "--gpus") {
      if (!need(i, 1)) return false;
      gpus = std::max(1, std::atoi(argv[++i]));
    } else if (a == "--same-device") {
      same_device = true;
    } else if (a == "--sub-shares") {
      if (!need(i, 1)) return false;
      sub_shares = std::max(1, std::min(4, std::atoi(argv[++i])));
    } else if (a == "--fovea") {
      if (!need(i, 1)) return false;
      if (!parseFovea(argv[++i], &fovea_radius, &fovea_n, &fovea_thr, err)) return false;
    } else if (a == "--fovea-density") {
      if (!need(i, 1)) return false;
      if (!parseFoveaDensity(argv[++i], &density_radius, &density_stride, err)) return false;
    } else if (a == "--fovea-temporal") {
      if (!need(i, 1)) return false;
      const std::string as = argv[++i];
      char* ea = nullptr;
      const float al = std::strtof(as.c_str(), &ea);
      if (as.empty() || *ea != 0 || !(al > 0.f && al <= 1.f)) {
        *err = "--fovea-temporal ALPHA: ALPHA must lie in (0, 1]";
        return false;
      }
      fovea_temporal_alpha = al;
    } else if (a == "--occluder") {
      if (!need(i, 1)) return false;
      Occluder o;
      if (!parseOccluder(argv[++i], &o, err)) return false;
      occluders.push_back(o);
    } else if (a == "--reproject") {
      if (!need(i, 1)) return false;
      char* end = nullptr;
      const long k = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || k < 1 || k > 1000000) {
        *err = "--reproject K: K must be an integer >= 1";
        return false;
      }
      reproject = static_cast<int>(k);
    } else if (a == "--interpolate") {
      if (!need(i, 1)) return false;
      char* end = nullptr;
      const long k = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || k < 2 || k > 1000000) {
        *err = "--interpolate K: K must be an integer >= 2";
        return false;
      }
      interpolate = static_cast<int>(k);
    } else if (a == "--reproject-warp") {
      if (!need(i, 1)) return false;
      const std::string v = argv[++i];
      if (v != "splat" && v != "gather") {
        *err = "--reproject-warp must be splat or gather";
        return false;
      }
      reproject_gather = v == "gather";
      reproject_warp_set = true;
    } else if (a == "--reproject-iterations") {
      if (!need(i, 1)) return false;
      char* end = nullptr;
      const long k = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || k < 1 || k > 8) {
        *err = "--reproject-iterations N: N must be an integer in 1..8";
        return false;
      }
      reproject_iterations = static_cast<int>(k);
      reproject_warp_set = true;
    } else if (a == "--reproject-tol") {
      if (!need(i, 1)) return false;
      const std::string ts = argv[++i];
      char* et = nullptr;
      const float t = std::strtof(ts.c_str(), &et);
      if (ts.empty() || *et != 0 || !(t >= 0.f) || !(t < 1e30f)) {
        *err = "--reproject-tol T: T must be a number >= 0";
        return false;
      }
      reproject_tol = t;
      reproject_warp_set = true;
    } else if (a == "--rerender") {
      if (!need(i, 1)) return false;
      rerender = argv[++i];
      if (rerender != "holes" && rerender != "unsourced") {
        *err = "--rerender must be holes or unsourced";
        return false;
      }
    } else if (a == "--supersample") {
      if (!need(i, 1)) return false;
      char* end = nullptr;
      const long k = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || k < 1 || k > 8) {
        *err = "--supersample S: S must be an integer in 1..8";
        return false;
      }
      supersample = static_cast<int>(k);
    } else if (a == "--sample-cap") {
      if (!need(i, 1)) return false;
      char* end = nullptr;
      const float x = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end != 0 || !(x == 0.f || (x >= 1.f && x - x == 0.f))) {
        *err = "--sample-cap X: X must be 0 (off) or a finite number >= 1";
        return false;
      }
      sample_cap = x;
    } else if (a == "--supersample-contrast") {
      if (!need(i, 1)) return false;
      char* end = nullptr;
      const float t = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end != 0 || !(t >= 0.f && t <= 1.f)) {
        *err = "--supersample-contrast T: T must be a number in [0, 1]";
        return false;
      }
      supersample_contrast = t;
    } else if (a == "--taa") {
      if (!need(i, 1)) return false;
      const std::string spec = argv[++i];
      const size_t colon = spec.find(':');
      const std::string as = spec.substr(0, colon), ts = colon == std::string::npos ? "0.02" : spec.substr(colon + 1);
      char *ea = nullptr, *et = nullptr;
      const float al = std::strtof(as.c_str(), &ea), tl = std::strtof(ts.c_str(), &et);
      if (as.empty() || *ea != 0 || ts.empty() || *et != 0 || !(al > 0.f && al <= 1.f) || !(tl >= 0.f && tl < INFINITY)) {
        *err = "--taa ALPHA[:TOL]: ALPHA must lie in (0, 1], TOL must be a number >= 0";
        return false;
      }
      taa_alpha = al;
      taa_tol = tl;
    } else if (a == "--taa-grid") {
      if (!need(i, 1)) return false;
      char* end = nullptr;
      const long k = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end != 0 || k < 1 || k > 8) {
        *err = "--taa-grid S: S must be an integer in 1..8";
        return false;
      }
      taa_grid = static_cast<int>(k);
    } else if (a == "--taau") {
      if (!need(i, 1)) return false;
      std::vector<std::string> f(1);
      for (const char* ch = argv[++i]; *ch; ++ch) {
        if (*ch == ':') f.emplace_back();
        else f.back() += *ch;
      }
      char *es = nullptr, *ea = nullptr, *et = nullptr;
      const long k = std::strtol(f[0].c_str(), &es, 10);
      const float al = f.size() > 1 ? std::strtof(f[1].c_str(), &ea) : 0.1f, tl = f.size() > 2 ? std::strtof(f[2].c_str(), &et) : 0.02f;
      bool ok = f.size() <= 3 && !f[0].empty() && *es == 0 && k >= 1 && k <= 4;
      ok = ok && (f.size() < 2 || (!f[1].empty() && *ea == 0)) && (f.size() < 3 || (!f[2].empty() && *et == 0));
      if (!ok || !(al > 0.f && al <= 1.f) || !(tl >= 0.f && tl < INFINITY)) {
        *err = "--taau S[:ALPHA[:TOL]]: S must be an integer in 1..4, ALPHA must lie in (0, 1], TOL must be a number >= 0";
        return false;
      }
      taau_scale = static_cast<int>(k);
      taau_alpha = al;
      taau_tol = tl;
    } else if (a == "--present-filter") {
      if (!need(i, 1)) return false;
      present_filter = argv[++i];
      if (present_filter != "nearest" && present_filter != "linear" && present_filter != "area") {
        *err = "--present-filter must be nearest, linear or area";
        return false;
      }
    } else if (a == "--oracle") {
      render_oracle = true;
    } else if (a == "--script") {
      if (!need(i, 1)) return false;
      script = argv[++i];
    } else if (a == "--log-camera") {
      log_camera = true;
    } else if (a == "--dry-run") {
      dry_run = true;
    } else if (a == "-h" || a == "--help") {
      *err = usage();
      return false;
    } else if (!a.empty() && a[0] != '-' && !model_set) {
      model_path = a;
      model_set = true;
    } else {
      *err = "unknown argument " + a;
      return false;
    }
  }
  if (width == 0 || height == 0) {
    *err = "size must be positive";
    return false;
  }
  if (ws_used && (window_width == 0 || window_height == 0)) {
    *err = "window size must be positive";
    return false;
  }
  if (interpolate > 1) {      // two keyframes of one context, rendered plainly and shown K frames late
    const char* why = reproject > 1 ? "--interpolate makes the frames between two keyframes; not with --reproject, which warps the last one"
                      : taa_alpha > 0.f ? "--interpolate shows keyframes as rendered; not with --taa"
                      : taau_scale > 0 ? "--interpolate shows keyframes as rendered; not with --taau"
                      : supersample > 1 ? "--interpolate: the mean of jittered frames has no depth map to warp by; not with --supersample"
                      : !density_stride.empty() ? "--interpolate: the lattice is not coupled to the other stages; not with --fovea-density"
                      : !occluders.empty() ? "--interpolate: the reprojection stages take no depth limit; not with --occluder"
                      : gpus > 1 ? "--interpolate warps whole frames of one context; use it with --gpus 1"
                      : render_oracle ? "--interpolate warps rendered frames; not with --oracle"
                                      : nullptr;
    if (why) {
      *err = why;
      return false;
    }
  }
  if (!rerender.empty() && reproject <= 1 && interpolate <= 1) {
    *err = "--rerender re-renders the holes of warped frames; only with --reproject K, K > 1";
    return false;
  }
  if (reproject_warp_set && reproject <= 1) {
    *err = "--reproject-warp / --reproject-iterations / --reproject-tol choose how warped frames are made; only with --reproject K, K > 1";
    return false;
  }
  if (supersample_contrast >= 0.f && supersample <= 1) {
    *err = "--supersample-contrast refines the edges of a supersampled frame; only with --supersample S, S >= 2";
    return false;
  }
  if (taa_alpha > 0.f && (reproject > 1 || supersample > 1)) {
    *err = reproject > 1 ? "--taa renders and resolves every frame; not with --reproject"
                         : "--taa spends one render per frame on a cycle of sub-pixel offsets; not with --supersample";
    return false;
  }
  if (taau_scale > 0 && (taa_alpha > 0.f || reproject > 1 || supersample > 1 || gpus > 1 || render_oracle)) {
    *err = taa_alpha > 0.f ? "--taau is a temporal resolve of its own; not with --taa"
           : reproject > 1 ? "--taau renders and resolves every frame; not with --reproject"
           : supersample > 1 ? "--taau spends one render per frame on a cycle of sub-pixel offsets; not with --supersample"
           : gpus > 1 ? "--taau resolves whole frames of one context; use it with --gpus 1"
                      : "--taau blends rendered frames; not with --oracle";
    return false;
  }
  if (!occluders.empty() && (gpus > 1 || render_oracle || reproject > 1 || supersample > 1 || taa_alpha > 0.f || taau_scale > 0)) {
    *err = gpus > 1 ? "--occluder blends whole frames of one context; use it with --gpus 1"
           : render_oracle ? "--occluder limits rendered frames; not with --oracle"
                           : "--occluder: the temporal and reprojection stages take no depth limit; not with --reproject, --supersample, --taa or --taau";
    return false;
  }
  if (!density_stride.empty()) {      // adanerf_render_masked's own limits, and the stages that take whole rendered frames
    const char* why = !fovea_n.empty() ? "a budget map is indexed by frame position and the masked render refuses it; not with --fovea"
                      : (gpus > 1 || sub_shares > 1) ? "the reconstruction reads a pixel's neighbours in whole frames of one context; use it with --gpus 1 and --sub-shares 1"
                      : (sampling == "fp16" || sampling == "fp32") ? "the masked render needs the split or guarded sampling mode; not with --sampling fp16 or fp32"
                      : render_oracle ? "it reconstructs rendered frames; not with --oracle"
                      : (reproject > 1 || supersample > 1 || taa_alpha > 0.f || taau_scale > 0 || !occluders.empty())
                          ? "the lattice is not coupled to the other stages; not with --reproject, --supersample, --taa, --taau or --occluder"
                          : nullptr;
    if (why) {
      *err = std::string("--fovea-density: ") + why;
      return false;
    }
  }
  if (sample_cap > 0.f && (!density_stride.empty() || !rerender.empty() || supersample_contrast >= 0.f || render_oracle)) {
    *err = render_oracle ? "--sample-cap bounds rendered frames; not with --oracle"
                         : "--sample-cap: the masked render refuses a cap (its threshold depends on which rays share a batch); not with --fovea-density, "
                           "--rerender or --supersample-contrast";
    return false;
  }
  if (fovea_temporal_alpha > 0.f && density_stride.empty()) {
    *err = "--fovea-temporal resolves the frames of a moving lattice; only with --fovea-density";
    return false;
  }
  total_size = width * height;
  if (sampling.empty()) sampling = "split";      // exact by construction; guarded / fp16 are opt-in (the default rule)
  if (!ws_used) {
    window_width = width;
    window_height = height;
  }
  // settings.cpp:38-46
  batch_size = static_cast<unsigned>(std::ceil(total_size / static_cast<float>(n_batches)));
  if (bs_used) batch_size = batch_arg <= 0 ? total_size : std::min(static_cast<unsigned>(batch_arg), total_size);
  batch_request = bs_used ? std::max(batch_arg, 0) : (n_batches > 1 ? static_cast<int>(batch_size) : 0);
  return true;
}
