"""CPU-only checks of the run-time frame size and the window presentation (adanerf_set_frame_size, adanerf_present): the C ABI declares
and exports both without a struct change, the integer definition of the presentation has the properties a blit must have, the hosts'
script grammar, command line and evaluator options accept what they should and nothing else.  What they render:
tests/test_gpu_set_frame_size.py and tests/test_gpu_present.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import present_reference as P
from conftest import ROOT

import adanerf_amd
from adanerf_amd import renderer as R


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def test_header_declares_and_library_exports_both_entry_points(lib, tmp_path):
    """A C99 translation unit that calls both compiles against include/adanerf_hip.h (-Wall -Werror -pedantic) and links against the
    library; the ABI version is still 4 and the three struct sizes are the header's and the Python mirror's; the ctypes host binds both."""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "set_frame_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "set_frame_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "set_frame_size(NULL) rc=-1 present(NULL) rc=-1 abi=4 flags=1,2,4"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # what the parent commit reports: no struct changed
    for name in ("adanerf_set_frame_size", "adanerf_present"):
        assert name in R.EXPORTS and hasattr(lib, name)
    assert lib.adanerf_set_frame_size(None, 0, 0) == -1          # ADANERF_EINVAL: no context
    assert lib.adanerf_present(None, None, 1, 1, None, 1, 1, 0) == -1
    assert lib.adanerf_abi_version() == 4
    assert (R.PRESENT_FLIP_Y, R.PRESENT_NEAREST, R.PRESENT_LINEAR) == (P.FLIP_Y, P.NEAREST, P.LINEAR) == (1, 2, 4)
    for name in ("set_frame_size", "present", "present_device"):
        assert name in dir(R.NeuralRenderer)
    sig = inspect.signature(R.NeuralRenderer.present).parameters
    assert list(sig)[1:] == ["window_w", "window_h", "flip_y", "filter"] and sig["flip_y"].default is False and sig["filter"].default is None


def test_python_settings_window_defaults_to_the_frame():
    s = R.Settings("m", 320, 200)
    assert (s.window_width, s.window_height) == (320, 200)
    s = R.Settings("m", 320, 200, window_width=1920, window_height=1080)
    assert (s.width, s.height, s.window_width, s.window_height) == (320, 200, 1920, 1080)
    # what the library is asked for: the batch as given, the library clamps it to the frame at every size
    assert R.Settings("m", 8, 8, batch_size=1000).requested_batch() == 1000 and R.Settings("m", 8, 8, batch_size=1000).resolved_batch() == 64
    assert R.Settings("m", 8, 8).requested_batch() == 0 and R.Settings("m", 10, 10, number_of_batches=3).requested_batch() == 34


# ---- the integer definition (tests/present_reference.py) ------------------------------------------

def _img(w, h, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img.reshape(-1)[::7] = 0
    img.reshape(-1)[3::11] = 255
    return img


SHAPES = [(1, 1), (2, 3), (7, 5), (33, 9), (97, 61)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_reference_equal_sizes_are_the_identity(w, h):
    img = _img(w, h, 1)
    for flags in (0, P.NEAREST, P.LINEAR):
        assert np.array_equal(P.present(img, w, h, flags), img)


@pytest.mark.parametrize("fx,fy", [(2, 2), (3, 1), (1, 4), (5, 3)])
def test_reference_nearest_at_an_integer_factor_replicates(fx, fy):
    img = _img(7, 5, 2)
    out = P.present(img, 7 * fx, 5 * fy, P.NEAREST)
    assert np.array_equal(out, np.repeat(np.repeat(img, fy, axis=0), fx, axis=1))
    # and down again by the same factor picks one pixel of every block: the original
    assert np.array_equal(P.present(out, 7, 5, P.NEAREST), img)


@pytest.mark.parametrize("dw,dh", [(1, 1), (5, 3), (14, 10), (13, 11), (40, 7), (3, 200), (1920, 2)])
def test_reference_linear_of_a_constant_is_that_constant(dw, dh):
    for value in (0, 1, 127, 254, 255):
        img = np.full((5, 7, 4), value, np.uint8)
        assert np.all(P.present(img, dw, dh, P.LINEAR) == value)


@pytest.mark.parametrize("sw,dw", [(2, 9), (7, 13), (7, 14), (33, 40), (40, 33), (256, 97), (3, 16384)])
def test_reference_linear_of_a_ramp_is_monotone(sw, dw):
    ramp = np.linspace(0, 255, sw).round().astype(np.uint8)
    img = np.repeat(ramp[None, :, None], 4, axis=2).repeat(3, axis=0)
    out = P.present(img, dw, 5, P.LINEAR).astype(np.int64)
    assert np.all(np.diff(out, axis=1) >= 0)
    if dw >= sw:      # an upscale's outermost pixel centres lie outside the source's: clamped to the edge
        assert out[:, 0].min() == 0 and out[:, -1].max() == 255
    assert np.all(out == out[:1])          # rows of a column ramp are equal
    down = P.present(img[:, ::-1], dw, 5, P.LINEAR).astype(np.int64)
    assert np.array_equal(down, out[:, ::-1])      # the filter is symmetric


@pytest.mark.parametrize("flags", [P.NEAREST, P.LINEAR, 0])
def test_reference_flip_y_reverses_the_rows(flags):
    img = _img(33, 9, 3)
    for dw, dh in ((40, 7), (13, 11), (33, 9), (5, 1)):
        assert np.array_equal(P.present(img, dw, dh, flags | P.FLIP_Y), P.present(img, dw, dh, flags)[::-1])


@pytest.mark.parametrize("sw,sh,dw,dh", [(7, 5, 13, 11), (33, 9, 40, 7), (97, 61, 64, 48), (1, 1, 5, 3), (3, 3, 2000, 1), (2, 300, 3, 2)])
def test_reference_results_lie_within_their_taps(sw, sh, dw, dh):
    img = _img(sw, sh, 4)
    out = P.present(img, dw, dh, P.LINEAR)
    lo, hi = P.tap_bounds(img, dw, dh)
    assert np.all(out >= lo) and np.all(out <= hi)
    assert out.dtype == np.uint8 and out.shape == (dh, dw, 4)


def test_reference_rule_and_flag_checks():
    assert P.uses_linear(64, 128) and not P.uses_linear(64, 64) and not P.uses_linear(128, 64)
    assert P.uses_linear(128, 64, P.LINEAR) and not P.uses_linear(64, 128, P.NEAREST)
    with pytest.raises(ValueError):
        P.uses_linear(8, 8, P.NEAREST | P.LINEAR)
    # taps: pixel centres; the first and last destination pixel of an upscale clamp to the edge
    t0, t1, f = P.linear_taps(2, 4)
    assert t0.tolist() == [0, 0, 0, 1] and t1.tolist() == [0, 1, 1, 1] and f.tolist() == [6, 2, 6, 2]
    assert P.nearest_taps(3, 7).tolist() == [0, 0, 1, 1, 1, 2, 2] and P.nearest_taps(7, 3).tolist() == [1, 3, 5]


# ---- hosts ------------------------------------------------------------------------------------------

LINES = [
    # (script line, parses, size pending, w, h, selection pending, n, oracle view toggled)
    ("size 32 24", True, True, 32, 24, False, 0, False),
    ("size 1 1", True, True, 1, 1, False, 0, False),
    ("+w size 640 480 -w", True, True, 640, 480, False, 0, False),
    ("size 64 48 n 4 -o", True, True, 64, 48, True, 4, True),
    ("size 64 48 size 32 24", True, True, 32, 24, False, 0, False),      # the last one of a line holds
    ("n 8", True, False, 0, 0, True, 8, False),
    ("size 32 24 # size abc", True, True, 32, 24, False, 0, False),      # a comment ends the line
    ("size", False, False, 0, 0, False, 0, False),
    ("size 32", False, False, 0, 0, False, 0, False),
    ("size 32 x", False, False, 0, 0, False, 0, False),
    ("size 32.5 24", False, False, 0, 0, False, 0, False),
    ("size 0 24", False, False, 0, 0, False, 0, False),
    ("size 32 -24", False, False, 0, 0, False, 0, False),
    ("size 32 24x", False, False, 0, 0, False, 0, False),
    ("size 70000 24", False, False, 0, 0, False, 0, False),
    ("size 32 24 12", False, True, 32, 24, False, 0, False),             # refused at the stray word; the host stops at a malformed line
    ("Size 32 24", False, False, 0, 0, False, 0, False),
]

ARGS = [
    # (command line, parses, frame, window, -w, --write-window, batch as the viewer's Settings has it, batch asked of the library)
    (["m", "-s", "64", "48"], True, (64, 48), (64, 48), 0, 0, 3072, 0),
    (["m", "-s", "64", "48", "-ws", "128", "96"], True, (64, 48), (128, 96), 0, 0, 3072, 0),
    (["m", "--windowSize", "128", "96", "--size", "64", "48", "-w"], True, (64, 48), (128, 96), 1, 0, 3072, 0),
    (["m", "-s", "64", "48", "--write-window"], True, (64, 48), (64, 48), 0, 1, 3072, 0),
    (["m", "-s", "64", "48", "-ws", "80", "60", "-w", "--write-window"], True, (64, 48), (80, 60), 1, 1, 3072, 0),
    (["m", "-s", "8", "8", "-bs", "1000"], True, (8, 8), (8, 8), 0, 0, 64, 1000),
    (["m", "-s", "64", "48", "-bs", "-1"], True, (64, 48), (64, 48), 0, 0, 3072, 0),
    (["m", "-s", "64", "48", "-nb", "4"], True, (64, 48), (64, 48), 0, 0, 768, 768),
    (["m", "-s", "64", "48", "-ws", "128"], False, None, None, 0, 0, 0, 0),
    (["m", "-s", "64", "48", "-ws", "0", "96"], False, None, None, 0, 0, 0, 0),
]


@pytest.fixture(scope="module")
def check_exe(lib, tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a C++ compiler is needed to build the replay check"
    from adanerf_amd.build import HOST, LIBDIR
    srcs = [os.path.join(HOST, f) for f in sorted(os.listdir(HOST)) if f.endswith(".cpp") and f != "main.cpp"]
    exe = str(tmp_path_factory.mktemp("size_token") / "replay_size_token_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "replay_size_token_check.cpp")] + srcs +
                   ["-L", LIBDIR, "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def test_script_grammar_accepts_and_rejects_the_size_token(check_exe):
    """InputHandler::replay through a stand-alone program over the host's own sources: `size W H` reaches NeuralRenderer::setFrameSize
    next to the other events of the line; a missing, malformed or out-of-range value and a stray word make the line malformed."""
    out = subprocess.run([check_exe] + [ln for ln, *_ in LINES], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().splitlines()
    assert len(got) == len(LINES)
    for (line, ok, size_pending, w, h, sel_pending, n, oracle), g in zip(LINES, got):
        f = dict(kv.split("=") for kv in g.split()[1:])
        assert g.split()[0] == ("ok" if ok else "bad"), (line, g)
        assert (int(f["size_pending"]), int(f["w"]), int(f["h"]), int(f["sel_pending"]), int(f["n"]), int(f["oracle"])) == \
               (int(size_pending), w, h, int(sel_pending), n, int(oracle)), (line, g)
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "size <W> <H>" in usage and "--write-window" in usage and "-ws|--windowSize W H" in usage


def test_command_line_stores_the_window_size(check_exe):
    for argv, ok, frame, window, write, write_window, batch, request in ARGS:
        out = subprocess.run([check_exe, "--settings"] + argv, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        g = out.stdout.strip()
        assert g.split()[0] == ("ok" if ok else "bad"), (argv, g)
        if ok:
            f = dict(kv.split("=") for kv in g.split()[1:])
            assert f["size"] == "%dx%d" % frame and f["window"] == "%dx%d" % window, (argv, g)
            assert (int(f["write"]), int(f["write_window"]), int(f["batch"]), int(f["request"])) == (write, write_window, batch, request), (argv, g)


def test_cli_dry_run_replays_the_size_token(lib, tmp_path):
    """--dry-run needs no device: a size token is validated by the code adanerf_create runs, and the batches per frame (camera steps)
    follow the size from the next frame on."""
    import adanerf_oracle as O
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    cli = adanerf_amd.build.build_cli()
    good = tmp_path / "good.txt"
    good.write_text("+w\nsize 32 24 n 4\n-w size 16 12\n")
    out = subprocess.run([cli, md, "-s", "16", "12", "--script", str(good), "--dry-run", "--log-camera"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and len([l for l in out.stdout.splitlines() if l.startswith("camera ")]) == 3, out.stdout + out.stderr
    for text, msg in (("+w\nsize 32\n", "malformed script line 2: size 32"), ("size 8192 4096\n", "width*height must be < 2^25")):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        out = subprocess.run([cli, md, "-s", "16", "12", "--script", str(bad), "--dry-run"], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and msg in out.stdout, out.stdout


def test_evaluator_scale_option_and_directory_names():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["m", "d"])
    assert a.sweep_scales is None and a.sweep_thresholds is None and a.sweep_samples is None      # without them: the evaluator as it was
    a = ap.parse_args(["m", "d", "--sweep-scales", "0.5", "1", "--out", "o"])
    assert a.sweep_scales == [0.5, 1.0] and a.sweep_samples is None and a.out == "o"
    a = ap.parse_args(["m", "d", "--sweep-samples", "4", "8", "--sweep-scales", "0.25", "--sweep-thresholds", "0.1"])
    assert (a.sweep_samples, a.sweep_thresholds, a.sweep_scales) == ([4, 8], [0.1], [0.25])
    for argv in (["m", "d", "--sweep-scales", "half"], ["m", "d", "--sweep-scales"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    assert E.sweep_dir_name(8, 0.1) == "n8_t0.1" and E.sweep_dir_name(128, 0.0) == "n128_t0"          # unchanged without a scale
    assert E.sweep_dir_name(8, 0.1, 0.5) == "n8_t0.1_s0.5" and E.sweep_dir_name(8, 0.2, 1.0) == "n8_t0.2_s1"
    assert E.sweep_dir_name(16, 0.05, 0.25) == "n16_t0.05_s0.25" and E.sweep_dir_name(4, 0.0, 2) == "n4_t0_s2"
    assert E.scaled_size(12, 10, 0.5) == (6, 5) and E.scaled_size(800, 800, 1) == (800, 800) and E.scaled_size(97, 61, 0.01) == (1, 1)
    assert E.scaled_size(800, 600, 0.75) == (600, 450)
    sig = inspect.signature(E.evaluate).parameters
    assert sig["sweep_scales"].default is None and list(sig)[-1] == "sweep_scales"
    # the summary of a run without the flag has the keys it had: no `scale`, no `sweep`
    recs = [dict(frame=0, image="x", samples_per_ray=3.0, ms=1.0, mse=0.01, psnr=20.0)]
    assert sorted(E.summarise(recs, False)) == ["frames", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    with pytest.raises(ValueError):
        E.evaluate("m", "d", sweep_scales=[0.5, 0.0])
