"""CPU-only checks of the run-time sample budget / threshold (adanerf_set_selection): the C ABI declares and exports it, the hosts'
script grammar and the evaluator's options accept what they should and nothing else.  What it renders: tests/test_gpu_set_selection.py."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

import adanerf_amd
from adanerf_amd import renderer as R


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def test_header_declares_and_library_exports_set_selection(lib, tmp_path):
    """A C99 translation unit that calls adanerf_set_selection compiles against include/adanerf_hip.h (-Wall -Werror -pedantic) and links
    against the library; the ABI version is still 4; the ctypes host binds it."""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "set_selection_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "set_selection_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "set_selection(NULL) rc=-1 abi=4"
    assert "adanerf_set_selection" in R.EXPORTS and hasattr(lib, "adanerf_set_selection")
    assert lib.adanerf_set_selection(None, 0, -1.0) == -1          # ADANERF_EINVAL: no context
    assert "set_selection" in dir(R.NeuralRenderer) and "not re-measured" in R.NeuralRenderer.set_selection.__doc__


LINES = [
    # (script line, parses, pending, n, thr, oracle view toggled)
    ("n 8", True, True, 8, -1.0, False),
    ("thr 0.15", True, True, 0, 0.15, False),
    ("n 12 thr 0.05 -o", True, True, 12, 0.05, True),
    ("thr 0", True, True, 0, 0.0, False),
    ("+w n 128 -w", True, True, 128, -1.0, False),
    ("-o", True, False, 0, -1.0, True),
    ("n 4 # thr abc", True, True, 4, -1.0, False),          # a comment ends the line
    ("n", False, False, 0, -1.0, False),
    ("thr", False, False, 0, -1.0, False),
    ("thr abc", False, False, 0, -1.0, False),
    ("n 8 extra", False, True, 8, -1.0, False),             # refused at the unknown token; the host stops at a malformed line
    ("n 8.5", False, False, 0, -1.0, False),
    ("n 0", False, False, 0, -1.0, False),
    ("n -3", False, False, 0, -1.0, False),
    ("thr -0.5", False, False, 0, -1.0, False),
    ("thr nan", False, False, 0, -1.0, False),
    ("thr 0.1x", False, False, 0, -1.0, False),
]


def test_script_grammar_accepts_and_rejects_the_selection_tokens(lib, tmp_path):
    """InputHandler::replay through a stand-alone program over the host's own sources: `n <int>` and `thr <float>` reach
    NeuralRenderer::setSelection next to the other events of the line; a missing, malformed or out-of-range value and a stray word make the
    line malformed."""
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a C++ compiler is needed to build the replay check"
    from adanerf_amd.build import HOST, LIBDIR
    srcs = [os.path.join(HOST, f) for f in sorted(os.listdir(HOST)) if f.endswith(".cpp") and f != "main.cpp"]
    exe = str(tmp_path / "replay_tokens_check")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "replay_tokens_check.cpp")] + srcs +
                   ["-L", LIBDIR, "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe] + [ln for ln, *_ in LINES], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.strip().splitlines()
    assert len(got) == len(LINES)
    for (line, ok, pending, n, thr, oracle), g in zip(LINES, got):
        f = dict(kv.split("=") for kv in g.split()[1:])
        assert g.split()[0] == ("ok" if ok else "bad"), (line, g)
        assert (int(f["pending"]), int(f["n"]), int(f["oracle"])) == (int(pending), n, int(oracle)), (line, g)
        assert abs(float(f["thr"]) - thr) < 1e-6, (line, g)
    # the CLI documents the tokens, and refuses a script that misuses them, naming the line
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "n <int>" in usage and "thr <float>" in usage


def test_cli_dry_run_replays_selection_tokens(lib, tmp_path):
    import adanerf_oracle as O
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    cli = adanerf_amd.build.build_cli()
    good = tmp_path / "good.txt"
    good.write_text("+w\nn 4 thr 0.3\n-w thr 0.1\n")
    out = subprocess.run([cli, md, "-s", "16", "12", "--script", str(good), "--dry-run", "--log-camera"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and len([l for l in out.stdout.splitlines() if l.startswith("camera ")]) == 3, out.stdout + out.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("+w\nthr abc\n")
    out = subprocess.run([cli, md, "-s", "16", "12", "--script", str(bad), "--dry-run"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "malformed script line 2: thr abc" in out.stdout


def test_evaluator_sweep_options_and_directory_names():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["m", "d"])
    assert a.sweep_thresholds is None and a.sweep_samples is None            # without them: the evaluator as it was
    a = ap.parse_args(["m", "d", "--sweep-thresholds", "0.1", "0.3", "--out", "o"])
    assert a.sweep_thresholds == [0.1, 0.3] and a.sweep_samples is None and a.out == "o"
    a = ap.parse_args(["m", "d", "--sweep-samples", "4", "8", "16", "--sweep-thresholds", "0", "--metrics", "psnr", "flip"])
    assert a.sweep_samples == [4, 8, 16] and a.sweep_thresholds == [0.0] and a.metrics == ["psnr", "flip"]
    for argv in (["m", "d", "--sweep-samples", "4.5"], ["m", "d", "--sweep-thresholds", "low"], ["m", "d", "--sweep-samples"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    assert E.sweep_dir_name(8, 0.1) == "n8_t0.1" and E.sweep_dir_name(128, 0.0) == "n128_t0"
    assert E.sweep_dir_name(16, 0.05) == "n16_t0.05" and E.sweep_dir_name(4, 0.35) == "n4_t0.35"
    import inspect
    sig = inspect.signature(E.evaluate).parameters
    assert sig["sweep_thresholds"].default is None and sig["sweep_samples"].default is None
