"""CPU-only checks of foveated ray density (adanerf_foveate_density / adanerf_fill_density / adanerf_host_density_mask): the C ABI declares
and exports the three without a struct change; the host mask -- the rule the device kernel compiles from the same header -- equals the
brute-force numpy definition (tests/density_reference.py) byte for byte; every corner the fill would read is a rendered pixel; the
rendered counts the documents quote; every refusal leaves the output untouched; and the Python parser, the CLI and the evaluator accept
and refuse the same settings.  What the device computes: tests/test_gpu_density.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import density_reference as DR
from conftest import ROOT

import adanerf_amd
from adanerf_amd import renderer as R

SIZES = ((48, 40), (37, 29))
NAMES = ("adanerf_foveate_density", "adanerf_fill_density", "adanerf_host_density_mask")


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def host_mask(lib, w, h, gaze, radius, stride, out=None, n_rings=None):
    """(code, mask): adanerf_host_density_mask through ctypes, with nothing checked on this side"""
    i32 = C.c_int32
    nr = len(radius) if n_rings is None else n_rings
    rad = None if radius is None else (i32 * max(len(radius), 1))(*radius)
    st = None if stride is None else (i32 * max(len(stride), 1))(*stride)
    if out is None:
        out = np.full(max(w * h, 1) if 0 < w * h < 1 << 28 else 1, 0xA5, np.uint8)
    rc = lib.adanerf_host_density_mask(w, h, gaze[0], gaze[1], nr, rad, st, out.ctypes.data)
    return rc, out


def random_settings(seed, w, h, count):
    """(gaze, radius, stride) * count: the gaze inside and outside the image, 0..4 rings, strides that never decrease"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        nr = int(rng.integers(0, 5))
        radius = sorted(int(r) for r in rng.choice(np.arange(0, max(w, h)), nr, replace=False))
        stride = sorted(int(s) for s in rng.choice([1, 2, 4, 8], nr + 1))
        gaze = (float(np.float32(rng.uniform(-0.5 * w, 1.5 * w))), float(np.float32(rng.uniform(-0.5 * h, 1.5 * h))))
        if rng.integers(0, 4) == 0:      # half-pixel and whole-pixel gazes: the ties of the nearest-centre rule
            gaze = (float(np.round(gaze[0] * 2) / 2), float(np.round(gaze[1])))
        out.append((gaze, radius, stride))
    return out


SPECIAL = [((24.0, 20.0), [], [1]), ((24.0, 20.0), [], [8]), ((3.25, 2.75), [5, 11], [1, 1, 1]), ((-1000.0, 2000.0), [3], [2, 4]),
           ((1e30, -1e30), [4, 9], [1, 2, 8]), ((18.5, 14.5), [0], [1, 8]), ((18.5, 14.5), [0, 1, 2, 3, 4, 5, 6, 7], [1, 1, 2, 2, 4, 4, 8, 8, 8])]


def test_header_declares_and_library_exports_the_entry_points(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "density_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "density_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "foveate_density(NULL) rc=-1 fill_density(NULL) rc=-1 unfilled=-7 host_density_mask rc=0 abi=4"
    assert [int(v) for v in lines[1].split()] == DR.density_mask(4, 3, (1.5, 1.5), [1], [1, 2]).tolist() == [0, 0, 0, 2] * 3
    assert all(n in R.EXPORTS and hasattr(lib, n) for n in NAMES) and lib.adanerf_abi_version() == 4
    assert [C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)] == [64, 164, 96]      # no struct changed
    header = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in header
    assert "What it does not do: combine with budget maps" in header


def test_a_null_context_is_refused_before_any_device_work(lib):
    i32 = C.c_int32
    assert lib.adanerf_foveate_density(None, 1.0, 1.0, 0, None, (i32 * 1)(1), 4096) == -1
    u = i32(-7)
    assert lib.adanerf_fill_density(None, 4096, 4, 4, 8192, None, None, None, C.byref(u)) == -1 and u.value == -7


@pytest.mark.parametrize("w,h", SIZES)
def test_host_mask_is_the_brute_force_definition_and_closes_every_corner(lib, w, h):
    settings = SPECIAL + random_settings(w * 1000 + h, w, h, 80)
    seen = set()
    for gaze, radius, stride in settings:
        rc, got = host_mask(lib, w, h, gaze, radius, stride)
        assert rc == 0, (gaze, radius, stride)
        want = DR.density_mask(w, h, gaze, radius, stride)
        assert np.array_equal(got, want), (gaze, radius, stride, np.flatnonzero(got != want)[:8])
        assert set(np.unique(got).tolist()) <= {0, 2, 4, 8}
        seen |= set(np.unique(got).tolist())
        s = DR.stride_map(w, h, gaze, radius, stride).reshape(-1)
        assert np.array_equal(got[got != 0], s[got != 0].astype(np.uint8)) and np.all(got[s == 1] == 0)
        for p in np.flatnonzero(got).tolist():      # every corner the fill of an unrendered pixel uses is a rendered pixel
            y, x = divmod(p, w)
            assert all(got[c] == 0 for c in DR.used_corners(x, y, int(got[p]), w, h)), (gaze, radius, stride, x, y)
        if all(v == 1 for v in stride):
            assert not got.any()
        if stride == [8]:
            yy, xx = np.divmod(np.arange(w * h), w)
            assert np.array_equal(got == 0, (yy % 8 == 0) & (xx % 8 == 0))
    assert seen == {0, 2, 4, 8}


def test_rendered_counts_the_documents_quote(lib):
    for (w, h), spec, count in (((800, 800), "120:1,300:2,4", 127399), ((1920, 1080), "200:1,500:2,4", 371879)):
        radius, stride = DR.parse_spec(spec)
        rc, m = host_mask(lib, w, h, (0.5 * w, 0.5 * h), radius, stride)
        assert rc == 0 and int(np.count_nonzero(m == 0)) == count
        assert np.array_equal(m, R.density_mask(w, h, (0.5 * w, 0.5 * h), spec))
        assert [tuple(r) for r in R.parse_fovea_density(spec)] == [(r, s) for r, s in zip(radius, stride)] + [(stride[-1],)]


def test_every_refusal_leaves_the_output_untouched(lib):
    w, h = 9, 7
    nan, inf = float("nan"), float("inf")
    ok = ((4.0, 3.0), [2, 5], [1, 2, 4])
    assert host_mask(lib, w, h, *ok)[0] == 0
    bad = [((nan, 3.0), [2, 5], [1, 2, 4], None), ((4.0, inf), [2, 5], [1, 2, 4], None), ((4.0, -inf), [], [1], None),
           (ok[0], [], [1], -1), (ok[0], list(range(9)), [1] * 10, None),
           (ok[0], [-1, 5], [1, 2, 4], None), (ok[0], [5, 5], [1, 2, 4], None), (ok[0], [5, 2], [1, 2, 4], None),
           (ok[0], [2, 5], [1, 3, 4], None), (ok[0], [2, 5], [0, 2, 4], None), (ok[0], [2, 5], [1, 2, 16], None), (ok[0], [2, 5], [1, 2, -2], None),
           (ok[0], [2, 5], [2, 1, 4], None), (ok[0], [2, 5], [1, 4, 2], None), (ok[0], [], [3], None),
           (ok[0], None, [1, 2, 4], 2), (ok[0], [2, 5], None, 2), (ok[0], [], None, 0)]
    for gaze, radius, stride, nr in bad:
        rc, out = host_mask(lib, w, h, gaze, radius, stride, n_rings=nr)
        assert rc == -1 and np.all(out == 0xA5), (gaze, radius, stride, nr)
        assert "adanerf_host_density_mask" in lib.adanerf_last_error(None).decode()
    for ww, hh in ((0, 7), (9, 0), (-1, 7), (16385, 7), (9, 16385)):
        rc, out = host_mask(lib, ww, hh, *ok, out=np.full(64, 0xA5, np.uint8))
        assert rc == -1 and np.all(out == 0xA5), (ww, hh)
    i32 = C.c_int32
    assert lib.adanerf_host_density_mask(w, h, 4.0, 3.0, 0, None, (i32 * 1)(1), None) == -1      # a NULL mask
    rc, out = host_mask(lib, w, h, ok[0], None, [4], n_rings=0)      # zero rings need no radius array
    assert rc == 0 and np.array_equal(out, DR.density_mask(w, h, ok[0], [], [4]))
    for bad_py in (dict(width=0, height=4), dict(width=4, height=1 << 15)):
        with pytest.raises(ValueError):
            R.density_mask(gaze_xy=(1, 1), rings=[(1,)], **bad_py)
    with pytest.raises(ValueError):
        R.density_mask(4, 4, (nan, 1.0), [(1,)])


GOOD_SPECS = ["1", "8", "120:1,300:2,4", "200:1,500:2,8", "0:1,2", "5:2,2", "1:1,2:1,3:2,4:2,5:4,6:4,7:8,8:8,8", " 3:1 , 4"]
BAD_SPECS = ["", ",", "3", "16", "0", "-2", "1:1", "1:1,", ",2", "5:1,3:2,4", "5:1,5:2,4", "-1:1,2", "5:2,1", "5:1,6:4,2", "5:3,4", "5:1:2,4", "5,4",
             "x:1,2", "5:x,2", "5:1,x", "1.5:1,2", "5:1,2.0", "1:1,2:1,3:1,4:1,5:1,6:1,7:1,8:1,9:1,1", "2147483648:1,2"]


def test_parse_fovea_density():
    assert R.parse_fovea_density("120:1,300:2,4") == [(120, 1), (300, 2), (4,)]
    assert R.parse_fovea_density("8") == [(8,)]
    for spec in GOOD_SPECS:
        rings = R.parse_fovea_density(spec)
        assert all(len(r) == 2 for r in rings[:-1]) and len(rings[-1]) == 1 and len(rings) <= 9
    for spec in BAD_SPECS:
        with pytest.raises(ValueError):
            R.parse_fovea_density(spec)


def test_cli_parser_accepts_and_refuses_what_the_python_parser_does(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--fovea-density R:S[,R:S...],S" in usage
    model = os.path.join(str(ROOT), "no_such_model")

    def run(*args):
        return subprocess.run([cli, model] + list(args) + ["--dry-run", "--frames", "1"], capture_output=True, text=True, timeout=60)
    for spec in GOOD_SPECS:
        if spec != spec.strip() or " " in spec:      # the shell form has no blanks
            continue
        out = run("--fovea-density", spec)
        assert out.returncode != 0 and "config.ini" in out.stdout and "Argument parsing failed" not in out.stdout, spec      # parsed: it fails on the model
    for spec in BAD_SPECS:
        out = run("--fovea-density", spec)
        assert out.returncode != 0 and "--fovea-density " + spec in out.stdout and "expected R:S[,R:S...],S" in out.stdout, spec
    out = subprocess.run([cli, "m", "--fovea-density"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "missing value after --fovea-density" in out.stdout
    for extra, why in ((["--fovea", "50:8:0.2,2:0.3"], "not with --fovea"), (["--gpus", "2"], "--gpus 1"), (["--sub-shares", "2"], "--sub-shares 1"),
                       (["--sampling", "fp16"], "not with --sampling fp16 or fp32"), (["--sampling", "fp32"], "not with --sampling fp16 or fp32"),
                       (["--oracle"], "not with --oracle"), (["--reproject", "2"], "not with --reproject"), (["--supersample", "2"], "not with --reproject"),
                       (["--taa", "0.1"], "not with --reproject"), (["--taau", "2"], "not with --reproject"), (["--occluder", "0,0,0,1"], "not with --reproject")):
        for args in (["--fovea-density", "5:1,2"] + extra, extra + ["--fovea-density", "5:1,2"]):
            out = run(*args)
            assert out.returncode != 0 and "--fovea-density: " in out.stdout and why in out.stdout, args
    for fine in (["--sampling", "split"], ["--sampling", "guarded"], ["--gpus", "1", "--sub-shares", "1"]):
        out = run("--fovea-density", "5:1,2", *fine)
        assert out.returncode != 0 and "config.ini" in out.stdout and "Argument parsing failed" not in out.stdout, fine


def test_python_host_signatures():
    sig = inspect.signature(R.NeuralRenderer.foveate_density).parameters
    assert list(sig) == ["self", "gaze_xy", "rings"]
    assert list(inspect.signature(R.NeuralRenderer.render_foveated).parameters) == ["self"]
    sig = inspect.signature(R.NeuralRenderer.fill_density_device).parameters
    assert list(sig) == ["self", "mask", "width", "height", "rgb", "depth_map", "acc_map", "rgba8", "count"]
    assert R.DENSITY_STRIDES == (1, 2, 4, 8)


def test_evaluator_takes_a_fovea_density(tmp_path):
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["m", "d"]).fovea_density is None
    assert ap.parse_args(["m", "d", "--fovea-density", "120:1,300:2,4"]).fovea_density == "120:1,300:2,4"
    assert inspect.signature(E.evaluate).parameters["fovea_density"].default is None
    for bad in ("5:1,3:2,4", "5:3,4", ""):
        with pytest.raises(ValueError):
            E.evaluate(str(tmp_path / "no_model"), str(tmp_path / "no_dataset"), fovea_density=bad)
    with pytest.raises(SystemExit):
        E.main(["m", "d", "--fovea-density", "5:3,4"])
    plain = [dict(frame=0, samples_per_ray=4.0, ms=1.0, mse=0.01, psnr=20.0, warped=False)]
    fov = [dict(plain[0], rendered_fraction=0.2, mse_foveated=0.02, psnr_foveated=17.0, ms_foveated=0.3)]
    s0, s1 = E.summarise(plain, False), E.summarise(fov, False)
    assert sorted(s1) == sorted(list(s0) + ["mean_psnr_foveated", "mean_rendered_fraction", "mean_ms_foveated"])
    assert all(s1[k] == s0[k] for k in s0) and (s1["mean_psnr_foveated"], s1["mean_rendered_fraction"], s1["mean_ms_foveated"]) == (17.0, 0.2, 0.3)
