"""CPU-only checks of foveated density over time (adanerf_foveate_density_phased / adanerf_fill_density_phased /
adanerf_host_density_mask_phased / adanerf_host_density_phase / adanerf_temporal_resolve_sparse): the C ABI declares and exports the five
without a struct change; the host mask -- the rule the device kernel compiles from the same header -- equals the brute-force numpy
definition (tests/sparse_temporal_reference.py) at all 64 phases, and every corner the phased fill would use is a rendered pixel; phase
(0, 0) is the unphased mask; the cycle covers every residue pair of every level in any L^2 consecutive frames; every refusal leaves its
output untouched; and the float32 restatement of the resolve is recorded against its float64 form.  What the device computes:
tests/test_gpu_sparse_temporal.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import density_reference as DR
import reproject_reference as RR
import sparse_temporal_reference as SR
from conftest import ROOT, load_case, record
from test_density_cpu import SPECIAL, random_settings

import adanerf_amd
from adanerf_amd import renderer as R

SIZES = ((48, 40), (37, 29), (5, 3))
NAMES = ("adanerf_foveate_density_phased", "adanerf_fill_density_phased", "adanerf_host_density_mask_phased", "adanerf_host_density_phase",
         "adanerf_temporal_resolve_sparse")
PHASES = [SR.phase_of(k) for k in range(64)]
ALL_8 = ((2.0, 1.0), [], [8])      # beside test_density_cpu.py's settings: on 5 x 3 most pixels have no corner on an axis at most phases


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


@pytest.fixture(scope="module")
def scene():
    return load_case("classroom_n8_thr02")[2]


def host_mask(lib, w, h, gaze, radius, stride, phase, out=None, n_rings=None):
    """(code, mask): adanerf_host_density_mask_phased through ctypes, with nothing checked on this side"""
    i32 = C.c_int32
    nr = len(radius) if n_rings is None else n_rings
    rad = None if radius is None else (i32 * max(len(radius), 1))(*radius)
    st = None if stride is None else (i32 * max(len(stride), 1))(*stride)
    if out is None:
        out = np.full(max(w * h, 1) if 0 < w * h < 1 << 28 else 1, 0xA5, np.uint8)
    rc = lib.adanerf_host_density_mask_phased(w, h, gaze[0], gaze[1], nr, rad, st, phase[0], phase[1], out.ctypes.data)
    return rc, out


def settings_of(w, h):
    """test_density_cpu.py's special settings, the first 20 of its random ones and the all-8 spec"""
    return SPECIAL + random_settings(w * 1000 + h, w, h, 20) + [ALL_8]


def test_header_declares_and_library_exports_the_entry_points(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "sparse_temporal_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "sparse_temporal_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert SR.phase_of(27) == (6, 5)
    assert lines[0] == ("foveate_density_phased(NULL) rc=-1 fill_density_phased(NULL) rc=-1 unfilled=-7 host_density_mask_phased rc=0 "
                        "host_density_phase(27) rc=0 6 5 temporal_resolve_sparse(NULL) rc=-1 rejected=-7 abi=4")
    assert [int(v) for v in lines[1].split()] == SR.mask_phased(4, 3, (1.5, 1.5), [1], [1, 2], (1, 1)).tolist()
    assert all(n in R.EXPORTS and hasattr(lib, n) for n in NAMES) and lib.adanerf_abi_version() == 4
    assert [C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)] == [64, 164, 96]      # no struct changed
    header = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in header
    assert "rotate the\n * lattice from frame to frame" not in header      # the item this closes is struck from "What it does not do"


def test_a_null_context_is_refused_before_any_device_work(lib):
    i32 = C.c_int32
    assert lib.adanerf_foveate_density_phased(None, 1.0, 1.0, 0, None, (i32 * 1)(1), 0, 0, 4096) == -1
    u = i32(-7)
    assert lib.adanerf_fill_density_phased(None, 4096, 4, 4, 0, 0, 8192, None, None, None, C.byref(u)) == -1 and u.value == -7
    pose = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert lib.adanerf_temporal_resolve_sparse(None, 4096, 0, 0, 8192, 8192, 8192, pose, pose, None, None, None, None, None, 0.1, 0.02, 0.5, 0, 8192, None,
                                               4096, None, None, C.byref(u)) == -1 and u.value == -7


@pytest.mark.parametrize("w,h", SIZES)
def test_host_mask_is_the_brute_force_definition_and_closes_every_corner_at_every_phase(lib, w, h):
    """all 64 phases: the host mask equals the brute-force rule; every corner the phased fill would use is a byte-0 pixel; phase (0, 0) is
    adanerf_host_density_mask byte for byte; over the 64 phases every pixel is rendered at least once, and a pixel whose ring has stride L at
    least once in any L^2 consecutive phases"""
    no_corner = 0
    for gaze, radius, stride in settings_of(w, h):
        s_map = DR.stride_map(w, h, gaze, radius, stride).reshape(-1)
        rendered = np.zeros((64, w * h), bool)
        for k, phase in enumerate(PHASES):
            rc, got = host_mask(lib, w, h, gaze, radius, stride, phase)
            assert rc == 0, (gaze, radius, stride, phase)
            want = SR.mask_phased(w, h, gaze, radius, stride, phase)
            assert np.array_equal(got, want), (gaze, radius, stride, phase, np.flatnonzero(got != want)[:8])
            assert np.array_equal(got[got != 0], s_map[got != 0].astype(np.uint8)) and np.all(got[s_map == 1] == 0)
            for p in np.flatnonzero(got).tolist():
                y, x = divmod(p, w)
                corners = SR.used_corners(x, y, int(got[p]), w, h, phase)
                assert all(got[c] == 0 for c in corners), (gaze, radius, stride, phase, x, y)
                no_corner += not corners
            rendered[k] = got == 0
            if phase == (0, 0):
                plain = np.full(w * h, 0xA5, np.uint8)
                i32 = C.c_int32
                assert lib.adanerf_host_density_mask(w, h, gaze[0], gaze[1], len(radius), (i32 * max(len(radius), 1))(*radius),
                                                     (i32 * len(stride))(*stride), plain.ctypes.data) == 0
                assert np.array_equal(got, plain) and np.array_equal(got, DR.density_mask(w, h, gaze, radius, stride))
                for p in np.flatnonzero(got).tolist():      # and the cell is the unphased one
                    y, x = divmod(p, w)
                    assert SR.used_corners(x, y, int(got[p]), w, h, phase) == DR.used_corners(x, y, int(got[p]), w, h)
        assert rendered.any(axis=0).all(), (gaze, radius, stride)
        twice = np.concatenate([rendered, rendered])      # the cycle repeats: windows that wrap
        for L in (2, 4, 8):
            of_L = s_map == L
            for k0 in range(64):
                assert twice[k0:k0 + L * L][:, of_L].any(axis=0).all(), (gaze, radius, stride, L, k0)
    if (w, h) == (5, 3):
        assert no_corner > 0      # a frame narrower than the stride: pixels with no corner on an axis


def test_the_cycle_hits_every_residue_pair_of_every_level_once(lib):
    got = []
    for k in range(-64, 192):
        px, py = C.c_int32(-9), C.c_int32(-9)
        assert lib.adanerf_host_density_phase(k, C.byref(px), C.byref(py)) == 0
        got.append((px.value, py.value))
        assert got[-1] == SR.phase_of(k) == R.density_phase(k) and 0 <= px.value <= 7 and 0 <= py.value <= 7
    assert got[64:128] == PHASES and got[:64] == PHASES and PHASES[0] == (0, 0) and len(set(PHASES)) == 64
    for L in (2, 4, 8):
        for k0 in range(64):
            seen = {(SR.phase_of(k)[0] % L, SR.phase_of(k)[1] % L) for k in range(k0, k0 + L * L)}
            assert len(seen) == L * L, (L, k0)
    assert R.density_phase(2 ** 31 + 5) == SR.phase_of(5)


def test_every_refusal_leaves_the_output_untouched(lib):
    w, h = 9, 7
    ok = ((4.0, 3.0), [2, 5], [1, 2, 4])
    assert host_mask(lib, w, h, *ok, (7, 7))[0] == 0
    for phase in ((-1, 0), (0, -1), (8, 0), (0, 8), (64, 64), (-8, 3)):
        rc, out = host_mask(lib, w, h, *ok, phase)
        assert rc == -1 and np.all(out == 0xA5), phase
        assert "adanerf_host_density_mask_phased" in lib.adanerf_last_error(None).decode()
        with pytest.raises(ValueError):
            R.density_mask_phased(w, h, ok[0], [(2, 1), (5, 2), (4,)], phase)
    nan = float("nan")
    bad = [((nan, 3.0), [2, 5], [1, 2, 4], None), (ok[0], [], [1], -1), (ok[0], [5, 2], [1, 2, 4], None), (ok[0], [2, 5], [1, 3, 4], None),
           (ok[0], [2, 5], [2, 1, 4], None), (ok[0], None, [1, 2, 4], 2), (ok[0], [2, 5], None, 2)]
    for gaze, radius, stride, nr in bad:      # what the unphased call refuses
        rc, out = host_mask(lib, w, h, gaze, radius, stride, (3, 5), n_rings=nr)
        assert rc == -1 and np.all(out == 0xA5), (gaze, radius, stride, nr)
    for ww, hh in ((0, 7), (9, 0), (16385, 7)):
        rc, out = host_mask(lib, ww, hh, *ok, (1, 1), out=np.full(64, 0xA5, np.uint8))
        assert rc == -1 and np.all(out == 0xA5), (ww, hh)
    i32 = C.c_int32
    assert lib.adanerf_host_density_mask_phased(w, h, 4.0, 3.0, 0, None, (i32 * 1)(1), 0, 0, None) == -1      # a NULL mask
    px, py = i32(-9), i32(-9)
    assert lib.adanerf_host_density_phase(3, None, C.byref(py)) == -1 and lib.adanerf_host_density_phase(3, C.byref(px), None) == -1
    assert (px.value, py.value) == (-9, -9)
    assert np.array_equal(R.density_mask_phased(w, h, ok[0], "2:1,5:2,4", (3, 5)), SR.mask_phased(w, h, *ok, (3, 5)))


def test_python_host_signatures():
    P = lambda f: list(inspect.signature(f).parameters)
    N = R.NeuralRenderer
    assert P(N.foveate_density_phased_device) == ["self", "gaze_xy", "rings", "phase_xy", "mask"]
    assert P(N.fill_density_phased_device) == ["self", "mask", "width", "height", "phase_xy", "rgb", "depth_map", "acc_map", "rgba8", "count"]
    assert P(N.temporal_resolve_sparse_device)[:16] == ["self", "mask", "phase_xy", "cur_rgb", "cur_depth", "cur_acc", "cur_pos", "cur_rot", "hist_rgb",
                                                        "hist_depth", "hist_count", "prev_pos", "prev_rot", "out_rgb", "out_depth", "out_count"]
    sig = inspect.signature(N.enable_foveated_temporal).parameters
    assert list(sig) == ["self", "alpha", "depth_tol", "clamp"] and (sig["alpha"].default, sig["depth_tol"].default, sig["clamp"].default) == (0.1, 0.02, True)
    assert P(N.render_foveated_temporal) == ["self"] and P(N.reset_foveated_temporal) == ["self"]
    assert P(N.render_foveated) == ["self"]      # unchanged


@pytest.mark.parametrize("w,h", SR.SIZES, ids=["%dx%d" % s for s in SR.SIZES])
def test_the_float32_restatement_against_its_float64_form(scene, w, h):
    """the residual of the definition against the same steps in float64, on every geometric case of the GPU tests: recorded, no bound.
    What must hold exactly are the things no rounding enters: without a history every pixel is rejected and shows the frame's bits, rendered
    pixels start at count 1 and reconstructed ones at 0; a reconstructed pixel that is live shows the history and keeps its count."""
    hr, hd, hc, prev = SR.history_at(scene, w, h, False)
    n = w * h
    worst = dict(tap=0, mask=0, colour=0.0)
    for motion, phase, with_depth, clamp in SR.geometric_cases():
        mask = SR.resolve_mask(w, h, phase)
        cur = SR.current_at(scene, w, h, mask, phase)
        dst = RR.moved(scene, **RR.MOTIONS[motion])
        args = (scene, w, h, False, mask, phase) + cur + dst + (hr, hd if with_depth else None, hc) + prev
        kw = dict(depth_tol=SR.TEST_TOL, flags=SR.CLAMP if clamp else 0)
        a, b = SR.sparse_f32(*args, **kw), SR.sparse_f64(*args, **kw)
        same = (a.tap == b.tap) & (a.mask == b.mask)
        both = same & a.live & np.all(np.isfinite(a.rgb) & np.isfinite(b.rgb), axis=1)
        worst["tap"] = max(worst["tap"], int(np.count_nonzero(a.tap != b.tap)))
        worst["mask"] = max(worst["mask"], int(np.count_nonzero(a.mask != b.mask)))
        if both.any():
            worst["colour"] = max(worst["colour"], float(np.max(np.abs(a.rgb[both].astype(np.float64) - b.rgb[both]))))
        rebuilt_live = a.live & np.isin(mask, (2, 4, 8))
        assert np.array_equal(a.count[rebuilt_live], hc[a.tap[rebuilt_live]]) and np.all(a.count[a.live & (mask == 0)] >= 2)
        assert np.all(a.count[~a.live] == (mask[~a.live] == 0)) and np.all(a.mask[mask == SR.FOREIGN] == 0)
        assert np.array_equal(a.rgb[~a.live].view(np.uint32), np.ascontiguousarray(cur[0], np.float32)[~a.live].view(np.uint32))
        if motion == "sees_none":
            assert a.rejected == n
    print("%dx%d: float32 against float64 over %d pixels: taps differing %d, verdicts differing %d, largest colour residual %.3g"
          % (w, h, n, worst["tap"], worst["mask"], worst["colour"]))
    record("sparse_temporal_f32_vs_f64", size="%dx%d" % (w, h), taps_differing=worst["tap"], verdicts_differing=worst["mask"], colour_residual=worst["colour"])
    mask = SR.resolve_mask(w, h, (3, 5))
    cur = SR.current_at(scene, w, h, mask, (3, 5))
    first = SR.sparse_f32(scene, w, h, False, mask, (3, 5), *cur, *prev, None, None, None, None, None)
    assert first.rejected == n and not first.mask.any() and np.array_equal(first.count, (mask == 0).astype(np.uint8))
    assert np.array_equal(first.rgb.view(np.uint32), np.ascontiguousarray(cur[0], np.float32).view(np.uint32))


# ---- hosts ------------------------------------------------------------------------------------------------------

def test_cli_parses_the_fovea_temporal_flag(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--fovea-temporal ALPHA" in usage and "cut: --taa / --taau / --fovea-temporal" in usage
    model = os.path.join(str(ROOT), "no_such_model")
    for bad in ("0", "-0.1", "1.5", "x", "", "0.1:0.02", "nan"):
        out = subprocess.run([cli, "m", "--fovea-density", "5:1,2", "--fovea-temporal", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--fovea-temporal ALPHA: ALPHA must lie in (0, 1]" in out.stdout, bad
    out = subprocess.run([cli, "m", "--fovea-temporal"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "missing value after --fovea-temporal" in out.stdout
    out = subprocess.run([cli, model, "--fovea-temporal", "0.1", "--dry-run", "--frames", "1"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "only with --fovea-density" in out.stdout
    for extra, why in ((["--taa", "0.1"], "not with --reproject"), (["--gpus", "2"], "--gpus 1"), (["--fovea", "50:8:0.2,2:0.3"], "not with --fovea")):
        out = subprocess.run([cli, model, "--fovea-density", "5:1,2", "--fovea-temporal", "0.1"] + extra + ["--dry-run", "--frames", "1"], capture_output=True,
                             text=True, timeout=60)
        assert out.returncode != 0 and "--fovea-density: " in out.stdout and why in out.stdout, extra      # --fovea-density's own refusals hold
    for order in (["--fovea-density", "5:1,2", "--fovea-temporal", "0.1"], ["--fovea-temporal", "1", "--fovea-density", "8"]):
        out = subprocess.run([cli, model] + order + ["--dry-run", "--frames", "1"], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "config.ini" in out.stdout and "Argument parsing failed" not in out.stdout, order      # parsed: it fails on the model


def test_evaluator_takes_the_fovea_temporal_options(tmp_path):
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["m", "d"])
    assert a.fovea_temporal is None and a.fovea_temporal_still is None
    a = ap.parse_args(["m", "d", "--fovea-density", "5:1,2", "--fovea-temporal", "0.2", "--fovea-temporal-still", "8"])
    assert a.fovea_temporal == 0.2 and a.fovea_temporal_still == 8
    sig = inspect.signature(E.evaluate).parameters
    assert sig["fovea_temporal"].default is None and sig["fovea_temporal_still"].default is None and list(sig)[-4:] == ["fovea_temporal", "fovea_temporal_still", "supersample_contrast", "sweep_scales"]
    for kw in (dict(fovea_temporal=0.2), dict(fovea_temporal_still=3), dict(fovea_density="5:1,2", fovea_temporal=0.0),
               dict(fovea_density="5:1,2", fovea_temporal=1.5), dict(fovea_density="5:1,2", fovea_temporal_still=0),
               dict(fovea_density="5:1,2", fovea_temporal_still=2.5), dict(fovea_density="5:1,2", fovea_temporal=0.1, temporal=0.1)):
        with pytest.raises(ValueError):
            E.evaluate(str(tmp_path / "no_model"), str(tmp_path / "no_dataset"), **kw)
    for argv in (["--fovea-temporal", "0.2"], ["--fovea-temporal-still", "3"], ["--fovea-density", "5:1,2", "--fovea-temporal", "2"],
                 ["--fovea-density", "5:1,2", "--fovea-temporal-still", "0"]):
        with pytest.raises(SystemExit):
            E.main(["m", "d"] + argv)
    fov = [dict(frame=0, samples_per_ray=4.0, ms=1.0, mse=0.01, psnr=20.0, rendered_fraction=0.2, mse_foveated=0.02, psnr_foveated=17.0, ms_foveated=0.3)]
    res = [dict(fov[0], foveated_temporal_rejected_fraction=0.5, mse_foveated_temporal=0.015, psnr_foveated_temporal=18.0)]
    s0, s1 = E.summarise(fov, False), E.summarise(res, False)
    assert sorted(s1) == sorted(list(s0) + ["mean_psnr_foveated_temporal", "mean_foveated_temporal_rejected_fraction"])
    assert all(s1[k] == s0[k] for k in s0) and (s1["mean_psnr_foveated_temporal"], s1["mean_foveated_temporal_rejected_fraction"]) == (18.0, 0.5)
