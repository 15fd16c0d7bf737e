"""CPU-only checks of the temporal resolve (adanerf_temporal_resolve): the C ABI declares and exports it without a struct change, both
hosts and the evaluator expose it, the restatement the GPU tests compare against (tests/temporal_reference.py) has the properties a
temporal filter must have, and the inputs of those tests keep pixel-boundary and depth-tolerance ties rare enough for exact equality to
be a fair demand.  What the kernel computes: tests/test_gpu_temporal.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import reproject_reference as RR
import temporal_reference as TR
from conftest import ROOT, load_case

import adanerf_amd
from adanerf_amd import renderer as R

F32 = np.float32
W, H = RR.SIZES[0]


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


@pytest.fixture(scope="module")
def scene():
    return load_case("classroom_n8_thr02")[2]


def test_header_declares_and_library_exports_the_entry_point(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "temporal_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "temporal_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "temporal_resolve(NULL) rc=-1 rejected=-7 abi=4 clamp=1"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # no struct changed
    assert "adanerf_temporal_resolve" in R.EXPORTS and hasattr(lib, "adanerf_temporal_resolve") and R.TEMPORAL_CLAMP == TR.CLAMP == 1
    assert lib.adanerf_abi_version() == 4


def test_a_null_context_is_refused_before_any_device_work(lib):
    f3, f9 = (C.c_float * 3)(0, 0, 0), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    rejected = C.c_int32(-7)
    assert lib.adanerf_temporal_resolve(None, None, None, None, f3, f9, None, None, None, f3, f9, 0.1, 0.02, 0.5, R.TEMPORAL_CLAMP, None, None, None, None,
                                        None, C.byref(rejected)) == -1
    assert lib.adanerf_temporal_resolve(None, 4096, 4096, 4096, f3, f9, 8192, 8192, 8192, f3, f9, 0.1, 0.02, 0.5, 0, 16384, None, None, None, None, None) == -1
    assert rejected.value == -7


def test_python_host_signatures():
    for name in ("enable_temporal", "render_temporal", "reset_temporal", "temporal_resolve_device"):
        assert name in dir(R.NeuralRenderer)
    sig = inspect.signature(R.NeuralRenderer.enable_temporal).parameters
    assert list(sig)[1:] == ["alpha", "depth_tol", "clamp", "grid"]
    assert (sig["alpha"].default, sig["depth_tol"].default, sig["clamp"].default, sig["grid"].default) == (0.1, 0.02, True, 2)
    assert list(inspect.signature(R.NeuralRenderer.render_temporal).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.reset_temporal).parameters) == ["self"]
    # the methods it stands beside keep theirs
    assert list(inspect.signature(R.NeuralRenderer.render_numpy).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.render_supersampled).parameters) == ["self", "s"]


# ---- properties of the definition ------------------------------------------------------------------

def resolve(scene, w, h, cur, hist, cur_pose, prev_pose, camera_origin=False, f=TR.temporal_f32, **kw):
    return f(scene, w, h, camera_origin, cur[0], cur[1], cur[2], cur_pose[0], cur_pose[1], hist[0], hist[1], hist[2], prev_pose[0], prev_pose[1], **kw)


@pytest.mark.parametrize("w,h", RR.SIZES)
def test_no_history_returns_the_current_frame(scene, w, h):
    cur = TR.current_at(scene, w, h, 1)
    pose = RR.src_pose(scene)
    for flags in (0, TR.CLAMP):
        out = resolve(scene, w, h, cur, (None, None, None), pose, (None, None), flags=flags)
        assert np.array_equal(out.rgb.view(np.uint32), cur[0].view(np.uint32))      # the bits, NaNs and signed zeros included
        assert np.all(out.mask == 0) and out.rejected == w * h and np.all(out.count == 1) and np.all(out.tap == -1)
        assert np.all(out.depth > 0) and np.count_nonzero(np.isinf(out.depth)) >= (w if h >= 3 else 0)      # the far row comes out at +inf


@pytest.mark.parametrize("w,h", RR.SIZES)
@pytest.mark.parametrize("camera_origin", [False, True])
def test_identity_pose_with_constant_images_gives_the_constant(scene, w, h, camera_origin):
    n = w * h
    _, dm, acc, _ = RR.depth_scene(w, h, 1, planted=False)
    pose = RR.src_pose(scene)
    const = np.full((n, 3), F32(0.3), F32) * F32([1.0, 2.0, -1.0])
    first = resolve(scene, w, h, (const, dm, acc), (None, None, None), pose, (None, None), camera_origin)
    for flags in (0, TR.CLAMP):
        for count in (None, first.count):
            out = resolve(scene, w, h, (const, dm, acc), (first.rgb, first.depth, count), pose, pose, camera_origin, flags=flags)
            assert out.rejected == 0 and np.all(out.mask == 1) and np.array_equal(out.tap, np.arange(n))
            assert np.array_equal(out.rgb, const)      # c + wx (c - c) and c + a (c - c) are c
            assert np.array_equal(out.depth.view(np.uint32), first.depth.view(np.uint32))
            assert np.all(out.count == (2 if count is not None else 1))


def test_lateral_move_rejects_the_band_the_box_uncovers(scene):
    """The frame a render at the new pose would give, built from the depth warp of the old one (two shells of constant distance, as
    tests/test_reproject_cpu.py): where the warp has holes the new camera sees wall the old one did not -- behind the box, and at the
    frame's edge.  Those pixels, and no others, are rejected."""
    for right in (0.04, 0.1):
        rgba, depth, acc, is_box = RR.depth_scene(W, H, 3, planted=False)
        acc = np.ones_like(acc)
        depth = (np.where(is_box, F32(1.5), F32(4.0)) * acc).astype(F32)
        src, dst = RR.src_pose(scene), RR.moved(scene, right=right)
        bare = RR.reproject_f32(scene, W, H, True, rgba, depth, acc, src[0], src[1], dst[0], dst[1], RR.ACC_MIN, RR.HOLE, 0)
        holes = bare[2] == 0
        nds, _ = RR.rays_f32(scene, W, H, dst[0], dst[1])
        rot = np.asarray(dst[1], F32).reshape(9)
        cos = -((rot[2] * nds[:, 0] + rot[5] * nds[:, 1]) + rot[8] * nds[:, 2])      # camera depth per unit of ray length from the camera
        t = np.where(holes, F32(4.0), np.where(holes, F32(1), bare[1]) / cos).astype(F32)
        hist = resolve(scene, W, H, (TR.colours(W, H, 5, False), depth, acc), (None, None, None), src, (None, None), True)
        out = resolve(scene, W, H, (TR.colours(W, H, 6, False), t, acc), (hist.rgb, hist.depth, hist.count), dst, src, True)
        x0, x1, y0, y1 = RR.box_of(W, H)
        band = np.flatnonzero(holes & (out.tap >= 0))      # holes whose point lies inside the old frame: the old camera saw the box there
        print("right %g: holes %d, of them behind the box %d, rejected %d" % (right, holes.sum(), band.size, out.rejected))
        assert np.array_equal(out.mask == 0, holes)
        assert band.size >= (y1 - y0 - 2) and np.all(is_box[out.tap[band]]) and np.all(np.abs(band % W - x1) <= 8)
        assert np.all(out.count[holes] == 1) and np.all(out.count[~holes] == 2)


def test_with_a_count_at_rest_the_weights_are_those_of_a_running_mean(scene):
    """1, 1/2, 1/3, ...: after k frames the history is the mean of the k frames, until 1 / k falls below alpha.  To 2e-5: at rest a pixel's
    point comes back to its own centre only to the rounding of the projection (some 1e-6 of a pixel at this size), so the bilinear
    history is the pixel's own value plus that share of a neighbour's, and the values lie in [0, 1)."""
    w, h = RR.SIZES[1]
    n = w * h
    _, dm, acc, _ = RR.depth_scene(w, h, 1, planted=False)
    pose = RR.src_pose(scene)
    rng = np.random.default_rng(11)
    frames = [rng.random((n, 3)).astype(F32) for _ in range(14)]
    alpha = 0.1
    hist, total = (None, None, None), np.zeros((n, 3), np.float64)
    for k, frame in enumerate(frames, 1):
        out = resolve(scene, w, h, (frame, dm, acc), hist, pose, pose if k > 1 else (None, None), alpha=alpha, flags=0)
        assert np.all(out.count == k) and out.rejected == (n if k == 1 else 0)
        if k <= 10:      # 1 / k >= alpha
            total += frame
            assert np.max(np.abs(out.rgb - total / k)) < 2e-5
            if k > 1:
                assert np.max(np.abs(out.rgb - (prev + F32(F32(1) / F32(k)) * (frame - prev)))) < 2e-5
        else:
            assert np.max(np.abs(out.rgb - (prev + F32(alpha) * (frame - prev)))) < 2e-5
            assert np.max(np.abs(out.rgb - (prev + F32(F32(1) / F32(k)) * (frame - prev)))) > 1e-3      # and not 1 / k any more
        prev = out.rgb
        hist = (out.rgb, out.depth, out.count)
    # the count saturates
    out = resolve(scene, w, h, (frames[0], dm, acc), (prev, hist[1], np.full(n, 254, np.uint8)), pose, pose)
    assert np.all(out.count == 255)
    out = resolve(scene, w, h, (frames[0], dm, acc), (prev, hist[1], np.full(n, 255, np.uint8)), pose, pose)
    assert np.all(out.count == 255)


def test_the_clamp_never_leaves_the_neighbourhood(scene):
    for (w, h) in RR.SIZES:
        for motion in ("identity", "lateral", "forward"):
            hr, hd, hc, prev = TR.history_at(scene, w, h, False, 1)
            cur = TR.current_at(scene, w, h, 1)
            dst = RR.moved(scene, **RR.MOTIONS[motion])
            alpha = 1e-6      # the output is the clamped history to rounding: hst + a (cur - hst)
            out = resolve(scene, w, h, cur, (hr * F32(7.0) - F32(3.0), None, None), dst, prev, alpha=alpha)
            lo, hi = TR.neighbourhood_bounds(cur[0], w, h)
            ok = out.accepted[:, None] & ~np.isnan(lo) & ~np.isnan(out.rgb) & ~np.isnan(cur[0])
            slack = 1e-5 * (np.abs(out.rgb) + np.abs(np.nan_to_num(cur[0])) + 1)
            assert np.all((out.rgb >= lo - slack)[ok]) and np.all((out.rgb <= hi + slack)[ok])
            assert np.count_nonzero(ok) > 0 or w * h == 1 or motion != "identity"
            free = resolve(scene, w, h, cur, (hr * F32(7.0) - F32(3.0), None, None), dst, prev, alpha=alpha, flags=0)
            if w * h > 100:
                assert np.count_nonzero(((free.rgb < lo - slack) | (free.rgb > hi + slack))[ok]) > 10      # the clamp had work to do
    # the order itself: NaNs skipped, -0 below +0, all NaN stays NaN
    a = np.array([np.nan, 0.0, -0.0, 1.0, np.nan, -2.0], F32)
    b = np.array([1.0, -0.0, 0.0, np.nan, np.nan, -3.0], F32)
    assert np.array_equal(TR.min_rule(a, b).view(np.uint32), np.array([1.0, -0.0, -0.0, 1.0, np.nan, -3.0], F32).view(np.uint32))
    assert np.array_equal(TR.max_rule(a, b).view(np.uint32), np.array([1.0, 0.0, 0.0, 1.0, np.nan, -2.0], F32).view(np.uint32))


CASES = [(w, h, name, cam) for (w, h) in RR.SIZES for name in RR.MOTIONS for cam in (False, True) if not cam or (name == "lateral" and (w, h) == RR.SIZES[0])]


@pytest.mark.parametrize("w,h,motion,camera_origin", CASES, ids=["%dx%d-%s%s" % (w, h, n, "-cf" if c else "") for w, h, n, c in CASES])
def test_inputs_keep_boundary_and_tolerance_ties_rare(scene, w, h, motion, camera_origin):
    """The input condition of the GPU tests' exact equality: float32 and float64 geometry agree on the nearest tap and on the mask of all
    but 1 % of the pixels (none, for a frame below 100 pixels), for every geometric case and both depth tolerances those tests run."""
    hr, hd, hc, prev = TR.history_at(scene, w, h, camera_origin, 1)
    cur = TR.current_at(scene, w, h, 1)
    dst = RR.moved(scene, **RR.MOTIONS[motion])
    for tol in (TR.DEPTH_TOL, 0.3):
        for depth in (hd, None):
            a = resolve(scene, w, h, cur, (hr, depth, hc), dst, prev, camera_origin, depth_tol=tol)
            b = resolve(scene, w, h, cur, (hr, depth, hc), dst, prev, camera_origin, f=TR.temporal_f64, depth_tol=tol)
            differ = [int(np.count_nonzero(a.tap != b.tap)), int(np.count_nonzero(a.mask != b.mask))]
            assert max(differ) <= (w * h) // 100, (differ, w * h)
            assert np.max(np.abs(np.nan_to_num(a.depth, posinf=0) - np.nan_to_num(b.depth, posinf=0))) < 1e-4
    if motion == "sees_none":
        assert a.rejected == w * h and np.all(a.tap == -1)


# ---- hosts ------------------------------------------------------------------------------------------

def test_cli_parses_the_taa_flags(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--taa ALPHA[:TOL]" in usage and "--taa-grid S" in usage and "cut:" in usage
    for bad in ("0", "-0.1", "1.5", "x", "0.1:", "0.1:-1", "0.1:x", ":0.1", "nan"):
        out = subprocess.run([cli, "m", "--taa", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--taa ALPHA[:TOL]: ALPHA must lie in (0, 1], TOL must be a number >= 0" in out.stdout, bad
    for bad in ("0", "9", "two", "2x"):
        out = subprocess.run([cli, "m", "--taa", "0.1", "--taa-grid", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--taa-grid S: S must be an integer in 1..8" in out.stdout, bad
    for flag in ("--taa", "--taa-grid"):
        out = subprocess.run([cli, "m", flag], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "missing value after " + flag in out.stdout
    for extra, word in ((["--reproject", "2"], "not with --reproject"), (["--supersample", "2"], "not with --supersample")):
        for order in (["--taa", "0.1:0.05"] + extra, extra + ["--taa", "0.1"]):
            out = subprocess.run([cli, "m"] + order, capture_output=True, text=True, timeout=60)
            assert out.returncode != 0 and word in out.stdout, order
    # accepted: parsing gets as far as the model directory; --reproject 1 / --supersample 1 are "off"
    for good in (["--taa", "0.1"], ["--taa", "1:0"], ["--taa", "0.25:0.05", "--taa-grid", "3", "--reproject", "1", "--supersample", "1"]):
        out = subprocess.run([cli, os.path.join(str(ROOT), "no_such_model")] + good + ["--dry-run", "--frames", "1"], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "config.ini" in out.stdout and "Argument parsing failed" not in out.stdout, good


def test_evaluator_temporal_options_and_summary_keys():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["m", "d"])
    assert a.temporal is None and a.temporal_still is None
    a = ap.parse_args(["m", "d", "--temporal", "0.2", "--temporal-still", "8"])
    assert a.temporal == 0.2 and a.temporal_still == 8
    for bad in (["--temporal", "x"], ["--temporal-still", "1.5"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["m", "d"] + bad)
    sig = inspect.signature(E.evaluate).parameters
    assert sig["temporal"].default is None and sig["temporal_still"].default is None
    for kw in (dict(temporal=0.0), dict(temporal=1.5), dict(temporal=float("nan")), dict(temporal_still=0), dict(temporal=0.1, reproject_stride=2),
               dict(temporal=0.1, supersample=2), dict(temporal_still=4, sweep_scales=[0.5])):
        with pytest.raises(ValueError):
            E.evaluate("m", "d", **kw)
    plain = [dict(frame=0, image="x", samples_per_ray=3.0, ms=1.0, mse=0.01, psnr=20.0, flip=0.1)]
    assert sorted(E.summarise(plain, True)) == ["frames", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]      # unchanged
    recs = [dict(plain[0], rejected_fraction=1.0, mse_temporal=0.01, psnr_temporal=20.0, flip_temporal=0.1),
            dict(plain[0], frame=1, rejected_fraction=0.5, mse_temporal=0.001, psnr_temporal=30.0, flip_temporal=0.3)]
    s = E.summarise(recs, True)
    assert sorted(s) == ["frames", "mean_flip", "mean_flip_temporal", "mean_ms", "mean_mse", "mean_psnr", "mean_psnr_temporal", "mean_rejected_fraction",
                         "mean_samples_per_ray"]
    assert (s["frames"], s["mean_psnr"], s["mean_psnr_temporal"], s["mean_rejected_fraction"], s["mean_flip_temporal"]) == (2, 20.0, 25.0, 0.75, 0.2)
    assert "mean_flip_temporal" not in E.summarise(recs, False)
