"""CPU-only checks of temporal upsampling (adanerf_temporal_upsample): the C ABI declares and exports it without a struct change, both hosts
and the evaluator expose it, the restatement the GPU tests compare against (tests/upsample_reference.py) has the properties the stage must
have, and the inputs of those tests keep rounding ties rare enough for exact equality to be a fair demand while every moved case both
accepts and rejects.  What the kernels compute: tests/test_gpu_upsample.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import antialias_reference as AR
import reproject_reference as RR
import temporal_reference as TR
import upsample_reference as UR
from conftest import ROOT, load_case

import adanerf_amd
from adanerf_amd import renderer as R

F32 = np.float32


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
    exe = str(tmp_path / "upsample_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "upsample_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "temporal_upsample(NULL) rc=-1 rejected=-7 abi=4 clamp=1"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # no struct changed
    assert "adanerf_temporal_upsample" in R.EXPORTS and hasattr(lib, "adanerf_temporal_upsample")
    assert lib.adanerf_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    assert " *   adanerf_temporal_upsample            none: the viewer blits the frame it rendered" in header      # the table of replaced calls


def test_a_null_context_is_refused_before_any_device_work(lib):
    f3, f9 = (C.c_float * 3)(0, 0, 0), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    rejected = C.c_int32(-7)
    assert lib.adanerf_temporal_upsample(None, 2, None, None, None, 0.25, -0.25, f3, f9, None, None, None, f3, f9, 0.1, 0.02, 0.5, R.TEMPORAL_CLAMP, None, None,
                                         None, None, None, C.byref(rejected)) == -1
    assert lib.adanerf_temporal_upsample(None, 2, 4096, 4096, 4096, 0.0, 0.0, f3, f9, 8192, 8192, 8192, f3, f9, 0.1, 0.02, 0.5, 0, 16384, None, None, None, None,
                                         None) == -1
    assert rejected.value == -7


def test_python_host_signatures():
    for name in ("enable_temporal_upsample", "render_upsampled", "reset_upsample", "temporal_upsample_device"):
        assert name in dir(R.NeuralRenderer)
    sig = inspect.signature(R.NeuralRenderer.enable_temporal_upsample).parameters
    assert list(sig)[1:] == ["scale", "alpha", "depth_tol", "clamp"]
    assert (sig["scale"].default, sig["alpha"].default, sig["depth_tol"].default, sig["clamp"].default) == (2, 0.1, 0.02, True)
    assert list(inspect.signature(R.NeuralRenderer.render_upsampled).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.reset_upsample).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.temporal_upsample_device).parameters)[:7] == ["self", "scale", "cur_rgb", "cur_depth", "cur_acc", "cur_dx",
                                                                                                "cur_dy"]
    # the methods it stands beside keep theirs
    assert list(inspect.signature(R.NeuralRenderer.enable_temporal).parameters)[1:] == ["alpha", "depth_tol", "clamp", "grid"]
    assert list(inspect.signature(R.NeuralRenderer.render_temporal).parameters) == ["self"]


# ---- properties of the definition ------------------------------------------------------------------

def up(scene, w, h, s, cur, offset, hist, cur_pose, prev_pose, camera_origin=False, f=UR.upsample_f32, **kw):
    return f(scene, w, h, s, camera_origin, cur[0], cur[1], cur[2], offset[0], offset[1], cur_pose[0], cur_pose[1], hist[0], hist[1], hist[2], prev_pose[0],
             prev_pose[1], **kw)


SMALL = [(w, h, s) for (w, h) in RR.SIZES for s in UR.SCALES[(w, h)] if (w, h) != (97, 61)] + [(97, 61, 2)]


@pytest.mark.parametrize("w,h,s", SMALL)
def test_no_history_gives_the_nearest_sample_image(scene, w, h, s):
    cur = UR.current_at(scene, w, h, 1)
    pose = RR.src_pose(scene)
    for offset in UR.offsets_of(s):
        for flags in (0, UR.CLAMP):
            out = up(scene, w, h, s, cur, offset, (None, None, None), pose, (None, None), flags=flags)
            i = (out.iy[:, None] * w + out.ix[None, :]).reshape(-1)
            assert np.array_equal(out.rgb.view(np.uint32), cur[0][i].view(np.uint32))      # the bits, NaNs and signed zeros included
            assert np.all(out.mask == 0) and out.rejected == s * w * s * h and np.all(out.tap == -1)
            assert np.array_equal(out.count, out.inside.astype(np.uint8))
            # the nearest sample: no other render pixel's sample is nearer the output pixel's centre, per axis, unless the clamp to the frame chose
            for n_out, n_in, d, ix in ((s * w, w, offset[0], out.ix), (s * h, h, offset[1], out.iy)):
                centre = (np.arange(n_out) + 0.5)[:, None]
                dist = np.abs((np.arange(n_in) + 0.5 + float(F32(d)))[None, :] * s - centre)
                assert np.all(dist[np.arange(n_out), ix] <= dist.min(axis=1) + 1e-4)


@pytest.mark.parametrize("w,h,s", SMALL)
@pytest.mark.parametrize("camera_origin", [False, True])
def test_identity_pose_with_constant_images_gives_the_constant(scene, w, h, s, camera_origin):
    n, N = w * h, s * w * s * h
    _, dm, acc, _ = RR.depth_scene(w, h, 1, planted=False)
    pose = RR.src_pose(scene)
    const = np.full((n, 3), F32(0.3), F32) * F32([1.0, 2.0, -1.0])
    grid = AR.subpixel_grid(s)
    first = up(scene, w, h, s, (const, dm, acc), grid[0], (None, None, None), pose, (None, None), camera_origin)
    for flags in (0, UR.CLAMP):
        for count in (None, first.count):
            for depth in (None, first.depth):
                out = up(scene, w, h, s, (const, dm, acc), grid[-1], (first.rgb, depth, count), pose, pose, camera_origin, flags=flags)
                assert np.array_equal(out.rgb, np.broadcast_to(const[0], (N, 3)))      # c + wx (c - c), c + a (c - c) and the copies are c
                if depth is None:
                    assert out.rejected == 0 and np.array_equal(out.tap, np.arange(N))
    again = up(scene, w, h, s, (const, dm, acc), grid[0], (first.rgb, first.depth, first.count), pose, pose, camera_origin)
    assert np.array_equal(again.depth.view(np.uint32), first.depth.view(np.uint32))      # the own depth does not depend on the history


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_every_output_pixel_is_hit_exactly_once_per_grid_cycle(s):
    """with the offsets of the s x s grid every output pixel has `inside` true in exactly one frame of the cycle, its sample at the pixel's
    centre to rounding; float32 and float64 agree on the render pixel everywhere, also for 800 random offsets"""
    rng = np.random.default_rng(5)
    for n in (1, 5, 16, 97):
        hits = np.zeros(s * n, int)
        for k in range(s):      # the grid's offsets along one axis
            d = AR.subpixel_grid(s)[k][0]
            ix, e = UR.nearest_sample(s * n, s, d, n)
            ix64, e64 = UR.nearest_sample(s * n, s, d, n, np.float64)
            assert np.array_equal(ix, ix64)
            inside = np.abs(e) <= F32(0.5)
            assert np.all(np.abs(e[inside]) < 1e-4) and np.array_equal(inside, np.abs(e64) <= 0.5)
            hits += inside
        assert np.all(hits == 1)
        for d in rng.uniform(-1, 1, 200):
            assert np.array_equal(UR.nearest_sample(s * n, s, d, n)[0], UR.nearest_sample(s * n, s, d, n, np.float64)[0])


# 4 x the largest |restatement - exact interleave| measured on the 16 x 12 frame below (0, 6.4e-6, 3.3e-5, 1.1e-4 for s = 1 .. 4)
INTERLEAVE_BOUND = {1: 0.0, 2: 2.6e-5, 3: 1.4e-4, 4: 4.5e-4}


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_at_rest_a_cycle_rebuilds_the_interleave_of_its_renders(scene, s):
    """At rest from a cut, after s^2 calls every count is 1 and the image is the interleave of the s^2 renders: output pixel J holds the
    sample of the frame in which it was `inside`.  Equal to INTERLEAVE_BOUND[s], for colours in [0, 1): a pixel that holds its own sample
    takes, in every later frame of the cycle, a share k = (1 - |ex|)(1 - |ey|) of a neighbour's sample, and k is 0 only to the rounding of
    ex (the sample sits a whole output pixel away to rounding); and its history comes back through four bilinear taps whose weights are 0
    or 1 only to the rounding of the projection (some 1e-5 of a pixel at this size).  Both are rounding shares of a neighbour's value, they
    add up over the s^2 - 1 later frames, and they grow with the frame's width (the ulp of u).  The bound is 4 x what the restatement
    itself shows against the exact interleave on this frame, the margin because the share depends on the colours drawn."""
    w, h = RR.SIZES[1]
    W, H = s * w, s * h
    _, dm, acc, _ = RR.depth_scene(w, h, 1, planted=False)
    pose = RR.src_pose(scene)
    rng = np.random.default_rng(7)
    exact, hits = np.zeros((H * W, 3), F32), np.zeros(H * W, int)
    hist = (None, None, None)
    for k, offset in enumerate(AR.subpixel_grid(s)):
        frame = rng.random((w * h, 3)).astype(F32)
        out = up(scene, w, h, s, (frame, dm, acc), offset, (hist[0], None, hist[2]), pose, pose if k else (None, None), flags=0)      # no history depth at rest, as the hosts
        assert out.rejected == (W * H if k == 0 else 0)
        hist = (out.rgb, out.depth, out.count)
        i = (out.iy[:, None] * w + out.ix[None, :]).reshape(-1)
        exact[out.inside] = frame[i[out.inside]]
        hits += out.inside
        assert np.array_equal(out.count, np.minimum(hits, 1).astype(np.uint8))      # 0: a placeholder so far
    assert np.all(hits == 1) and np.all(out.count == 1)
    err = float(np.max(np.abs(out.rgb - exact)))
    print("s = %d: largest |restatement - exact interleave| %.3g (bound %.3g)" % (s, err, INTERLEAVE_BOUND[s]))
    assert err <= INTERLEAVE_BOUND[s]


def test_with_a_count_at_rest_the_weights_are_those_of_a_running_mean(scene):
    """s = 2: an output pixel's own sample comes once per cycle of 4 frames, with weight 1, 1/2, 1/3, ...: after c cycles the pixel is the
    mean of its c own samples, until 1 / c falls below alpha.  To 1e-4: the rounding shares of the test above (under 3e-5 over 10 cycles
    on this frame, measured on the restatement), with a margin."""
    w, h = RR.SIZES[1]
    s, alpha = 2, 0.1
    N = s * w * s * h
    _, dm, acc, _ = RR.depth_scene(w, h, 1, planted=False)
    pose = RR.src_pose(scene)
    rng = np.random.default_rng(11)
    grid = AR.subpixel_grid(s)
    hist, total = (None, None, None), np.zeros((N, 3), np.float64)
    for f in range(13 * s * s):
        frame = rng.random((w * h, 3)).astype(F32)
        before = hist[0]
        out = up(scene, w, h, s, (frame, dm, acc), grid[f % 4], (hist[0], None, hist[2]), pose, pose if f else (None, None), alpha=alpha, flags=0)
        hist = (out.rgb, out.depth, out.count)
        i = (out.iy[:, None] * w + out.ix[None, :]).reshape(-1)
        own = out.inside
        c = f // 4 + 1
        assert np.all(out.count[own] == c) and set(np.unique(out.count[~own])) <= {c - 1, c}
        if c <= 10:      # 1 / c >= alpha
            total[own] += frame[i[own]]
            assert np.max(np.abs(out.rgb[own] - total[own] / c)) < 1e-4
        else:
            assert np.max(np.abs(out.rgb[own] - (before[own] + F32(alpha) * (frame[i[own]] - before[own])))) < 1e-4
            assert np.max(np.abs(out.rgb[own] - (before[own] + F32(1.0 / c) * (frame[i[own]] - before[own])))) > 1e-3      # and not 1 / c any more
        if f >= 4:
            assert np.max(np.abs(out.rgb[~own] - before[~own])) < 1e-4      # the others keep their history (in the first cycle: a placeholder)
    # the count saturates at 255, and only the pixels that hold the frame's own sample count it
    for planted in (254, 255):
        out = up(scene, w, h, s, (frame, dm, acc), grid[0], (hist[0], None, np.full(N, planted, np.uint8)), pose, pose)
        assert np.all(out.count[out.inside] == 255) and np.all(out.count[~out.inside] == planted)
    # a placeholder (count 0) is replaced, not blended: mask 2, the nearest sample's bits, count = inside
    out = up(scene, w, h, s, (frame, dm, acc), grid[0], (hist[0], None, np.zeros(N, np.uint8)), pose, pose)
    i = (out.iy[:, None] * w + out.ix[None, :]).reshape(-1)
    assert np.all(out.mask == 2) and out.rejected == 0 and np.array_equal(out.rgb.view(np.uint32), frame[i].view(np.uint32))
    assert np.array_equal(out.count, out.inside.astype(np.uint8))


def test_the_clamp_never_leaves_the_neighbourhood(scene):
    for (w, h, s) in [(16, 12, 2), (16, 12, 3), (97, 61, 2), (64, 1, 2)]:
        for motion in ("identity", "lateral", "forward"):
            hr, hd, hc, prev = UR.history_at(scene, w, h, s, False, UR.SEED)
            cur = UR.current_at(scene, w, h, UR.SEED)
            dst = RR.moved(scene, **RR.MOTIONS[motion])
            alpha = 1e-6      # the output is the clamped history to rounding: hst + k a (cur - hst)
            wild = hr * F32(7.0) - F32(3.0)
            out = up(scene, w, h, s, cur, (0.25, -0.25), (wild, None, None), dst, prev, alpha=alpha)
            i = (out.iy[:, None] * w + out.ix[None, :]).reshape(-1)
            lo, hi = TR.neighbourhood_bounds(cur[0], w, h)
            lo, hi, centre = lo[i], hi[i], cur[0][i]
            ok = out.accepted[:, None] & ~np.isnan(lo) & ~np.isnan(out.rgb) & ~np.isnan(centre)
            slack = 1e-5 * (np.abs(out.rgb) + np.abs(np.nan_to_num(centre)) + 1)
            assert np.all((out.rgb >= lo - slack)[ok]) and np.all((out.rgb <= hi + slack)[ok])
            assert np.count_nonzero(ok) > 0
            free = up(scene, w, h, s, cur, (0.25, -0.25), (wild, None, None), dst, prev, alpha=alpha, flags=0)
            if s * w * s * h > 200:
                assert np.count_nonzero(((free.rgb < lo - slack) | (free.rgb > hi + slack))[ok]) > 10      # the clamp had work to do


CASES = [(w, h, s, cam) for (w, h) in RR.SIZES for s in UR.SCALES[(w, h)] for cam in (False, True) if not cam or (w, h, s) == (16, 12, 2)]


@pytest.mark.parametrize("w,h,s,camera_origin", CASES, ids=["%dx%d_x%d%s" % (w, h, s, "-cf" if c else "") for w, h, s, c in CASES])
def test_inputs_keep_ties_rare_and_every_moved_case_accepts_and_rejects(scene, w, h, s, camera_origin):
    """The input conditions of the GPU tests' exact equality, on every geometric case they run (UR.geometric_cases) at their tolerance:
    float32 and float64 agree on the render pixel (ix / iy) everywhere and on the nearest tap and the mask of all but 1 % of the pixels
    (none, for a frame below 100 pixels); and every moved case with the depth test on, on a frame of at least 100 output pixels, except
    sees_none, has at least 5 % of its pixels accepted and at least 5 % rejected -- the equality is about both branches."""
    N = s * w * s * h
    hr, hd, hc, prev = UR.history_at(scene, w, h, s, camera_origin, UR.SEED)
    cur = UR.current_at(scene, w, h, UR.SEED)
    seen = set()
    for motion, offset, with_depth, with_count, clamp in UR.geometric_cases(s):
        key = (motion, offset, with_depth, with_count)      # the clamp changes no tap and no mask
        if key in seen:
            continue
        seen.add(key)
        dst = RR.moved(scene, **RR.MOTIONS[motion])
        hist = (hr, hd if with_depth else None, hc if with_count else None)
        a = up(scene, w, h, s, cur, offset, hist, dst, prev, camera_origin, depth_tol=UR.TEST_TOL)
        b = up(scene, w, h, s, cur, offset, hist, dst, prev, camera_origin, f=UR.upsample_f64, depth_tol=UR.TEST_TOL)
        assert np.array_equal(a.ix, b.ix) and np.array_equal(a.iy, b.iy)
        differ = [int(np.count_nonzero(a.tap != b.tap)), int(np.count_nonzero(a.mask != b.mask))]
        assert max(differ) <= N // 100, (key, differ, N)
        assert np.max(np.abs(np.nan_to_num(a.depth, posinf=0) - np.nan_to_num(b.depth, posinf=0))) < 1e-4
        if motion == "sees_none":
            assert a.rejected == N and np.all(a.tap == -1)
        elif motion != "identity" and with_depth and N >= 100 and not camera_origin:
            accepted, rejected = int(np.count_nonzero(a.accepted)), a.rejected
            assert 20 * accepted >= N and 20 * rejected >= N, (key, accepted, rejected, N)


# ---- hosts ------------------------------------------------------------------------------------------

def test_cli_parses_the_taau_flag(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--taau S[:ALPHA[:TOL]]" in usage and "cut: --taa / --taau" in usage
    for bad in ("0", "5", "-1", "x", "2:", "2:0", "2:1.5", "2:x", "2:0.1:", "2:0.1:-1", "2:0.1:x", ":0.1", "2.5", "2:0.1:0.02:3", "2:nan"):
        out = subprocess.run([cli, "m", "--taau", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--taau S[:ALPHA[:TOL]]: S must be an integer in 1..4, ALPHA must lie in (0, 1], TOL must be a number >= 0" in out.stdout, bad
    out = subprocess.run([cli, "m", "--taau"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "missing value after --taau" in out.stdout
    for extra, word in ((["--taa", "0.1"], "not with --taa"), (["--reproject", "2"], "not with --reproject"), (["--supersample", "2"], "not with --supersample"),
                        (["--gpus", "2"], "use it with --gpus 1"), (["--oracle"], "not with --oracle")):
        for order in (["--taau", "2:0.1:0.05"] + extra, extra + ["--taau", "3"]):
            out = subprocess.run([cli, "m"] + order, capture_output=True, text=True, timeout=60)
            assert out.returncode != 0 and "--taau" in out.stdout and word in out.stdout, order
    # accepted: parsing gets as far as the model directory; --reproject 1 / --supersample 1 / --gpus 1 are "off"
    for good in (["--taau", "2"], ["--taau", "1:1:0"], ["--taau", "4:0.25"], ["--taau", "3:0.25:0.05", "--reproject", "1", "--supersample", "1", "--gpus", "1"]):
        out = subprocess.run([cli, os.path.join(str(ROOT), "no_such_model")] + good + ["--dry-run", "--frames", "1"], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "config.ini" in out.stdout and "Argument parsing failed" not in out.stdout, good


def test_evaluator_upsample_options_and_summary_keys():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["m", "d"])
    assert a.temporal_upsample is None and a.temporal_upsample_frames is None
    a = ap.parse_args(["m", "d", "--temporal-upsample", "2", "--temporal-upsample-frames", "8"])
    assert a.temporal_upsample == 2 and a.temporal_upsample_frames == 8
    for bad in (["--temporal-upsample", "x"], ["--temporal-upsample", "5"], ["--temporal-upsample", "0"], ["--temporal-upsample-frames", "1.5"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["m", "d"] + bad)
    sig = inspect.signature(E.evaluate).parameters
    assert sig["temporal_upsample"].default is None and sig["temporal_upsample_frames"].default is None
    for kw in (dict(temporal_upsample=0), dict(temporal_upsample=5), dict(temporal_upsample=2.5), dict(temporal_upsample=2, temporal_upsample_frames=0),
               dict(temporal_upsample_frames=4), dict(temporal_upsample=2, temporal=0.1), dict(temporal_upsample=2, temporal_still=3),
               dict(temporal_upsample=2, reproject_stride=2), dict(temporal_upsample=2, supersample=2), dict(temporal_upsample=2, sweep_scales=[0.5])):
        with pytest.raises(ValueError):
            E.evaluate("m", "d", **kw)
    plain = [dict(frame=0, image="x", samples_per_ray=3.0, ms=1.0, mse=0.01, psnr=20.0, flip=0.1)]
    assert sorted(E.summarise(plain, True)) == ["frames", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]      # unchanged
    temporal = [dict(plain[0], rejected_fraction=1.0, mse_temporal=0.01, psnr_temporal=20.0, flip_temporal=0.1)]
    assert sorted(E.summarise(temporal, True)) == ["frames", "mean_flip", "mean_flip_temporal", "mean_ms", "mean_mse", "mean_psnr", "mean_psnr_temporal",
                                                   "mean_rejected_fraction", "mean_samples_per_ray"]      # unchanged
    recs = [dict(plain[0], temporal_upsample=2, rejected_fraction=0.0, mse_upsampled=0.01, psnr_upsampled=20.0, flip_upsampled=0.1),
            dict(plain[0], frame=1, temporal_upsample=2, rejected_fraction=0.5, mse_upsampled=0.001, psnr_upsampled=30.0, flip_upsampled=0.3)]
    s = E.summarise(recs, True)
    assert sorted(s) == ["frames", "mean_flip", "mean_flip_upsampled", "mean_ms", "mean_mse", "mean_psnr", "mean_psnr_upsampled", "mean_rejected_fraction",
                         "mean_samples_per_ray"]
    assert (s["frames"], s["mean_psnr"], s["mean_psnr_upsampled"], s["mean_rejected_fraction"], s["mean_flip_upsampled"]) == (2, 20.0, 25.0, 0.25, 0.2)
    assert "mean_flip_upsampled" not in E.summarise(recs, False)


def test_evaluator_refuses_a_scale_that_does_not_divide_the_dataset(tmp_path):
    """12 x 10 at S = 4: ValueError before any context is made"""
    import json
    from adanerf_amd import evaluate as E
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    m = np.eye(4, dtype=np.float32)
    json.dump(dict(resolution=[12, 10], camera_angle_x=0.8, view_cell_center=[0, 0, 0], view_cell_size=[1, 1, 1], flip_depth=False,
                   depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    json.dump(dict(frames=[dict(file_path="./test/00000", transform_matrix=m.tolist())]), open(ds / "transforms_test.json", "w"))
    with pytest.raises(ValueError, match="does not divide"):
        E.evaluate(str(tmp_path / "no_model"), str(ds), temporal_upsample=4)
