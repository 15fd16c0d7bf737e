"""CPU-only checks of the depth reprojection (adanerf_reproject): the C ABI declares and exports it without a struct change, the
restatement the GPU tests compare against (tests/reproject_reference.py) has the properties a warp must have on the inputs those tests
use, and those inputs keep pixel-boundary and depth ties rare enough for exact equality to be a fair demand.  What the kernels compute:
tests/test_gpu_reproject.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import reproject_reference as RR
from conftest import ROOT, load_case

import adanerf_amd
from adanerf_amd import renderer as R

W, H = RR.SIZES[0]


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


@pytest.fixture(scope="module")
def scene():
    return load_case("classroom_n8_thr02")[2]


def warp(scene, w, h, inputs, dst, camera_origin=False, flags=RR.FILL, f=RR.reproject_f32):
    rgba, depth, acc, _ = inputs
    sp, sr = RR.src_pose(scene)
    return f(scene, w, h, camera_origin, rgba, depth, acc, sp, sr, dst[0], dst[1], RR.ACC_MIN, RR.HOLE, flags)


def test_header_declares_and_library_exports_the_entry_point(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "reproject_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "reproject_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "reproject(NULL) rc=-1 holes=-7 abi=4 fill=1"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # no struct changed
    assert "adanerf_reproject" in R.EXPORTS and hasattr(lib, "adanerf_reproject") and R.REPROJECT_FILL == RR.FILL == 1
    assert lib.adanerf_abi_version() == 4


def test_a_null_context_is_refused_before_any_device_work(lib):
    f3, f9 = (C.c_float * 3)(0, 0, 0), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    holes = C.c_int32(-7)
    assert lib.adanerf_reproject(None, None, None, None, f3, f9, f3, f9, 0.5, 0, R.REPROJECT_FILL, None, None, None, C.byref(holes)) == -1
    assert lib.adanerf_reproject(None, 4096, 4096, 4096, f3, f9, f3, f9, 0.5, 0, 0, 8192, None, None, None) == -1
    assert holes.value == -7


def test_python_host_keeps_its_signatures():
    for name in ("reproject", "reproject_device", "enable_reprojection"):
        assert name in dir(R.NeuralRenderer)
    sig = inspect.signature(R.NeuralRenderer.reproject).parameters
    assert list(sig)[1:] == ["dst_pos", "dst_rot", "fill", "acc_min"] and sig["fill"].default is True and sig["acc_min"].default == 0.5
    assert list(inspect.signature(R.NeuralRenderer.render_numpy).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.set_camera).parameters) == ["self", "pos", "rot_c2w"]


# ---- properties of the definition ------------------------------------------------------------------

@pytest.mark.parametrize("w,h", RR.SIZES)
@pytest.mark.parametrize("camera_origin", [False, True])
def test_identity_pose_returns_the_frame(scene, w, h, camera_origin):
    """also the planted far pixels: a pixel without a surface is a direction, and lands on itself"""
    inputs = RR.depth_scene(w, h, 1)
    for flags in (0, RR.FILL):
        colour, depth, mask, holes, winner = warp(scene, w, h, inputs, RR.src_pose(scene), camera_origin, flags)
        assert holes == 0 and np.all(mask == 1) and np.array_equal(winner, np.arange(w * h))
        assert np.array_equal(colour, inputs[0].reshape(-1, 4))
        assert np.all(depth > 0) and np.count_nonzero(np.isinf(depth)) >= (w if h >= 3 else 0)      # the far row comes out at +inf


def test_pure_rotation_moves_far_and_near_pixels_alike(scene):
    """a near pixel's point lies on its own ray through the camera position (the sphere exit is on that ray), so under a rotation
    alone it lands where its direction lands: the two differ only where fp32 rounding crosses a pixel boundary"""
    rgba, depth, acc, _ = RR.depth_scene(W, H, 2, planted=False)
    dst = RR.moved(scene, yaw=20.0)
    near = warp(scene, W, H, (rgba, depth, acc, None), dst, flags=0)
    far = warp(scene, W, H, (rgba, depth, np.zeros_like(acc), None), dst, flags=0)
    assert np.all(np.isinf(far[1][far[2] == 1])) and np.all(np.isfinite(near[1]))
    assert np.array_equal(near[2], far[2]) and 0 < near[3] == far[3] < W * H
    sp, sr = RR.src_pose(scene)
    s_near = RR.splat(scene, W, H, False, depth, acc, sp, sr, dst[0], dst[1], RR.ACC_MIN)
    s_far = RR.splat(scene, W, H, False, depth, np.zeros_like(acc), sp, sr, dst[0], dst[1], RR.ACC_MIN)
    assert np.all(s_near[3]) and not np.any(s_far[3])
    assert np.mean(s_near[1] == s_far[1]) >= 0.999      # every source pixel lands where its direction lands
    # where two source pixels share a destination the near frame keeps the nearer, the far frame the lower index: winners may differ there only
    alone = np.bincount(s_near[1][s_near[0]], minlength=W * H) == 1
    assert np.mean(near[4][alone] == far[4][alone]) >= 0.999 and np.count_nonzero(alone) > W * H // 2
    # the picture moved: a 20 degree turn to the left of a ~65 degree field of view shifts it by about a third of the width
    row = (H // 2) * W
    src_cols = near[4][row:row + W][near[2][row:row + W] == 1] % W
    dst_cols = np.flatnonzero(near[2][row:row + W] == 1)
    assert np.all(dst_cols - src_cols > W // 5) and np.all(dst_cols - src_cols < W // 2)


def test_lateral_move_opens_holes_behind_the_box_and_the_fill_takes_the_wall(scene):
    rgba, depth, acc, is_box = RR.depth_scene(W, H, 3, planted=False)
    depth = (np.where(is_box, np.float32(1.5), np.float32(4.0)) * acc).astype(np.float32)      # two shells of constant distance: no cracks of their own
    rgba.reshape(-1, 4)[is_box] = (255, 0, 0, 255)       # red box in front of a blue wall
    rgba.reshape(-1, 4)[~is_box] = (0, 0, 255, 255)
    dst = RR.moved(scene, right=0.04)                    # about 2 px of parallax for the box, 0.8 px for the wall
    inputs = (rgba, depth, acc, is_box)
    bare = warp(scene, W, H, inputs, dst, flags=0)
    filled = warp(scene, W, H, inputs, dst, flags=RR.FILL)
    x0, x1, y0, y1 = RR.box_of(W, H)
    holes = np.flatnonzero(bare[2] == 0)
    rows = (holes // W > y0) & (holes // W < y1 - 1)
    # the camera moved right, the box moved left in the picture: its trailing side is the right one
    inner = holes[rows & (np.abs(holes % W - (x1 - 2)) <= 2)]
    leading = holes[rows & (np.abs(holes % W - (x0 - 2)) <= 2)]
    print("holes %d, at the trailing edge %d, at the leading edge %d, box rows %d" % (holes.size, inner.size, leading.size, y1 - y0 - 2))
    assert np.unique(inner // W).size >= (y1 - y0 - 2) * 3 // 4 and leading.size <= inner.size // 4
    assert np.all(bare[0][holes] == np.frombuffer(np.uint32(RR.HOLE).tobytes(), np.uint8)) and np.all(bare[1][holes] == 0)
    # on the leading side the box covers wall pixels: where both land in one pixel the box is in front
    sp, sr = RR.src_pose(scene)
    ok, pix, zc, near = RR.splat(scene, W, H, False, depth, acc, sp, sr, dst[0], dst[1], RR.ACC_MIN)
    both = np.zeros(W * H, int)
    np.add.at(both, pix[ok], np.where(is_box[ok], 1, 1000))
    mixed = np.flatnonzero((both % 1000 > 0) & (both >= 1000))
    assert mixed.size >= (y1 - y0) // 2 and np.all(is_box[bare[4][mixed]]) and np.all(mixed % W < x0 + 2)
    # with the fill: a hole next to a wall pixel takes the wall, the farther of the two surfaces beside it
    wall_won = np.zeros((H + 2, W + 2), bool)
    wall_won[1:-1, 1:-1] = ((bare[4] >= 0) & ~is_box[np.maximum(bare[4], 0)]).reshape(H, W)
    beside_wall = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            beside_wall |= wall_won[dy:dy + H, dx:dx + W]
    took = inner[beside_wall.reshape(-1)[inner]]
    assert took.size >= (y1 - y0) // 2
    assert np.all(filled[2][took] == 2) and np.all(filled[0][took] == (0, 0, 255, 255)) and np.all(filled[1][took] > 3.0)
    assert filled[3] <= bare[3] - took.size and np.array_equal(filled[4], bare[4])
    assert np.array_equal(filled[0][bare[2] == 1], bare[0][bare[2] == 1])      # the fill touches holes only


def test_backward_move_makes_collisions_and_the_nearer_source_wins(scene):
    inputs = RR.depth_scene(W, H, 4, planted=False)
    dst = RR.moved(scene, forward=-0.3)
    sp, sr = RR.src_pose(scene)
    ok, pix, zc, near = RR.splat(scene, W, H, False, inputs[1], inputs[2], sp, sr, dst[0], dst[1], RR.ACC_MIN)
    colour, depth, mask, holes, winner = warp(scene, W, H, inputs, dst, flags=0)
    landed = np.flatnonzero(ok)
    assert landed.size - np.unique(pix[landed]).size > W      # many source pixels share a destination
    nearest = np.full(W * H, np.inf, np.float32)
    np.minimum.at(nearest, pix[landed], zc[landed])
    won = winner >= 0
    assert np.array_equal(won, np.isfinite(nearest)) and np.array_equal(depth[won], nearest[won])
    assert np.array_equal(pix[winner[won]], np.flatnonzero(won))


CASES = [(w, h, name, cam) for (w, h) in RR.SIZES for name in RR.MOTIONS for cam in (False, True) if not cam or (name == "lateral" and (w, h) == RR.SIZES[0])]


@pytest.mark.parametrize("w,h,motion,camera_origin", CASES, ids=["%dx%d-%s%s" % (w, h, n, "-cf" if c else "") for w, h, n, c in CASES])
def test_inputs_keep_boundary_and_depth_ties_rare(scene, w, h, motion, camera_origin):
    """The input condition of the GPU tests' exact equality: float32 and float64 geometry agree on the winning source pixel of at least
    98 % of the destination pixels, for every geometric case those tests run."""
    inputs = RR.depth_scene(w, h, 1)
    dst = RR.moved(scene, **RR.MOTIONS[motion])
    a = warp(scene, w, h, inputs, dst, camera_origin)
    b = warp(scene, w, h, inputs, dst, camera_origin, f=RR.reproject_f64)
    assert np.mean(a[4] == b[4]) >= 0.98, (np.mean(a[4] == b[4]), a[3], b[3])
    assert np.mean(a[2] == b[2]) >= 0.98
    if motion == "sees_none":
        assert a[3] == w * h and np.all(a[2] == 0)
    if motion == "behind_part" and w * h > 100:
        ok = RR.splat(scene, w, h, camera_origin, inputs[1], inputs[2], *RR.src_pose(scene), dst[0], dst[1], RR.ACC_MIN)
        assert np.count_nonzero(~(ok[2] > 0)) > w      # part of the scene is behind the destination camera


# ---- hosts ------------------------------------------------------------------------------------------

def test_cli_parses_the_reproject_flag(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--reproject K" in usage
    for bad in ("0", "-2", "two", "3x"):
        out = subprocess.run([cli, "m", "--reproject", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--reproject K: K must be an integer >= 1" in out.stdout, bad
    out = subprocess.run([cli, "m", "--reproject"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "missing value after --reproject" in out.stdout


def test_evaluator_stride_option_and_summary_keys():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["m", "d"]).reproject_stride is None
    assert ap.parse_args(["m", "d", "--reproject-stride", "3"]).reproject_stride == 3
    with pytest.raises(SystemExit):
        ap.parse_args(["m", "d", "--reproject-stride", "x"])
    sig = inspect.signature(E.evaluate).parameters
    assert sig["reproject_stride"].default is None
    for kw in (dict(reproject_stride=0), dict(reproject_stride=2, sweep_scales=[0.5])):
        with pytest.raises(ValueError):
            E.evaluate("m", "d", **kw)
    plain = [dict(frame=0, image="x", samples_per_ray=3.0, ms=1.0, mse=0.01, psnr=20.0, flip=0.1)]
    assert sorted(E.summarise(plain, True)) == ["frames", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]      # unchanged
    recs = [dict(plain[0], warped=False), dict(frame=1, image="y", warped=True, hole_fraction=0.25, mse=0.1, psnr=10.0, flip=0.3),
            dict(frame=2, image="z", warped=True, hole_fraction=0.75, mse=0.1, psnr=14.0, flip=0.5)]
    s = E.summarise(recs, True)
    assert sorted(s) == ["frames", "mean_flip", "mean_flip_rendered", "mean_flip_warped", "mean_hole_fraction", "mean_ms", "mean_mse", "mean_psnr",
                         "mean_psnr_rendered", "mean_psnr_warped", "mean_samples_per_ray"]
    assert (s["frames"], s["mean_psnr_rendered"], s["mean_psnr_warped"], s["mean_hole_fraction"]) == (3, 20.0, 12.0, 0.5)
    assert (s["mean_samples_per_ray"], s["mean_ms"], s["mean_flip_rendered"], s["mean_flip_warped"]) == (3.0, 1.0, 0.1, 0.4)
    assert "mean_flip_warped" not in E.summarise(recs, False)
