"""CPU-only checks of the gather reprojection (adanerf_reproject_gather): the C ABI declares and exports it without a struct change, the
hosts have their new flags and methods and keep the old ones, the restatement the GPU tests compare against
(tests/reproject_gather_reference.py) has the properties a gather warp must have, and the inputs of the GPU tests keep pixel-boundary
and tolerance ties rare enough for exact equality to be a fair demand.  What the kernels compute: tests/test_gpu_reproject_gather.py.

A finding these tests record.  On the smooth wall + box scene at depth_tol 0.02 the forward move leaves 35 mask-0 pixels of 5917 (the
splat without fill: 1033), and they are NOT at the box's outline or the frame border: all 35 are alive pixels on the wall's steepest
slope (columns 13-14 and 94-95), where the depth steps by 0.30 x 0.37 = 0.111 per column at a distance of about 4, a relative step of
0.028.  There the iteration ends in a 2-cycle between two neighbouring taps, and the estimate made from one is compared with the depth
of the other: a difference of one depth step, which a tolerance below the step cannot accept.  So a tolerance has to exceed the
relative depth step per pixel of the surfaces it is to verify; at the hosts' default (0.05 > 0.028) the forward move leaves no hole at
all.  The location property is therefore asserted at the default tolerance, and at 0.02 the count and the cause are."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import reproject_gather_reference as G
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


@pytest.fixture(scope="module")
def scene_cf():
    return load_case("classroom_coarse_fine_16_24")[2]


def warp(scene, w, h, depth, acc, dst, camera_origin=False, f=G.gather_f32, seed=1, **kw):
    sp, sr = RR.src_pose(scene)
    return f(scene, w, h, camera_origin, G.colours(w, h, seed), depth, acc, sp, sr, dst[0], dst[1], **kw)


# ---- the ABI and the hosts -------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_point(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "reproject_gather_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "reproject_gather_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "reproject_gather(NULL) rc=-1 holes=-7 abi=4 guess=1"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # no struct changed
    assert "adanerf_reproject_gather" in R.EXPORTS and hasattr(lib, "adanerf_reproject_gather") and R.GATHER_GUESS == G.GUESS == 1
    assert lib.adanerf_abi_version() == 4


def test_a_null_context_is_refused_before_any_device_work(lib):
    f3, f9 = (C.c_float * 3)(0, 0, 0), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    holes = C.c_int32(-7)
    assert lib.adanerf_reproject_gather(None, None, None, None, f3, f9, f3, f9, 0.5, 0.05, 3, 0, 1, None, None, None, None, C.byref(holes)) == -1
    assert lib.adanerf_reproject_gather(None, 4096, 4096, 4096, f3, f9, f3, f9, 0.5, 0.05, 3, 0, 0, 65536, None, None, None, None) == -1
    assert holes.value == -7


def test_cli_help_names_the_flags_and_refuses_them_without_reproject(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--reproject-warp splat|gather", "--reproject-iterations N", "--reproject-tol T", "--reproject K", "--rerender holes|unsourced"):
        assert flag in usage, flag
    for args, word in ((["--reproject-warp", "gather"], "only with --reproject K"), (["--reproject", "1", "--reproject-warp", "splat"], "only with --reproject K"),
                       (["--reproject-iterations", "2"], "only with --reproject K"), (["--reproject", "3", "--reproject-warp", "scatter"], "splat or gather"),
                       (["--reproject", "3", "--reproject-iterations", "9"], "1..8"), (["--reproject", "3", "--reproject-iterations", "0"], "1..8"),
                       (["--reproject", "3", "--reproject-tol", "-1"], ">= 0"), (["--reproject", "3", "--reproject-tol", "nan"], ">= 0"),
                       (["--reproject-warp"], "missing value after --reproject-warp")):
        out = subprocess.run([cli, "m"] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout)


def test_python_host_keeps_its_signatures_and_has_the_new_methods():
    sig = inspect.signature(R.NeuralRenderer.reproject).parameters
    assert list(sig)[1:] == ["dst_pos", "dst_rot", "fill", "acc_min"] and sig["fill"].default is True and sig["acc_min"].default == 0.5
    assert list(inspect.signature(R.NeuralRenderer.render_numpy).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.enable_reprojection).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.reproject_rerender).parameters)[1:] == ["dst_pos", "dst_rot", "rerender", "fill", "acc_min"]
    assert list(inspect.signature(R.NeuralRenderer.reproject_device).parameters)[1:11] == ["src_rgba8", "src_depth", "src_acc", "src_pos", "src_rot", "dst_pos",
                                                                                          "dst_rot", "dst_rgba8", "dst_depth", "dst_mask"]
    sig = inspect.signature(R.NeuralRenderer.reproject_gather).parameters
    assert list(sig)[1:] == ["dst_pos", "dst_rot", "iterations", "depth_tol", "guess", "acc_min"]
    assert (sig["iterations"].default, sig["depth_tol"].default, sig["guess"].default, sig["acc_min"].default) == (R.GATHER_ITERATIONS, R.GATHER_DEPTH_TOL, True, 0.5)
    assert (R.GATHER_ITERATIONS, R.GATHER_DEPTH_TOL) == (G.ITERATIONS, G.DEPTH_TOL)
    sig = inspect.signature(R.NeuralRenderer.reproject_gather_rerender).parameters
    assert list(sig)[1:4] == ["dst_pos", "dst_rot", "rerender"] and sig["rerender"].default == "holes"
    assert list(inspect.signature(R.NeuralRenderer.reproject_gather_device).parameters)[1:9] == ["src_rgb", "src_depth", "src_acc", "src_pos", "src_rot", "dst_pos",
                                                                                                "dst_rot", "dst_rgb"]


def test_evaluator_has_the_warp_option_and_keeps_its_summary_keys():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["m", "d"]).reproject_warp is None
    a = ap.parse_args(["m", "d", "--reproject-stride", "2", "--reproject-warp", "gather", "--reproject-iterations", "2", "--reproject-tol", "0.1"])
    assert (a.reproject_warp, a.reproject_iterations, a.reproject_tol) == ("gather", 2, 0.1)
    with pytest.raises(SystemExit):
        ap.parse_args(["m", "d", "--reproject-warp", "scatter"])
    sig = inspect.signature(E.evaluate).parameters
    assert sig["reproject_warp"].default == "splat" and sig["reproject_stride"].default is None
    for kw in (dict(reproject_warp="gather"), dict(reproject_stride=2, reproject_warp="scatter"), dict(reproject_iterations=2)):
        with pytest.raises(ValueError):
            E.evaluate("m", "d", **kw)
    recs = [dict(frame=0, image="x", warped=False, samples_per_ray=3.0, ms=1.0, mse=0.01, psnr=20.0),
            dict(frame=1, image="y", warped=True, warp="gather", hole_fraction=0.25, mse=0.1, psnr=10.0)]
    assert sorted(E.summarise(recs, False)) == ["frames", "mean_hole_fraction", "mean_ms", "mean_mse", "mean_psnr", "mean_psnr_rendered", "mean_psnr_warped",
                                                "mean_samples_per_ray"]


# ---- properties of the definition ------------------------------------------------------------------

@pytest.mark.parametrize("w,h", G.GPU_SIZES)
@pytest.mark.parametrize("camera_origin", [False, True])
def test_identity_pose_has_no_holes_and_every_tap_is_the_pixel_itself(scene, w, h, camera_origin):
    """also the planted far pixels: a pixel without a surface is a direction, and lands on itself"""
    _, depth, acc, _ = RR.depth_scene(w, h, 1)
    for it in (1, 3, 8):
        a = warp(scene, w, h, depth, acc, RR.src_pose(scene), camera_origin, iterations=it)
        assert a.holes == 0 and np.all(a.mask == 1) and np.array_equal(a.tap, np.arange(w * h))
        assert np.all(a.depth > 0) and np.count_nonzero(np.isinf(a.depth)) >= (w if h >= 3 else 0)      # the far row comes out at +inf
        src = G.colours(w, h, 1)      # a tap next to a pixel centre: the pixel's own colour up to the rounding of (u, vv), unless a NaN is near
        clean = np.isfinite(a.rgb).all(axis=1)
        assert np.count_nonzero(clean) > 0 and np.allclose(a.rgb[clean], src[clean], rtol=0, atol=1e-3)


def _splat_holes(scene, depth, acc, dst):
    sp, sr = RR.src_pose(scene)
    rgba = np.zeros((H, W, 4), np.uint8)
    return RR.reproject_f32(scene, W, H, False, rgba, depth, acc, sp, sr, dst[0], dst[1], flags=0)[3]


def _outline_distance(x, y, x0, x1, y0, y1):
    """Chebyshev distance of the pixels (x, y) to the outline of the rectangle of pixels x0..x1, y0..y1"""
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    din = np.minimum(np.minimum(x - x0, x1 - x), np.minimum(y - y0, y1 - y))
    dout = np.maximum(np.maximum(np.maximum(x0 - x, x - x1), 0), np.maximum(np.maximum(y0 - y, y - y1), 0))
    return np.where(inside, din, dout)


def test_forward_move_leaves_a_fraction_of_the_splats_holes(scene):
    """The forward move magnifies: the splat cracks, the gather does not.  At the hosts' tolerance (above the scene's relative depth
    step per pixel, 0.028: the module's docstring) fewer than a tenth of the splat's unfilled holes are left and none of them lies more
    than 2 px from the box's outline or the frame border; at 0.02 still fewer than a tenth, every one of them an alive pixel whose
    2-cycle the tolerance cannot accept, and ADANERF_GATHER_GUESS keeps them all."""
    _, depth, acc, is_box = RR.depth_scene(W, H, 1, planted=False)
    dst = RR.moved(scene, **RR.MOTIONS["forward"])
    splat_holes = _splat_holes(scene, depth, acc, dst)
    a = warp(scene, W, H, depth, acc, dst, iterations=3, depth_tol=G.DEPTH_TOL)
    sp, sr = RR.src_pose(scene)
    ok, pix, _, _ = RR.splat(scene, W, H, False, depth, acc, sp, sr, dst[0], dst[1], RR.ACC_MIN)
    bx, by = pix[ok & is_box] % W, pix[ok & is_box] // W      # where the box lies in the destination frame
    holes = np.flatnonzero(a.mask == 0)
    hx, hy = holes % W, holes // W
    to_outline = _outline_distance(hx, hy, bx.min(), bx.max(), by.min(), by.max())
    to_border = np.minimum(np.minimum(hx, W - 1 - hx), np.minimum(hy, H - 1 - hy))
    tight = warp(scene, W, H, depth, acc, dst, iterations=3, depth_tol=0.02)
    print("forward: splat holes %d, gather mask 0 at tol %.2f: %d, at 0.02: %d (dead %d)" % (splat_holes, G.DEPTH_TOL, a.holes, tight.holes,
                                                                                           int(np.count_nonzero(~tight.alive))))
    assert splat_holes > 500 and a.holes * 10 < splat_holes
    assert np.all(np.minimum(to_outline, to_border) <= 2)
    assert tight.holes * 10 < splat_holes and np.all(tight.alive[tight.mask == 0])
    assert warp(scene, W, H, depth, acc, dst, iterations=3, depth_tol=0.02, flags=G.GUESS).holes == 0


def test_lateral_move_opens_the_trailing_edge_band_of_the_box(scene):
    """Two shells of constant distance: the camera moves right, the picture moves left, the box by more than the wall.  Behind the box's
    trailing (right) edge a band of wall shows that the source frame never saw, as wide as the two parallaxes differ; the only other
    holes are the band at the frame's right border that the wall's own parallax uncovers."""
    _, depth, acc, is_box = RR.depth_scene(W, H, 3, planted=False)
    depth = (np.where(is_box, np.float32(1.5), np.float32(4.0)) * acc).astype(np.float32)
    right = 0.1
    dst = RR.moved(scene, right=right)
    a = warp(scene, W, H, depth, acc, dst, iterations=3, depth_tol=0.02)
    sp, sr = RR.src_pose(scene)
    _, zs = G.surfaces(scene, W, H, False, depth, acc, sp, sr, dtype=np.float64)
    focal = O.focal_from_fov(W, scene.fov)
    par_box, par_wall = focal * right / np.median(zs[is_box]), focal * right / np.median(zs[~is_box])      # px, towards the left
    want = par_box - par_wall
    x0, x1, y0, y1 = RR.box_of(W, H)
    edge = (x1 - 1) - par_box      # where the box's last column lies in the destination frame
    m = (a.mask == 0).reshape(H, W)
    border = int(np.ceil(par_wall)) + 1
    print("parallax box %.2f px, wall %.2f px, band %.2f px wide from column %.1f; holes %d" % (par_box, par_wall, want, edge, a.holes))
    assert want > 1.5
    for y in range(y0 + 1, y1 - 1):
        cols = np.flatnonzero(m[y, :W - border])
        assert cols.size and np.array_equal(cols, np.arange(cols[0], cols[0] + cols.size)), (y, cols)      # one run per row
        assert abs(cols.size - want) <= 1 and abs(cols[0] - (edge + 1)) <= 1, (y, cols)
    ys, xs = np.nonzero(m)
    in_band = (ys >= y0 - 1) & (ys <= y1) & (xs >= edge - 1) & (xs <= edge + want + 2)
    assert np.all(in_band | (xs >= W - border))      # nothing at the leading edge, nothing on the shells
    assert not np.any(a.alive[a.mask == 0] & (np.flatnonzero(a.mask == 0) % W >= W - border))      # the border band: dead, it left the source frame


def test_sees_none_makes_every_pixel_a_hole(scene):
    _, depth, acc, _ = RR.depth_scene(W, H, 1)
    for flags in (0, G.GUESS):
        a = warp(scene, W, H, depth, acc, RR.moved(scene, **RR.MOTIONS["sees_none"]), flags=flags)
        assert a.holes == W * H and np.all(a.mask == 0) and np.all(a.depth == 0) and np.all(a.rgb == 0) and not np.any(np.signbit(a.rgb))
        assert np.all(a.rgba8 == np.frombuffer(np.uint32(RR.HOLE).tobytes(), np.uint8))


@pytest.mark.parametrize("motion", ["lateral", "forward", "backward", "yaw20", "behind_part"])
def test_the_guess_flag_only_promotes_alive_holes(scene, motion):
    _, depth, acc, _ = RR.depth_scene(W, H, 1)
    dst = RR.moved(scene, **RR.MOTIONS[motion])
    bare = warp(scene, W, H, depth, acc, dst, depth_tol=0.02)
    guess = warp(scene, W, H, depth, acc, dst, depth_tol=0.02, flags=G.GUESS)
    assert np.array_equal(guess.mask == 1, bare.mask == 1)      # mask 1 is unchanged
    one = bare.mask == 1
    assert np.array_equal(guess.rgb[one].view(np.uint32), bare.rgb[one].view(np.uint32)) and np.array_equal(guess.depth[one].view(np.uint32), bare.depth[one].view(np.uint32))
    assert np.all(bare.mask[guess.mask == 2] == 0)      # every mask 2 was a hole
    # a translation has depth edges to disagree at; under a rotation alone every point stays on its source ray, and nothing is unverified
    assert (np.count_nonzero(guess.mask == 2) > 0) == (motion != "yaw20")
    assert np.array_equal(guess.mask == 0, ~guess.alive)      # what is still a hole is dead
    assert guess.holes == int(np.count_nonzero(~guess.alive)) <= bare.holes and set(np.unique(bare.mask).tolist()) <= {0, 1}


# ---- the input condition of the GPU tests' exact equality --------------------------------------------

CASES = [(w, h, name, cam) for (w, h) in G.GPU_SIZES for name in RR.MOTIONS for cam in (False, True) if not cam or (name == "lateral" and (w, h) == RR.SIZES[0])]


@pytest.mark.parametrize("w,h,motion,camera_origin", CASES, ids=["%dx%d-%s%s" % (w, h, n, "-cf" if c else "") for w, h, n, c in CASES])
def test_inputs_keep_boundary_and_tolerance_ties_rare(scene, scene_cf, w, h, motion, camera_origin):
    """float32 and float64 agree on the mask of at least 98 % of the pixels and on the final tap of at least 98 % of the pixels both
    accept, at 1 and at 3 iterations, for every (size, motion, origin) the GPU test runs -- with planted far pixels and
    ADANERF_GATHER_GUESS, as there."""
    sc = scene_cf if camera_origin else scene
    _, depth, acc, _ = RR.depth_scene(w, h, 1)
    dst = RR.moved(sc, **RR.MOTIONS[motion])
    for it in (1, 3):
        a = warp(sc, w, h, depth, acc, dst, camera_origin, iterations=it, flags=G.GUESS)
        b = warp(sc, w, h, depth, acc, dst, camera_origin, f=G.gather_f64, iterations=it, flags=G.GUESS)
        both = (a.mask > 0) & (b.mask > 0)
        assert np.mean(a.mask == b.mask) >= 0.98, (it, np.mean(a.mask == b.mask))
        assert not both.any() or np.mean(a.tap[both] == b.tap[both]) >= 0.98, (it, np.mean(a.tap[both] == b.tap[both]))
        if motion == "sees_none":
            assert a.holes == w * h
