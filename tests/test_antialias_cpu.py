"""CPU-only checks of the anti-aliasing entry points (adanerf_set_pixel_offset, adanerf_host_subpixel_grid, adanerf_accumulate /
adanerf_resolve_mean, ADANERF_PRESENT_AREA): the C ABI declares and exports them without a struct change, the restatements the GPU tests
compare against (tests/antialias_reference.py) have the properties their definitions promise, the offset ray table at offset (0, 0) is the
oracle's table bit for bit, and both hosts and the evaluator parse their new arguments.  What the kernels compute:
tests/test_gpu_antialias.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import antialias_reference as AR
import present_reference as P
import reproject_reference as RR
from conftest import ROOT, load_case

import adanerf_amd
from adanerf_amd import renderer as R

NEW = ["adanerf_set_pixel_offset", "adanerf_get_pixel_offset", "adanerf_accumulate", "adanerf_resolve_mean", "adanerf_host_subpixel_grid"]


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


@pytest.fixture(scope="module")
def scene():
    return load_case("classroom_n8_thr02")[2]


def test_header_declares_and_library_exports_the_entry_points(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "antialias_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "antialias_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "null rc=-1 -1 -1 -1 -1 out=-7 sum=0 abi=4 area=8"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # no struct changed
    assert lines[2] == "grid(2,3) 0.25 0.25"
    for name in NEW:
        assert name in R.EXPORTS and hasattr(lib, name)
    assert R.PRESENT_AREA == AR.AREA == 8 and R.PRESENT_FILTERS["area"] == 8 and lib.adanerf_abi_version() == 4


def test_null_contexts_are_refused_before_any_device_work(lib):
    out = (C.c_float * 2)(-7, -7)
    assert lib.adanerf_set_pixel_offset(None, 0.0, 0.0) == -1 and lib.adanerf_get_pixel_offset(None, out) == -1 and out[0] == -7
    assert lib.adanerf_accumulate(None, 4096, 1, 8192, 1) == -1 and lib.adanerf_resolve_mean(None, 4096, 1, 1, 8192, None) == -1
    assert lib.adanerf_present(None, 4096, 2, 2, 8192, 1, 1, R.PRESENT_AREA) == -1


# ---- the sub-pixel grid --------------------------------------------------------------------------------

def _grid(lib, s):
    out = []
    for k in range(s * s):
        dx, dy = C.c_float(-7), C.c_float(-7)
        assert lib.adanerf_host_subpixel_grid(s, k, C.byref(dx), C.byref(dy)) == 0
        out.append((dx.value, dy.value))
    return out


def test_subpixel_grid_values(lib):
    assert _grid(lib, 1) == [(0.0, 0.0)]
    assert _grid(lib, 2) == [(-0.25, -0.25), (0.25, -0.25), (-0.25, 0.25), (0.25, 0.25)]
    third = float(np.float32(1.0 / 3.0))
    assert _grid(lib, 3) == [(x, y) for y in (-third, 0.0, third) for x in (-third, 0.0, third)]
    eighth = [(2 * i + 1 - 8) / 16.0 for i in range(8)]      # sixteenths: exact in fp32
    assert _grid(lib, 8) == [(x, y) for y in eighth for x in eighth]
    for s in range(1, 9):
        g = _grid(lib, s)
        assert g == AR.subpixel_grid(s) == R.subpixel_grid(s) == R.NeuralRenderer.subpixel_grid(s)
        assert sum(np.float64(x) for x, _ in g) == 0.0 and sum(np.float64(y) for _, y in g) == 0.0      # the mean ray is the pixel centre
        assert all(abs(x) < 0.5 and abs(y) < 0.5 for x, y in g) and len(set(g)) == s * s


def test_subpixel_grid_refusals(lib):
    dx, dy = C.c_float(-7), C.c_float(-7)
    for s, k in ((0, 0), (-1, 0), (9, 0), (2, 4), (2, -1), (1, 1), (8, 64)):
        assert lib.adanerf_host_subpixel_grid(s, k, C.byref(dx), C.byref(dy)) == -1, (s, k)
    assert lib.adanerf_host_subpixel_grid(2, 0, None, C.byref(dy)) == -1 and lib.adanerf_host_subpixel_grid(2, 0, C.byref(dx), None) == -1
    assert (dx.value, dy.value) == (-7.0, -7.0)
    assert "adanerf_host_subpixel_grid" in lib.adanerf_last_error(None).decode()
    for bad in (0, 9, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            R.subpixel_grid(bad)


# ---- the area filter's definition ----------------------------------------------------------------------

def _image(w, h, seed):
    rng = np.random.default_rng(seed + 1000 * w + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    flat = img.reshape(-1)
    flat[rng.integers(0, flat.size, max(2, flat.size // 7))] = 0
    flat[rng.integers(0, flat.size, max(2, flat.size // 7))] = 255
    return img


@pytest.mark.parametrize("sw,sh,dw,dh", AR.AREA_PROPERTY_SIZES, ids=["%dx%d-%dx%d" % s for s in AR.AREA_PROPERTY_SIZES])
def test_area_reference_properties(sw, sh, dw, dh):
    for src, dst in ((sw, dw), (sh, dh)):
        wt = AR.area_weights(src, dst)
        assert np.all(wt.sum(axis=1) == src) and np.all(wt.sum(axis=0) == dst)
        first, last = AR.area_taps(src, dst)
        for x in range(dst):      # the contributing pixels are exactly first..last, each with a positive weight
            nz = np.flatnonzero(wt[x])
            assert nz[0] == first[x] and nz[-1] == last[x] and nz.size == last[x] - first[x] + 1
    img = _image(sw, sh, 3)
    out = AR.area_present(img, dw, dh)
    assert out.shape == (dh, dw, 4) and out.dtype == np.uint8
    if (sw, sh) == (dw, dh):
        assert np.array_equal(out, img)      # equal sizes: the identity
    for v in (0, 1, 127, 255):               # a constant image stays constant
        assert np.all(AR.area_present(np.full((sh, sw, 4), v, np.uint8), dw, dh) == v)
    assert np.array_equal(AR.area_present(img[:, ::-1], dw, dh), out[:, ::-1])      # mirrored input, mirrored output
    assert np.array_equal(AR.area_present(img[::-1], dw, dh), out[::-1])
    assert np.array_equal(AR.area_present(img, dw, dh, flip_y=True), out[::-1])
    if (sw, sh) == (2 * dw, 2 * dh):      # an exact 2 x reduction: the half-up rounded mean of each 2 x 2 block
        blocks = img.astype(np.int64).reshape(dh, 2, dw, 2, 4).sum(axis=(1, 3))
        assert np.array_equal(out, ((blocks + 2) // 4).astype(np.uint8))


def test_area_filter_needs_at_most_nine_taps_up_to_a_ratio_of_eight():
    worst = 0
    for dst in range(1, 40):
        for src in range(1, AR.AREA_MAX_RATIO * dst + 1):
            first, last = AR.area_taps(src, dst)
            worst = max(worst, int((last - first + 1).max()))
            assert first[0] == 0 and last[-1] == src - 1 and np.all(last < src)
    assert worst == 9


def test_gpu_sizes_are_within_the_ratio_and_cover_both_directions():
    assert all(sw <= 8 * dw and sh <= 8 * dh for sw, sh, dw, dh in AR.AREA_SIZES)
    assert any(dw > sw for sw, sh, dw, dh in AR.AREA_SIZES) and any((sw, sh) == (dw, dh) for sw, sh, dw, dh in AR.AREA_SIZES)
    assert P.NEAREST == R.PRESENT_NEAREST and P.LINEAR == R.PRESENT_LINEAR and P.FLIP_Y == R.PRESENT_FLIP_Y


# ---- accumulate / resolve ------------------------------------------------------------------------------

def test_accumulate_and_resolve_reference():
    a = np.array([[0.25, -1.0, 2.0], [np.nan, np.inf, 0.999]], np.float32)
    b = np.array([[0.5, 0.5, 0.5], [1.0, -np.inf, 1e-3]], np.float32)
    s = AR.accumulate_f32(None, a, True)
    assert s.tobytes() == a.tobytes() and s is not a
    s = AR.accumulate_f32(s, b, False)
    assert s.dtype == np.float32 and s[0].tolist() == [0.75, -0.5, 2.5] and np.isnan(s[1, 0]) and np.isnan(s[1, 1])
    m, px = AR.resolve_f32(s, 2)
    assert m[0].tolist() == [0.375, -0.25, 1.25] and px[0].tolist() == [95, 0, 255, 255]      # (uchar)(0.375 * 255) = 95: truncated, not rounded
    assert px[1].tolist()[:2] == [0, 0] and px[1, 3] == 255                                    # a NaN becomes 0
    one, px1 = AR.resolve_f32(a, 1)
    assert one.tobytes() == a.tobytes() and px1[0].tolist() == [63, 0, 255, 255] and px1[1].tolist() == [0, 255, 254, 255]
    assert AR.resolve_f32(np.float32([[1.0, 1.0, 1.0]]), 65536)[0][0, 0] == np.float32(2.0 ** -16)


# ---- the offset ray table ------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", AR.RAY_SIZES + [(800, 800), (1920, 1080)], ids=lambda v: str(v))
def test_ray_table_at_offset_zero_is_the_oracle_s(scene, w, h):
    want = O.generate_ray_directions(w, h, scene.fov)
    got = AR.ray_table(w, h, scene.fov)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    if w * h <= 97 * 61:
        pos, rot = RR.src_pose(scene)
        nds, p = RR.rays_f32(scene, w, h, pos, rot)
        rays = AR.rays(scene, w, h, pos, rot)
        assert rays[:, 0:3].tobytes() == p.tobytes() and rays[:, 4:7].tobytes() == nds.tobytes() and not rays[:, [3, 7]].any()
        cam = AR.rays(scene, w, h, pos, rot, camera_origin=True)
        assert np.all(cam[:, 0:3] == np.asarray(pos, np.float32)) and cam[:, 4:7].tobytes() == nds.tobytes()


def test_ray_table_offsets_move_the_rays_as_defined(scene):
    w, h = 16, 12
    base = AR.ray_table(w, h, scene.fov).reshape(h, w, 3)
    # a whole pixel to the right is the neighbour's ray up to the rounding of start + pp: the same direction within a few ulp
    right = AR.ray_table(w, h, scene.fov, 1.0, 0.0).reshape(h, w, 3)
    assert np.allclose(right[:, :-1], base[:, 1:], rtol=0, atol=1e-6) and not np.array_equal(right, base)
    down = AR.ray_table(w, h, scene.fov, 0.0, 1.0).reshape(h, w, 3)
    assert np.allclose(down[:-1], base[1:], rtol=0, atol=1e-6)
    # positive dx: towards higher columns (camera +x), positive dy: towards higher rows (camera -y)
    q = AR.ray_table(w, h, scene.fov, 0.25, 0.25).reshape(h, w, 3)
    assert np.all(q[..., 0] > base[..., 0]) and np.all(q[..., 1] < base[..., 1])
    # a component equal to 0 leaves that axis alone: vy / vz of every ray is the centre table's (up to the rounding of the normalisation)
    only_x = AR.ray_table(w, h, scene.fov, 0.25, 0.0).reshape(h, w, 3)
    assert np.allclose(only_x[..., 1] / only_x[..., 2], base[..., 1] / base[..., 2], rtol=0, atol=1e-6) and np.all(only_x[..., 0] > base[..., 0])
    # the 2 x 2 grid's rays at w x h are the centre rays of 2w x 2h: mathematically the same directions
    fine = AR.ray_table(2 * w, 2 * h, scene.fov).reshape(2 * h, 2 * w, 3)
    for k, (dx, dy) in enumerate(AR.subpixel_grid(2)):
        sub = AR.ray_table(w, h, scene.fov, dx, dy).reshape(h, w, 3)
        assert np.allclose(sub, fine[k // 2::2, k % 2::2], rtol=0, atol=1e-6), k


def test_local_pixels_follow_the_strips():
    assert AR.local_pixels(3, 2).tolist() == [0, 1, 2, 3, 4, 5]
    assert AR.local_pixels(2, 10, strip_rows=4, world=2, rank=1).tolist() == [8, 9, 10, 11, 12, 13, 14, 15]
    assert AR.local_pixels(2, 10, strip_rows=4, world=2, rank=0).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19]


# ---- hosts ---------------------------------------------------------------------------------------------

def test_python_host_signatures():
    NR = R.NeuralRenderer
    for name in ("set_pixel_offset", "pixel_offset", "subpixel_grid", "accumulate_device", "resolve_mean_device", "render_supersampled"):
        assert name in dir(NR)
    assert list(inspect.signature(NR.set_pixel_offset).parameters) == ["self", "dx", "dy"]
    assert isinstance(NR.pixel_offset, property)
    assert list(inspect.signature(NR.accumulate_device).parameters) == ["self", "rgb", "n_rays", "sum_out", "first"]
    assert list(inspect.signature(NR.resolve_mean_device).parameters) == ["self", "sum_in", "n_rays", "frames", "rgba8_out", "rgb_out"]
    assert list(inspect.signature(NR.render_supersampled).parameters) == ["self", "s"]
    sig = inspect.signature(NR.present).parameters
    assert list(sig)[1:] == ["window_w", "window_h", "flip_y", "filter"] and sig["filter"].default is None      # unchanged
    assert list(inspect.signature(NR.render_numpy).parameters) == ["self"]


def test_cli_parses_the_new_arguments(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--supersample S" in usage and "--present-filter nearest|linear|area" in usage and "--reproject K" in usage
    for bad in ("0", "9", "-2", "two", "2x"):
        out = subprocess.run([cli, "m", "--supersample", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--supersample S: S must be an integer in 1..8" in out.stdout, bad
    for bad in ("cubic", "", "AREA"):
        out = subprocess.run([cli, "m", "--present-filter", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--present-filter must be nearest, linear or area" in out.stdout, bad
    for flag in ("--supersample", "--present-filter"):
        out = subprocess.run([cli, "m", flag], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "missing value after " + flag in out.stdout


def test_evaluator_arguments():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    a = ap.parse_args(["m", "d"])
    assert a.supersample is None and a.present_filter is None
    a = ap.parse_args(["m", "d", "--supersample", "2", "--present-filter", "area", "--sweep-scales", "2"])
    assert a.supersample == 2 and a.present_filter == "area" and a.sweep_scales == [2.0]
    for bad in (["--supersample", "0"], ["--supersample", "9"], ["--supersample", "x"], ["--present-filter", "cubic"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["m", "d"] + bad)
    with pytest.raises(SystemExit):
        E.main(["m", "d", "--supersample", "2", "--reproject-stride", "2"])
    sig = inspect.signature(E.evaluate).parameters
    assert sig["supersample"].default is None and sig["present_filter"].default is None
    for kw in (dict(supersample=0), dict(supersample=9), dict(supersample=2, reproject_stride=2), dict(present_filter="cubic")):
        with pytest.raises(ValueError):
            E.evaluate("m", "d", **kw)
    assert "only sensible choice for scales above 1" in " ".join(ap.format_help().split())
