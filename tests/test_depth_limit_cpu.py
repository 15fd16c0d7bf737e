"""CPU-only checks of hybrid rendering (adanerf_set_depth_limit / adanerf_compact_depth_limit / adanerf_blend_behind /
adanerf_host_sphere_zc): the host-side sphere occluder against the float64 restatement of tests/depth_limit_reference.py, bit for bit;
every ADANERF_EINVAL case of it; the C ABI declares and exports the four calls and the Python host binds them.  What it renders:
tests/test_gpu_depth_limit.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import depth_limit_reference as D
from conftest import ROOT

import adanerf_amd
from adanerf_amd import renderer as R

F32 = np.float32
EINVAL = -1
NAMES = ("adanerf_set_depth_limit", "adanerf_compact_depth_limit", "adanerf_blend_behind", "adanerf_host_sphere_zc")


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


POS = np.array([0.783, -3.19, 1.39], F32)
ROT = O.camera_rotation(100.0, -12.5)
FRAMES = ((1, 1, 1.7), (97, 61, 71.3), (16, 8, 9.25))


def _ahead(dist, right=0.0, up=0.0):
    """a point `dist` along the viewing axis of (POS, ROT), `right` / `up` off it"""
    r = ROT.astype(np.float64)
    return (POS.astype(np.float64) + right * r[:, 0] + up * r[:, 1] - dist * r[:, 2]).astype(F32)


# name -> (centre, radius): the camera outside the sphere, inside it, the sphere behind the camera, a ray through the centre, and spheres
# whose silhouette crosses the frame (grazing rays: hits and misses side by side)
SPHERES = {
    "outside": (_ahead(4.0, 0.3, -0.2), 1.25),
    "inside": (_ahead(0.5, 0.1, 0.1), 3.0),
    "behind": (_ahead(-4.0, 0.2, 0.1), 1.5),
    "through_the_centre": (_ahead(5.0), 0.75),
    "grazing_small": (_ahead(6.0, 0.5, 0.25), 0.4),
    "grazing_wide": (_ahead(2.0, -1.0, 0.5), 1.3),
    "touching_the_camera_plane": (_ahead(1.0, 0.0, 0.0), 1.001),
}


@pytest.mark.parametrize("name", sorted(SPHERES))
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f[:2])
def test_sphere_zc_equals_the_float64_restatement_bit_for_bit(lib, frame, name):
    w, h, focal = frame
    center, radius = SPHERES[name]
    want, disc = D.sphere(w, h, focal, POS, ROT, center, radius)
    # hit or miss must not hang on the discriminant's last bit
    assert (np.abs(disc) > 1e-9).all(), (name, float(np.abs(disc).min()))
    got = R.sphere_zc(w, h, focal, POS, ROT, center, radius)
    assert got.dtype == F32 and got.shape == (w * h,)
    assert got.tobytes() == want.tobytes(), (name, frame)
    hit = np.isfinite(want)
    if name == "behind":
        assert not hit.any()
    if name == "inside":
        assert hit.all() and (want > 0).all()
    if name in ("outside", "through_the_centre"):
        assert hit.any() and (want[hit] > 0).all()
    if name == "through_the_centre" and w % 2 == 1 and h % 2 == 1:      # the centre pixel looks straight down the axis: zc = distance - radius
        mid = (h // 2) * w + w // 2
        assert abs(float(want[mid]) - (5.0 - 0.75)) < 1e-5
    if name.startswith("grazing") and w * h > 1000:
        assert hit.any() and (~hit).any()


def test_sphere_zc_orders_its_roots_and_misses(lib):
    """the smallest positive root: the near surface from outside, the far one from inside; nothing behind the camera"""
    eye = np.eye(3, dtype=F32)
    zero = np.zeros(3, F32)
    assert R.sphere_zc(1, 1, 10.0, zero, eye, [0, 0, -3], 1.0)[0] == F32(2.0)
    assert R.sphere_zc(1, 1, 10.0, zero, eye, [0, 0, 0], 1.0)[0] == F32(1.0)
    assert R.sphere_zc(1, 1, 10.0, zero, eye, [0, 0, 3], 1.0)[0] == F32(np.inf)
    assert R.sphere_zc(1, 1, 10.0, zero, eye, [5, 0, -3], 1.0)[0] == F32(np.inf)


def test_sphere_zc_refuses_what_the_header_lists(lib):
    fp = C.POINTER(C.c_float)
    out = np.full(16 * 8 + 8, -7.0, F32)

    def call(w=16, h=8, focal=9.25, pos=POS, rot=ROT, center=SPHERES["outside"][0], radius=1.25, dst=out):
        arr = [None if a is None else np.ascontiguousarray(a, F32).reshape(-1) for a in (pos, rot, center)]
        ptr = [None if a is None else a.ctypes.data_as(fp) for a in arr]
        return lib.adanerf_host_sphere_zc(w, h, focal, ptr[0], ptr[1], ptr[2], radius, None if dst is None else dst.ctypes.data_as(fp))

    bad3 = lambda v, i: np.where(np.arange(3) == i, F32(v), POS).astype(F32)
    bad9 = lambda v, i: np.where(np.arange(9) == i, F32(v), ROT.reshape(-1)).astype(F32)
    cases = [dict(pos=None), dict(rot=None), dict(center=None), dict(dst=None), dict(w=0), dict(h=0), dict(w=-3), dict(w=16385), dict(h=16385),
             dict(focal=float("nan")), dict(focal=float("inf")), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=0.0),
             dict(radius=-1.0), dict(pos=bad3(np.nan, 1)), dict(pos=bad3(np.inf, 2)), dict(center=bad3(-np.inf, 0)), dict(center=bad3(np.nan, 2)),
             dict(rot=bad9(np.nan, 4)), dict(rot=bad9(np.inf, 8))]
    for kw in cases:
        assert call(**kw) == EINVAL, kw
    assert (out == F32(-7.0)).all()      # nothing written by a refused call
    assert call() == 0
    assert (out[16 * 8:] == F32(-7.0)).all() and out[:16 * 8].tobytes() == D.sphere(16, 8, 9.25, POS, ROT, *SPHERES["outside"])[0].tobytes()
    assert call(w=16384, h=1, dst=np.empty(16384, F32)) == 0
    with pytest.raises(ValueError):
        R.sphere_zc(0, 8, 9.25, POS, ROT, [0, 0, 0], 1.0)
    with pytest.raises(ValueError):
        R.sphere_zc(16, 8, 9.25, POS, ROT, [0, 0, 0], 0.0)


def test_reference_trim_and_blend_follow_the_stated_rule():
    """the restatement itself on hand-made numbers: equality drops, a NaN on either side keeps, rows may empty; the blend's branches"""
    ztab = np.arange(128, dtype=F32)
    rays = np.zeros((3, 8), F32)
    rays[:, 6] = -1.0      # looking down -z from the origin: zc = z
    bins = np.array([[2, 5, 9], [2, 5, 9], [2, 5, -1]], np.int16)
    wts = np.array([[.1, .2, .3], [.4, .5, .6], [.7, .8, 0]], F32)
    zc = D.sample_zc(rays, ztab, bins, np.zeros(3, F32), np.eye(3, dtype=F32))
    assert np.array_equal(zc[:2], np.array([[2, 5, 9], [2, 5, 9]], F32))
    c, b, w = D.trim([3, 3, 2], bins, wts, zc, np.array([5.0, np.nan, -np.inf], F32))
    assert c.tolist() == [1, 3, 0] and b.tolist() == [[2, -1, -1], [2, 5, 9], [-1, -1, -1]]
    assert w[0].tolist() == [F32(.1), 0, 0] and w[2].tolist() == [0, 0, 0]
    rgb = np.array([[.1, .2, .3]] * 6, F32)
    behind = np.array([[1, 1, 1], [np.nan, np.inf, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [np.nan, 1, 1]], F32)
    acc = np.array([0.25, 1.0, 2.0, -1.0, np.nan, 0.5], F32)
    out, rgba = D.blend(rgb, acc, behind)
    assert out[0].tolist() == [F32(.1) + F32(.75), F32(.2) + F32(.75), F32(.3) + F32(.75)]
    assert out[1].tobytes() == rgb[1].tobytes() and out[2].tobytes() == rgb[2].tobytes() and out[4].tobytes() == rgb[4].tobytes()
    assert out[3].tolist() == [F32(.1) + F32(1), F32(.2) + F32(1), F32(.3) + F32(1)]
    assert np.isnan(out[5, 0]) and rgba[5].tolist() == [0, 178, 204, 255]


def test_header_declares_and_library_exports_the_hybrid_calls(lib, tmp_path):
    """A C99 translation unit that takes the address of the four calls with their exact prototypes compiles against include/adanerf_hip.h
    (-Wall -Werror -pedantic) and links against the library; the ABI version is still 4; the ctypes host binds them."""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "depth_limit_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "depth_limit_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "set_depth_limit(NULL) rc=-1 compact_depth_limit(NULL) rc=-1 blend_behind(NULL) rc=-1 sphere_zc rc=0 zc=2 abi=4"
    for name in NAMES:
        assert name in R.EXPORTS and hasattr(lib, name)
    assert lib.adanerf_set_depth_limit(None, None) == EINVAL and lib.adanerf_blend_behind(None, None, None, None, 0, None, None) == EINVAL
    syms = subprocess.run(["nm", "-D", "--defined-only", adanerf_amd.library_path()], capture_output=True, text=True, check=True).stdout
    assert all(" T %s\n" % name in syms for name in NAMES)
    for name in ("set_depth_limit", "blend_behind", "compact_depth_limit", "sphere_zc", "render_hybrid"):
        assert name in dir(R.NeuralRenderer)
    header = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    assert all("int %s(" % name in header for name in NAMES)
    # the two kernels are part of the code object's source: the depth trim through the header of the render path's unit, the blend through
    # the unit of the image-space stages, and both units are built into the library
    from adanerf_amd import build as B
    kernels = open(os.path.join(ROOT, "adanerf_amd", "csrc", "kernels.hip.hpp")).read()
    stages = open(os.path.join(ROOT, "adanerf_amd", "csrc", "stages.hip")).read()
    assert '#include "k_depth_limit.hip.hpp"' in kernels and '#include "k_blend.hip.hpp"' in stages
    assert "k_depth_limit.hip.hpp" in B.include_closure(["adanerf_hip.hip"]) and "k_blend.hip.hpp" in B.include_closure(["stages.hip"])
    assert {"adanerf_hip.hip", "stages.hip"} <= set(B.LIB_SOURCES)
