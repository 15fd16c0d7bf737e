"""CPU-only checks of the two-source reprojection (adanerf_reproject_pair, adanerf_host_pair_weight): the C ABI declares and exports both
without a struct change, the hosts have their new flags and methods and keep the old ones, the restatement the GPU tests compare against
(tests/reproject_pair_reference.py) has the properties a two-source warp must have, and the inputs of the GPU tests keep pixel-boundary
and tolerance ties rare enough for exact equality to be a fair demand.  What the kernels compute: tests/test_gpu_reproject_pair.py."""
import ctypes as C
import inspect
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import reproject_pair_reference as P
import reproject_reference as RR
from conftest import ROOT, load_case

import adanerf_amd
from adanerf_amd import renderer as R

W, H = RR.SIZES[0]
F32 = np.float32


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


# ---- the ABI and the hosts -------------------------------------------------------------------------

def test_header_declares_and_library_exports_the_entry_points(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "reproject_pair_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "reproject_pair_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "reproject_pair(NULL) rc=-1 holes=-7 abi=4 fill=1"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # no struct changed
    assert lines[2] == "pair_weight 0.5"
    assert all(n in R.EXPORTS and hasattr(lib, n) for n in ("adanerf_reproject_pair", "adanerf_host_pair_weight"))
    assert lib.adanerf_abi_version() == 4


def test_a_null_context_is_refused_before_any_device_work(lib):
    f3, f9 = (C.c_float * 3)(0, 0, 0), (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    holes = C.c_int32(-7)
    assert lib.adanerf_reproject_pair(None, None, None, None, f3, f9, None, None, None, f3, f9, f3, f9, 0.5, 0.5, 0.05, 0, 1, None, None, None, None, None,
                                      C.byref(holes)) == -1
    assert lib.adanerf_reproject_pair(None, 4096, 4096, 4096, f3, f9, 4096, 4096, 4096, f3, f9, f3, f9, 0.5, 0.5, 0.05, 0, 0, 65536, None, None, None, None, None) == -1
    assert holes.value == -7


def _weight_f64(dst, a, b):
    """the header's definition: float64 from the fp32 positions, one rounded operation per step, the cast last"""
    d = []
    for s in (a, b):
        e = [float(F32(x)) - float(F32(y)) for x, y in zip(dst, s)]
        d.append(math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))
    return 0.5 if d[0] + d[1] == 0.0 else float(F32(d[0] / (d[0] + d[1])))


def test_pair_weight(lib):
    a, b = [0.25, -1.5, 3.0], [1.75, 0.5, 2.0]
    mid = [1.0, -0.5, 2.5]
    assert R.pair_weight(mid, a, b) == 0.5 and R.pair_weight(a, a, b) == 0.0 and R.pair_weight(b, a, b) == 1.0 and R.pair_weight(a, a, a) == 0.5
    rng = np.random.default_rng(5)
    fp = C.POINTER(C.c_float)
    for _ in range(200):
        dst, pa, pb = (rng.normal(size=3) * 10.0 ** rng.integers(-3, 4)).astype(F32), rng.normal(size=3).astype(F32), rng.normal(size=3).astype(F32)
        out = C.c_float(-1)
        assert lib.adanerf_host_pair_weight(dst.ctypes.data_as(fp), pa.ctypes.data_as(fp), pb.ctypes.data_as(fp), C.byref(out)) == 0
        want = _weight_f64(dst, pa, pb)
        assert F32(out.value).view(np.uint32) == F32(R.pair_weight(dst, pa, pb)).view(np.uint32) == F32(want).view(np.uint32)
        assert 0.0 <= out.value <= 1.0
    out = C.c_float(-1)
    bad = np.array([np.nan, 0, 0], F32)
    ok = np.zeros(3, F32)
    for args in ((bad, ok, ok), (ok, bad, ok), (ok, ok, np.array([0, np.inf, 0], F32))):
        assert lib.adanerf_host_pair_weight(*[x.ctypes.data_as(fp) for x in args], C.byref(out)) == -1 and out.value == -1
        with pytest.raises(ValueError):
            R.pair_weight(*args)
    assert lib.adanerf_host_pair_weight(None, ok.ctypes.data_as(fp), ok.ctypes.data_as(fp), C.byref(out)) == -1
    assert lib.adanerf_host_pair_weight(ok.ctypes.data_as(fp), ok.ctypes.data_as(fp), ok.ctypes.data_as(fp), None) == -1


def test_python_host_keeps_its_signatures_and_has_the_new_methods():
    sig = inspect.signature(R.NeuralRenderer.reproject).parameters
    assert list(sig)[1:] == ["dst_pos", "dst_rot", "fill", "acc_min"] and sig["fill"].default is True and sig["acc_min"].default == 0.5
    assert list(inspect.signature(R.NeuralRenderer.render_numpy).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.enable_reprojection).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.reproject_rerender).parameters)[1:] == ["dst_pos", "dst_rot", "rerender", "fill", "acc_min"]
    assert list(inspect.signature(R.NeuralRenderer.reproject_gather).parameters)[1:] == ["dst_pos", "dst_rot", "iterations", "depth_tol", "guess", "acc_min"]
    assert list(inspect.signature(R.NeuralRenderer.enable_interpolation).parameters) == ["self"]
    assert list(inspect.signature(R.NeuralRenderer.render_keyframe).parameters) == ["self"]
    sig = inspect.signature(R.NeuralRenderer.interpolate).parameters
    assert list(sig)[1:] == ["dst_pos", "dst_rot", "weight_b", "fill", "acc_min", "depth_tol"]
    assert (sig["weight_b"].default, sig["fill"].default, sig["acc_min"].default, sig["depth_tol"].default) == (None, True, 0.5, 0.05) and P.DEPTH_TOL == 0.05
    sig = inspect.signature(R.NeuralRenderer.interpolate_rerender).parameters
    assert list(sig)[1:4] == ["dst_pos", "dst_rot", "rerender"] and sig["rerender"].default == "holes"
    assert list(inspect.signature(R.NeuralRenderer.reproject_pair_device).parameters)[1:14] == [
        "a_rgb", "a_depth", "a_acc", "a_pos", "a_rot", "b_rgb", "b_depth", "b_acc", "b_pos", "b_rot", "dst_pos", "dst_rot", "dst_rgb"]
    assert list(inspect.signature(R.pair_weight).parameters) == ["dst_pos", "a_pos", "b_pos"]


def test_cli_help_names_the_flag_and_refuses_what_it_excludes(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--interpolate K", "--reproject-warp splat|gather", "--reproject K", "--rerender holes|unsourced"):
        assert flag in usage, flag
    for args, word in ((["--interpolate", "1"], "K must be an integer >= 2"), (["--interpolate", "0"], "K must be an integer >= 2"),
                       (["--interpolate", "two"], "K must be an integer >= 2"), (["--interpolate", "2.5"], "K must be an integer >= 2"),
                       (["--interpolate"], "missing value after --interpolate"),
                       (["--interpolate", "3", "--reproject", "2"], "not with --reproject"), (["--interpolate", "3", "--taa", "0.1"], "not with --taa"),
                       (["--interpolate", "3", "--taau", "2"], "not with --taau"), (["--interpolate", "3", "--supersample", "2"], "not with --supersample"),
                       (["--interpolate", "3", "--fovea-density", "10:1,2"], "not with --fovea-density"),
                       (["--interpolate", "3", "--occluder", "0,0,0,1"], "not with --occluder"),
                       (["--interpolate", "3", "--gpus", "2"], "--interpolate warps whole frames of one context; use it with --gpus 1"),
                       (["--rerender", "holes"], "only with --reproject K")):
        out = subprocess.run([cli, "m"] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and word in out.stdout, (args, out.stdout[-400:])
        if "--interpolate" in args and len(args) > 2:
            assert "--interpolate" in [l for l in out.stdout.splitlines() if word in l][0]      # each exclusion is the flag's own message
    # --rerender goes with --interpolate as it goes with --reproject: the arguments pass, the model directory is what is missing
    out = subprocess.run([cli, "m", "--interpolate", "3", "--rerender", "holes"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "only with --reproject" not in out.stdout and "config.ini" in out.stdout + out.stderr


def test_evaluator_has_the_option_and_keeps_its_summary_keys():
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["m", "d"]).interpolate_stride is None
    assert ap.parse_args(["m", "d", "--interpolate-stride", "3", "--rerender", "holes"]).interpolate_stride == 3
    sig = inspect.signature(E.evaluate).parameters
    assert sig["interpolate_stride"].default is None and sig["reproject_stride"].default is None and sig["reproject_warp"].default == "splat"
    for kw in (dict(interpolate_stride=0), dict(interpolate_stride=-2), dict(interpolate_stride=2.5), dict(interpolate_stride=2, reproject_stride=2),
               dict(interpolate_stride=2, supersample=2), dict(interpolate_stride=2, temporal=0.1), dict(interpolate_stride=2, temporal_still=2),
               dict(interpolate_stride=2, temporal_upsample=2), dict(interpolate_stride=2, fovea_density="10:1,2"), dict(interpolate_stride=2, sweep_scales=[0.5]),
               dict(interpolate_stride=2, sweep_samples=[4]), dict(interpolate_stride=2, sweep_sample_caps=[4.0]), dict(interpolate_stride=2, reproject_warp="gather"),
               dict(rerender="holes")):
        with pytest.raises(ValueError):
            E.evaluate("m", "d", **kw)
    for argv in (["m", "d", "--interpolate-stride", "2", "--reproject-stride", "2"], ["m", "d", "--interpolate-stride", "2", "--supersample", "2"],
                 ["m", "d", "--interpolate-stride", "2", "--temporal", "0.1"], ["m", "d", "--rerender", "holes"]):
        with pytest.raises(SystemExit):
            E.main(argv)
    key = dict(frame=0, image="x", interpolated=False, samples_per_ray=3.0, ms=1.0, mse=0.01, psnr=20.0, flip=0.1)
    made = dict(frame=1, image="y", interpolated=True, hole_fraction=0.25, blended_fraction=0.5, mse=0.1, psnr=10.0, flip=0.3)
    plain_keys = ["frames", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    ip_keys = plain_keys + ["mean_blended_fraction", "mean_hole_fraction", "mean_psnr_interpolated", "mean_psnr_rendered"]
    s = E.summarise([key, made], False)
    assert sorted(s) == sorted(ip_keys)
    assert (s["mean_psnr_rendered"], s["mean_psnr_interpolated"], s["mean_hole_fraction"], s["mean_blended_fraction"]) == (20.0, 10.0, 0.25, 0.5)
    assert (s["mean_samples_per_ray"], s["mean_ms"], s["mean_psnr"]) == (3.0, 1.0, 15.0)
    assert sorted(E.summarise([key, made], True)) == sorted(ip_keys + ["mean_flip", "mean_flip_interpolated", "mean_flip_rendered"])
    rr = dict(made, rerendered_fraction=0.25, psnr_rerendered=12.0, mse_rerendered=0.06)
    s = E.summarise([key, rr], False)
    assert sorted(s) == sorted(ip_keys + ["mean_psnr_interpolated_rerendered", "mean_rerendered_fraction"]) and s["mean_psnr_interpolated_rerendered"] == 12.0
    # a plain run and a --reproject-stride run keep exactly the keys they have
    plain = dict(frame=0, image="x", samples_per_ray=3.0, ms=1.0, mse=0.01, psnr=20.0)
    assert sorted(E.summarise([plain], False)) == plain_keys
    warped = [dict(plain, warped=False), dict(frame=1, image="y", warped=True, warp="splat", hole_fraction=0.25, mse=0.1, psnr=10.0)]
    assert sorted(E.summarise(warped, False)) == sorted(plain_keys + ["mean_hole_fraction", "mean_psnr_rendered", "mean_psnr_warped"])


# ---- properties of the definition ------------------------------------------------------------------

def _rgba(n):
    return np.zeros((n, 4), np.uint8)


def _single(scene, a, dst, flags, cam=False):
    return RR.reproject_f32(scene, W, H, cam, _rgba(W * H), a.depth, a.acc, a.pos, a.rot, dst[0], dst[1], flags=flags)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_b_identical_to_a_is_the_single_source_warp(scene, name):
    """mask, depth and winner are reproject_f32's for every weight_b; the colour is exactly A's at every winner"""
    a, _, dp, dr = P.case(scene, W, H, False, name)
    for flags in (0, RR.FILL):
        _, depth, mask, holes, winner = _single(scene, a, (dp, dr), flags)
        for wb in (0.0, 0.25, 1.0):
            r = P.pair_f32(scene, W, H, False, a, a, dp, dr, weight_b=wb, flags=flags)
            assert np.array_equal(r.mask, mask) and np.array_equal(r.depth.view(np.uint32), depth.view(np.uint32)) and r.holes == holes
            assert np.array_equal(r.winner_a, winner) and np.array_equal(r.winner_b, winner)
            won = winner >= 0
            finite = np.isfinite(a.rgb[winner[won]])
            assert np.array_equal(r.rgb[won][finite], a.rgb[winner[won]][finite])      # as values: cA + w * (cA - cA) turns a -0 into +0
            assert np.all(r.source[won] == 3) and np.all(r.source[mask == 2] == 1) and np.all(r.source[mask == 0] == 0)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_a_hole_of_the_pair_is_a_hole_of_both_single_warps(scene, name):
    a, b, dp, dr = P.case(scene, W, H, False, name)
    ma, mb = _single(scene, a, (dp, dr), 0)[2], _single(scene, b, (dp, dr), 0)[2]
    r = P.pair_f32(scene, W, H, False, a, b, dp, dr, flags=0)
    assert np.array_equal(r.mask == 0, (ma == 0) & (mb == 0)) and set(np.unique(r.mask).tolist()) <= {0, 1}
    assert r.holes <= min(int(np.count_nonzero(ma == 0)), int(np.count_nonzero(mb == 0)))
    assert np.array_equal(r.source == 0, r.mask == 0) and np.all(r.depth[r.mask == 0] == 0) and np.all(r.rgb[r.mask == 0].view(np.uint32) == 0)
    assert np.all(r.rgba8[r.mask == 0] == np.frombuffer(np.uint32(RR.HOLE).tobytes(), np.uint8))
    print("%s: holes from A alone %d, from B alone %d, when both are used %d of %d" % (name, np.count_nonzero(ma == 0), np.count_nonzero(mb == 0), r.holes, W * H))
    if name != "independent":      # the consistent scene: the two views uncover each other's disocclusions
        assert r.holes * 2 < min(int(np.count_nonzero(ma == 0)), int(np.count_nonzero(mb == 0)))


def test_a_near_winner_beats_a_far_one_and_the_nearer_of_two_near_ones_wins(scene):
    a, b, dp, dr = P.case(scene, W, H, False, "independent")      # far pixels planted in both frames, at different places
    r = P.pair_f32(scene, W, H, False, a, b, dp, dr, depth_tol=0.0, flags=0)
    both = (r.winner_a >= 0) & (r.winner_b >= 0)
    za, zb = (r.key_a >> np.uint64(32)).astype(np.uint32).view(F32), (r.key_b >> np.uint64(32)).astype(np.uint32).view(F32)
    far_a, far_b = np.isinf(za) & both, np.isinf(zb) & both
    assert np.count_nonzero(far_a & ~far_b) > 0 and np.count_nonzero(far_b & ~far_a) > 0
    assert np.all(r.source[far_a & ~far_b] == 2) and np.all(r.source[far_b & ~far_a] == 1)
    assert np.all(r.source[far_a & far_b] == 3) and np.all(np.isinf(r.depth[far_a & far_b]))
    near = both & ~far_a & ~far_b & ~r.agree
    assert np.count_nonzero(near) > 1000      # at tolerance 0 nearly every doubly covered pixel disagrees
    assert np.array_equal(r.source[near], np.where(zb[near] < za[near], 2, 1)) and np.array_equal(r.depth[near], np.minimum(za[near], zb[near]))
    taken = np.where(r.source[near] == 1, r.winner_a[near], r.winner_b[near])
    src = np.where((r.source[near] == 1)[:, None], a.rgb[taken], b.rgb[taken])
    assert np.array_equal(r.rgb[near].view(np.uint32), src.view(np.uint32))


@pytest.mark.parametrize("name", ["forward", "yaw", "independent"])
def test_the_fill_takes_the_largest_of_the_sixteen_keys(scene, name):
    a, b, dp, dr = P.case(scene, W, H, False, name)
    r = P.pair_f32(scene, W, H, False, a, b, dp, dr, flags=RR.FILL)
    bare = P.pair_f32(scene, W, H, False, a, b, dp, dr, flags=0)
    filled = np.flatnonzero(r.mask == 2)
    assert filled.size > 0 and np.all(bare.mask[filled] == 0) and np.array_equal(r.mask == 1, bare.mask == 1)
    ka, kb = bare.key_a.reshape(H, W), bare.key_b.reshape(H, W)
    for j in filled:
        y, x = divmod(int(j), W)
        cand = [(int(k[yy, xx]), s, yy * W + xx) for s, k in ((1, ka), (2, kb)) for yy in range(max(0, y - 1), min(H, y + 2))
                for xx in range(max(0, x - 1), min(W, x + 2)) if (yy, xx) != (y, x) and k[yy, xx] != 0]
        best = max(cand, key=lambda c: (c[0], -c[1]))      # the largest key; on equal keys A
        src_px = best[0] & 0xFFFFFFFF
        assert r.source[j] == best[1] and r.depth[j].view(np.uint32) == best[0] >> 32
        assert np.array_equal(r.rgb[j].view(np.uint32), (a if best[1] == 1 else b).rgb[src_px].view(np.uint32))
    # every remaining hole has no winner among its neighbours in either z-buffer
    for j in np.flatnonzero(r.mask == 0):
        y, x = divmod(int(j), W)
        assert not ka[max(0, y - 1):y + 2, max(0, x - 1):x + 2].any() and not kb[max(0, y - 1):y + 2, max(0, x - 1):x + 2].any()


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_weight_zero_returns_a_and_weight_one_stays_within_an_ulp_of_b(scene, name):
    a, b, dp, dr = P.case(scene, W, H, False, name)
    r = P.pair_f32(scene, W, H, False, a, b, dp, dr, weight_b=0.0)
    agree = r.source == 3
    ca, cb = a.rgb[r.winner_a[agree]], b.rgb[r.winner_b[agree]]
    finite = np.isfinite(ca) & np.isfinite(cb)
    assert np.count_nonzero(agree) > 1000 and np.array_equal(r.rgb[agree][finite], ca[finite])
    one = P.pair_f32(scene, W, H, False, a, b, dp, dr, weight_b=1.0)
    assert np.allclose(one.rgb[agree][finite], cb[finite], rtol=0, atol=4 * np.finfo(F32).eps)      # cA + (cB - cA): two roundings of values below 2
    assert np.array_equal(one.source, r.source) and np.array_equal(one.mask, r.mask)      # the weight moves no decision


# ---- the input condition of the GPU tests' exact equality --------------------------------------------

CASES = [(w, h, name, cam) for (w, h) in RR.SIZES for name in P.CASE_NAMES for cam in (False, True)]


@pytest.mark.parametrize("w,h,name,camera_origin", CASES, ids=["%dx%d-%s%s" % (w, h, n, "-cf" if c else "") for w, h, n, c in CASES])
def test_inputs_keep_boundary_and_depth_ties_rare(scene, scene_cf, w, h, name, camera_origin):
    """float32 and float64 agree on each source's winner on at least 98 % of the destination pixels and on the agree / disagree decision
    on at least 98 % of the pixels where both have winners, for every (size, case, origin) the GPU test runs.  At the hosts' tolerance
    that is asserted as it stands.  At depth_tol 0 the decision is zA == zB, and one frame cannot meet a percentage: on the 1 x 1
    lateral frame the only pixel looks down the ball's axis from two mirrored cameras, so the two depths are equal in exact arithmetic,
    float32 keeps them equal and float64 does not (1 of 1 pixels differ; the mirrored pairs of the 97 x 61 frame: 4 of 5325).  There the
    bound is 2 % of the pixels or one pixel, whichever is larger; the GPU test demands pair_f32's bits on that pixel as on every other."""
    sc = scene_cf if camera_origin else scene
    a, b, dp, dr = P.case(sc, w, h, camera_origin, name)
    for tol in (0.0, P.DEPTH_TOL):
        r32 = P.pair_f32(sc, w, h, camera_origin, a, b, dp, dr, depth_tol=tol)
        r64 = P.pair_f64(sc, w, h, camera_origin, a, b, dp, dr, depth_tol=tol)
        same_a, same_b = np.mean(r32.winner_a == r64.winner_a), np.mean(r32.winner_b == r64.winner_b)
        both = (r32.winner_a >= 0) & (r32.winner_b >= 0) & (r64.winner_a >= 0) & (r64.winner_b >= 0)
        same_d = np.mean(r32.agree[both] == r64.agree[both]) if both.any() else 1.0
        differ = int(np.count_nonzero(r32.agree[both] != r64.agree[both]))
        assert same_a >= 0.98 and same_b >= 0.98, (tol, same_a, same_b)
        assert same_d >= 0.98 or (tol == 0.0 and differ <= 1), (tol, same_d, differ, int(np.count_nonzero(both)))
