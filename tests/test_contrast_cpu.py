"""CPU-only checks of adaptive supersampling (adanerf_contrast_mask / adanerf_accumulate_masked / adanerf_resolve_mean_masked /
adanerf_host_contrast_mask): the C ABI declares and exports the four without a struct change; the host mask -- the rule the device kernel
compiles from the same header -- equals the brute-force numpy definition (tests/contrast_reference.py) byte for byte, NaN, infinities,
-0 and the exact-threshold pair included; the reference rejects rules that are wrong in one way; every refusal leaves the outputs
untouched; and the CLI, the evaluator and the Python host accept and refuse the same settings.  What the device computes:
tests/test_gpu_adaptive_aa.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import contrast_reference as CR
from conftest import ROOT

import adanerf_amd
from adanerf_amd import renderer as R

SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (5, 4), (67, 5))      # (w, h)
NAMES = ("adanerf_contrast_mask", "adanerf_accumulate_masked", "adanerf_resolve_mean_masked", "adanerf_host_contrast_mask")
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def host_mask(lib, rgb, w, h, thr, out=None, count=True):
    """(code, mask, n_flagged): adanerf_host_contrast_mask through ctypes, with nothing checked on this side"""
    a = None if rgb is None else np.ascontiguousarray(rgb, dtype=f32)
    if out is None:
        out = np.full(max(w * h, 1) if 0 < w * h < 1 << 24 else 1, 0xA5, np.uint8)
    n = C.c_int32(-7)
    rc = lib.adanerf_host_contrast_mask(None if a is None else a.ctypes.data, w, h, thr, out.ctypes.data, C.byref(n) if count else None)
    return rc, out, int(n.value)


def random_image(seed, w, h):
    return np.random.default_rng(seed).uniform(-0.5, 1.5, (h * w, 3)).astype(f32)


def special_image(seed, w, h):
    """random values with NaN, +-inf and -0.0 sprinkled in, at least one of each where the image has the room"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 1.5, h * w * 3).astype(f32)
    specials = [f32("nan"), f32("inf"), f32("-inf"), f32(-0.0), f32(0.0), f32(1.0)]
    idx = rng.permutation(a.size)[:max(a.size // 3, min(a.size, len(specials)))]
    for k, i in enumerate(idx):
        a[i] = specials[k % len(specials)]
    return a.reshape(h * w, 3)


def check(lib, rgb, w, h, thr):
    rc, got, n = host_mask(lib, rgb, w, h, thr)
    want, n_want = CR.contrast_mask(rgb, w, h, thr)
    assert rc == 0
    assert np.array_equal(got, want), (w, h, thr, np.flatnonzero(got != want)[:8])
    assert n == n_want == int(np.count_nonzero(got == 0))
    g = got.reshape(h, w) == 0      # symmetry: every flagged pixel has a flagged neighbour
    for y, x in zip(*np.nonzero(g)):
        nb = g[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
        assert nb.sum() >= 2, (w, h, thr, x, y)
    return got


def test_header_declares_and_library_exports_the_entry_points(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "contrast_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "contrast_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == ("contrast_mask(NULL) rc=-1 flagged=-7 accumulate_masked(NULL) rc=-1 resolve_mean_masked(NULL) rc=-1 "
                        "host_contrast_mask rc=0 flagged=2 abi=4")
    assert [int(v) for v in lines[1].split()] == [1, 0, 0, 1]
    assert all(n in R.EXPORTS and hasattr(lib, n) for n in NAMES) and lib.adanerf_abi_version() == 4
    assert [C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)] == [64, 164, 96]      # no struct changed
    header = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in header
    for phrase in ("v(p, ch) = fminf(fmaxf(d_rgb[3 p + ch], 0), 1)", "the comparison is strict", "A 1 x 1 image flags nothing",
                   "d_mask[p] = 0 if flagged"):
        assert phrase in header, phrase
    rule = open(os.path.join(ROOT, "adanerf_amd", "csrc", "contrast_rule.hpp")).read()
    for user in ("k_contrast.hip.hpp", "model_setup.cpp"):      # one text, compiled twice
        assert '#include "contrast_rule.hpp"' in open(os.path.join(ROOT, "adanerf_amd", "csrc", user)).read()
    assert "contrast_mask_byte" in rule and "hip_runtime" not in rule


def test_a_null_context_is_refused_before_any_device_work(lib):
    n = C.c_int32(-7)
    assert lib.adanerf_contrast_mask(None, 4096, 4, 4, 0.5, 8192, C.byref(n)) == -1 and n.value == -7
    assert lib.adanerf_accumulate_masked(None, 4096, 8192, 1, 4, 16384, 1) == -1
    assert lib.adanerf_resolve_mean_masked(None, 4096, 8192, 1, 4, 4, None, 16384) == -1


@pytest.mark.parametrize("w,h", SIZES)
def test_host_mask_is_the_brute_force_definition(lib, w, h):
    seen = set()
    for k, thr in enumerate((0.0, 0.05, 0.3, 0.7, 1.0)):
        seen |= set(check(lib, random_image(w * 100 + h * 10 + k, w, h), w, h, thr).tolist())
        seen |= set(check(lib, special_image(w * 100 + h * 10 + k, w, h), w, h, thr).tolist())
    assert seen == ({1} if w * h == 1 else {0, 1})
    # threshold 1: no clamped difference exceeds it; threshold 0 on a constant image: nothing differs
    assert np.all(check(lib, special_image(5, w, h), w, h, 1.0) == 1)
    assert np.all(check(lib, np.full((h * w, 3), 0.25, f32), w, h, 0.0) == 1)
    if w * h > 1:      # threshold 0 flags every pixel of an image in which all neighbours differ
        ramp = (np.arange(h * w, dtype=f32) / f32(h * w)).repeat(3).reshape(-1, 3)
        assert np.all(check(lib, ramp, w, h, 0.0) == 0)


def test_special_values_clamp_as_the_byte_contract_does(lib):
    nan, inf = f32("nan"), f32("inf")
    # one row of pairs: (left, right, flagged at threshold 0.5)
    pairs = [(nan, 0.0, False), (nan, 1.0, True), (-inf, 0.0, False), (inf, 1.0, False), (inf, -inf, True), (-0.0, 0.0, False), (nan, -5.0, False),
             (7.0, 1.0, False), (-3.0, 0.6, True), (inf, nan, True), (1.5, 0.49, True), (1.5, 0.5, False)]
    for a, b, flagged in pairs:
        for ch in range(3):
            rgb = np.zeros((2, 3), f32)
            rgb[0, :] = 0.25
            rgb[1, :] = 0.25
            rgb[0, ch], rgb[1, ch] = a, b
            for w, h in ((2, 1), (1, 2)):
                got = check(lib, rgb, w, h, 0.5)
                assert np.all(got == (0 if flagged else 1)), (a, b, ch, w, h)


def test_the_threshold_pair_is_strict_in_fp32(lib):
    """a pair whose contrast equals the threshold exactly is not flagged; one ulp above it is"""
    for lo, thr in ((0.25, 0.5), (0.125, 0.3), (0.0, 0.1), (0.0009765625, 0.05)):
        thr32 = f32(thr)
        hi = f32(f32(lo) + thr32)
        assert f32(hi - f32(lo)) == thr32      # the difference is representable: the pair sits exactly on the threshold
        above = np.nextafter(hi, f32(2))
        assert f32(above - f32(lo)) > thr32
        for ch in range(3):
            for (w, h), q in (((2, 1), 1), ((1, 2), 1), ((2, 2), 3)):      # horizontal, vertical and diagonal neighbours
                rgb = np.full((w * h, 3), lo, f32)
                rgb[q, ch] = hi
                assert np.all(check(lib, rgb, w, h, float(thr32)) == 1), (lo, thr, ch, w, h)
                rgb[q, ch] = above
                got = check(lib, rgb, w, h, float(thr32))
                assert np.all(got == 0), (lo, thr, ch, w, h)      # in a 2 x 2 image every pixel neighbours q


def test_the_reference_rejects_rules_that_are_wrong_in_one_way(lib):
    w, h = 5, 4
    # a lone diagonal step: only the diagonal neighbour differs
    diag = np.full((h * w, 3), 0.2, f32)
    diag[0] = 0.9      # pixel (1, 1) differs from (0, 0) alone, and only across the diagonal
    want, _ = CR.contrast_mask(diag, w, h, 0.5)
    assert want.reshape(h, w)[1, 1] == 0 and not np.array_equal(CR.faulty_masks(diag, w, h, 0.5)["no diagonals"], want)
    # a pair exactly on the threshold
    edge = np.full((h * w, 3), 0.25, f32)
    edge[7, 1] = 0.75
    want, n = CR.contrast_mask(edge, w, h, 0.5)
    assert n == 0 and not np.array_equal(CR.faulty_masks(edge, w, h, 0.5)[">= instead of >"], want)
    # values outside [0, 1] that the display clamps together
    hot = np.full((h * w, 3), 1.0, f32)
    hot[9, 2] = 40.0
    hot[3, 0] = np.nan
    hot[4, 0] = 0.0
    want, n = CR.contrast_mask(hot, w, h, 0.5)
    assert not np.array_equal(CR.faulty_masks(hot, w, h, 0.5)["no clamp"], want)
    for img in (diag, edge, hot):      # and the library is on the reference's side each time
        check(lib, img, w, h, 0.5)


def test_every_refusal_leaves_the_output_untouched(lib):
    w, h = 6, 5
    rgb = random_image(3, w, h)
    assert host_mask(lib, rgb, w, h, 0.3)[0] == 0
    nan, inf = float("nan"), float("inf")
    for thr in (nan, inf, -inf, -0.001, 1.001, 2.0, -1.0):
        rc, out, n = host_mask(lib, rgb, w, h, thr)
        assert rc == -1 and np.all(out == 0xA5) and n == -7, thr
        assert "adanerf_host_contrast_mask" in lib.adanerf_last_error(None).decode()
    for ww, hh in ((0, 5), (6, 0), (-1, 5), (16385, 5), (6, 16385)):
        rc, out, n = host_mask(lib, rgb, ww, hh, 0.3, out=np.full(64, 0xA5, np.uint8))
        assert rc == -1 and np.all(out == 0xA5) and n == -7, (ww, hh)
    n = C.c_int32(-7)
    out = np.full(w * h, 0xA5, np.uint8)
    assert lib.adanerf_host_contrast_mask(None, w, h, 0.3, out.ctypes.data, C.byref(n)) == -1 and np.all(out == 0xA5) and n.value == -7
    assert lib.adanerf_host_contrast_mask(rgb.ctypes.data, w, h, 0.3, None, C.byref(n)) == -1 and n.value == -7
    # an image that is not 4-byte aligned; a mask inside the image (first byte, last byte), each refused with the image's bytes intact
    raw = np.zeros(w * h * 12 + 8, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 4
    assert lib.adanerf_host_contrast_mask(base + 1, w, h, 0.3, out.ctypes.data, C.byref(n)) == -1 and np.all(out == 0xA5) and n.value == -7
    img = rgb.copy()
    for off in (0, w * h * 12 - 1, -(w * h) + 1):
        assert lib.adanerf_host_contrast_mask(img.ctypes.data, w, h, 0.3, img.ctypes.data + off, C.byref(n)) == -1 and n.value == -7, off
        assert np.array_equal(img.view(np.uint32), rgb.view(np.uint32))
    # a mask at an odd address and a NULL count are fine
    odd = np.full(w * h + 2, 0xA5, np.uint8)
    assert lib.adanerf_host_contrast_mask(rgb.ctypes.data, w, h, 0.3, odd.ctypes.data + 1, None) == 0
    assert np.array_equal(odd[1:-1], CR.contrast_mask(rgb, w, h, 0.3)[0]) and odd[0] == odd[-1] == 0xA5
    for bad in (dict(width=0, height=4), dict(width=4, height=1 << 15)):
        with pytest.raises(ValueError):
            R.host_contrast_mask(np.zeros((16, 3), f32), threshold=0.3, **bad)
    for thr in (nan, -0.1, 1.5):
        with pytest.raises(ValueError):
            R.host_contrast_mask(np.zeros((16, 3), f32), 4, 4, thr)
    with pytest.raises(ValueError):
        R.host_contrast_mask(np.zeros((15, 3), f32), 4, 4, 0.3)
    m, cnt = R.host_contrast_mask(rgb, w, h, 0.3)
    assert np.array_equal(m, CR.contrast_mask(rgb, w, h, 0.3)[0]) and cnt == int(np.count_nonzero(m == 0))


def test_masked_pair_reference_is_the_unmasked_pair_on_the_selected_pixels():
    """the numpy restatements the GPU tests compare against: selected pixels equal antialias_reference's, the others keep their bits"""
    import antialias_reference as AR
    rng = np.random.default_rng(11)
    n = 40
    mask = rng.choice(np.array([0, 1, 2, 31, 32, 255], np.uint8), n)
    for values in (1, 2, 5, 1 << 31, 0xFFFFFFFF):
        sel = CR.selected(mask, values)
        assert np.array_equal(sel, np.array([m < 32 and (values >> int(m)) & 1 == 1 for m in mask]))
        canary = np.full((n, 3), np.uint32(0x7FC12345), np.uint32).view(f32)      # a NaN payload
        rgb = rng.uniform(-1, 2, (n, 3)).astype(f32)
        first = CR.accumulate_masked(rgb, mask, values, canary, True)
        assert np.array_equal(first[sel], rgb[sel]) and np.all(first.view(np.uint32)[~sel] == 0x7FC12345)
        second = CR.accumulate_masked(rgb, mask, values, first, False)
        assert np.array_equal(second[sel], AR.accumulate_f32(first, rgb, False)[sel]) and np.all(second.view(np.uint32)[~sel] == 0x7FC12345)
        rgba_before = np.full((n, 4), 0x5A, np.uint8)
        m, b = CR.resolve_mean_masked(second, mask, values, 2, canary, rgba_before)
        want_m, want_b = AR.resolve_f32(second, 2)
        assert np.array_equal(m[sel], want_m[sel]) and np.array_equal(b[sel], want_b[sel])
        assert np.all(m.view(np.uint32)[~sel] == 0x7FC12345) and np.all(b[~sel] == 0x5A)
    assert not CR.selected(mask, 1 << 31)[mask != 31].any() and CR.selected(mask, 1 << 31)[mask == 31].all()


def test_cli_parses_supersample_contrast(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--supersample-contrast T" in usage
    model = os.path.join(str(ROOT), "no_such_model")

    def run(*args):
        return subprocess.run([cli, model] + list(args) + ["--dry-run", "--frames", "1"], capture_output=True, text=True, timeout=60)
    for t in ("0", "1", "0.3", "1e-3", "0.05"):
        for args in (["--supersample", "2", "--supersample-contrast", t], ["--supersample-contrast", t, "--supersample", "8"]):
            out = run(*args)
            assert out.returncode != 0 and "config.ini" in out.stdout and "Argument parsing failed" not in out.stdout, args      # parsed: it fails on the model
    for t in ("", "x", "0.3x", "-0.1", "1.01", "2", "nan", "inf", "-inf"):
        out = run("--supersample", "2", "--supersample-contrast", t)
        assert out.returncode != 0 and "--supersample-contrast T: T must be a number in [0, 1]" in out.stdout, t
    out = subprocess.run([cli, "m", "--supersample-contrast"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "missing value after --supersample-contrast" in out.stdout
    for args in (["--supersample-contrast", "0.3"], ["--supersample-contrast", "0.3", "--supersample", "1"]):
        out = run(*args)
        assert out.returncode != 0 and "only with --supersample S, S >= 2" in out.stdout, args
    # every combination --supersample refuses is refused in the same words
    for extra in (["--taa", "0.1"], ["--taau", "2"], ["--occluder", "0,0,0,1"], ["--fovea-density", "5:1,2"]):
        plain = run("--supersample", "2", *extra)
        adaptive = run("--supersample", "2", "--supersample-contrast", "0.3", *extra)
        assert plain.returncode != 0 and adaptive.returncode != 0 and "--supersample" in plain.stdout
        assert "config.ini" not in plain.stdout and adaptive.stdout == plain.stdout, extra


def test_python_host_signatures():
    P = R.NeuralRenderer
    assert list(inspect.signature(P.contrast_mask).parameters) == ["self", "rgb", "width", "height", "threshold", "mask_out", "count"]
    assert inspect.signature(P.contrast_mask).parameters["count"].default is True
    assert list(inspect.signature(P.accumulate_masked_device).parameters) == ["self", "rgb", "mask", "values", "n_rays", "sum_out", "first"]
    assert list(inspect.signature(P.resolve_mean_masked_device).parameters) == ["self", "sum_in", "mask", "values", "n_rays", "frames", "rgba8_out",
                                                                                 "rgb_out"]
    assert list(inspect.signature(P.render_supersampled_adaptive).parameters) == ["self", "s", "threshold"]
    assert list(inspect.signature(P.render_supersampled).parameters) == ["self", "s"]      # unchanged
    assert list(inspect.signature(R.host_contrast_mask).parameters) == ["rgb", "width", "height", "threshold"]


def test_evaluator_takes_a_supersample_contrast(tmp_path):
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["m", "d"]).supersample_contrast is None
    assert ap.parse_args(["m", "d", "--supersample", "2", "--supersample-contrast", "0.3"]).supersample_contrast == 0.3
    params = list(inspect.signature(E.evaluate).parameters)
    assert params[-1] == "sweep_scales" and params[-2] == "supersample_contrast"
    assert inspect.signature(E.evaluate).parameters["supersample_contrast"].default is None
    no = (str(tmp_path / "no_model"), str(tmp_path / "no_dataset"))
    for kw in (dict(supersample_contrast=0.3), dict(supersample=1, supersample_contrast=0.3), dict(supersample=2, supersample_contrast=1.5),
               dict(supersample=2, supersample_contrast=-0.1), dict(supersample=2, supersample_contrast=float("nan")),
               dict(supersample=2, supersample_contrast=0.3, reproject_stride=2), dict(supersample=2, supersample_contrast=0.3, temporal=0.1)):
        with pytest.raises(ValueError):
            E.evaluate(*no, **kw)
    for argv in (["m", "d", "--supersample-contrast", "0.3"], ["m", "d", "--supersample", "1", "--supersample-contrast", "0.3"],
                 ["m", "d", "--supersample", "2", "--supersample-contrast", "1.5"], ["m", "d", "--supersample", "2", "--supersample-contrast", "x"]):
        with pytest.raises(SystemExit):
            E.main(argv)
    plain = [dict(frame=0, samples_per_ray=4.0, ms=1.0, mse=0.01, psnr=20.0, supersample=2)]
    ada = [dict(plain[0], refined_fraction=0.25), dict(plain[0], frame=1, refined_fraction=0.75)]
    s0, s1 = E.summarise(plain, False), E.summarise(ada, False)
    assert sorted(s1) == sorted(list(s0) + ["mean_refined_fraction"]) and s1["mean_refined_fraction"] == 0.5
