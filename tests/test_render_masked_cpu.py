"""CPU-only checks of masked rendering (adanerf_render_masked): the C ABI declares and exports it and the two buffer constants of its ray
list without a struct change, the numpy definition the GPU tests compare against (tests/mask_reference.py) agrees with a per-pixel loop,
and both hosts and the evaluator accept --rerender only with their reprojection option.  What the device computes:
tests/test_gpu_render_masked.py."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import mask_reference as MR
from conftest import ROOT

import adanerf_amd
from adanerf_amd import renderer as R


@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


def test_header_declares_and_library_exports_the_entry_point(lib, tmp_path):
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the header from C"
    from adanerf_amd.build import LIBDIR
    exe = str(tmp_path / "mask_abi_check")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", os.path.join(ROOT, "tests", "mask_abi_check.c"), "-L", LIBDIR,
                    "-ladanerf_hip", "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "render_masked(NULL) rc=-1 rendered=-7 abi=4 list=10 count=11"
    assert lines[1] == "sizes %d %d %d" % (C.sizeof(R._Options), C.sizeof(R.Info), C.sizeof(R.Stats)) == "sizes 64 164 96"      # no struct changed
    assert "adanerf_render_masked" in R.EXPORTS and hasattr(lib, "adanerf_render_masked")
    assert (R.BUF_RAY_LIST, R.BUF_RAY_LIST_COUNT) == (10, 11) and lib.adanerf_abi_version() == 4
    header = open(os.path.join(ROOT, "include", "adanerf_hip.h")).read()
    assert "needs a ray mask" not in header and "would need a ray mask" not in header


def test_a_null_context_is_refused_before_any_device_work(lib):
    rendered = C.c_int32(-7)
    assert lib.adanerf_render_masked(None, None, 1, None, None, None, C.byref(rendered)) == -1
    assert lib.adanerf_render_masked(None, 4096, 5, 8192, 16384, None, None) == -1
    assert rendered.value == -7


def _loop(mask, values):
    out = []
    for p, b in enumerate(mask.tolist()):
        if b < 32 and (values >> b) & 1:
            out.append(p)
    return np.asarray(out, np.int32)


@pytest.mark.parametrize("values", [1, 5, 1 << 31, 0xFFFFFFFF])
def test_list_of_is_the_per_pixel_rule(values):
    rng = np.random.default_rng(values & 0xFFFF)
    alphabet = np.array([0, 1, 2, 31, 32, 255], np.uint8)
    for n in (1, 6, 33, 1073):
        mask = rng.choice(alphabet, size=n)
        if n == 6:
            mask = alphabet.copy()
        got = MR.list_of(mask, values)
        assert got.dtype == np.int32 and np.array_equal(got, _loop(mask, values)), (n, values)
        assert np.all(np.diff(got) > 0)
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(MR.list_of(every, values), _loop(every, values))
    assert np.array_equal(MR.list_of(every, values), np.asarray([b for b in range(32) if (values >> b) & 1], np.int32))


def test_expected_replaces_the_selected_elements_only():
    mask = np.array([0, 1, 2, 31, 32, 255, 0, 2], np.uint8)
    before = np.arange(8 * 3, dtype=np.float32).reshape(8, 3)
    full = -before - 1
    want = before.copy()
    want[[0, 2, 6, 7]] = full[[0, 2, 6, 7]]
    assert np.array_equal(MR.expected(before, full, mask, 5), want)
    assert np.array_equal(MR.expected(before[:, 0], full[:, 0], mask, 1), np.where(mask == 0, full[:, 0], before[:, 0]))
    assert np.array_equal(MR.expected(before, full, mask, 1 << 31), np.where((mask == 31)[:, None], full, before))


def test_the_gpu_tests_masks_are_what_their_names_say():
    for n, w in ((1920, 48), (1073, 37)):
        count = {k: len(MR.list_of(*f(n, w))) for k, f in MR.MASKS.items()}
        assert (count["m1_first"], count["m1_last"], count["m127"], count["m128"], count["m129"], count["all"]) == (1, 1, 127, 128, 129, n)
        assert MR.list_of(*MR.MASKS["m1_first"](n, w))[0] == 0 and MR.list_of(*MR.MASKS["m1_last"](n, w))[0] == n - 1
        seg, _ = MR.empty_segment(n, w)
        assert np.all(seg[64:96] == 1) and np.all(seg[32:64] == 0) and np.all(seg[96:128] == 0)
        tile, _ = MR.empty_tile(n, w)
        assert np.all(tile[128:256] == 1) and np.all(tile[:128] == 0) and np.all(tile[256:384] == 0)
        assert 0.25 * n < count["random30"] < 0.35 * n
        mixed, values = MR.mixed_bytes(n, w)
        assert values == 5 and set(np.unique(mixed).tolist()) == {0, 1, 2, 31, 32, 255}
        assert np.array_equal(MR.list_of(mixed, 5), np.flatnonzero((mixed == 0) | (mixed == 2)))


def test_python_host_signatures():
    sig = inspect.signature(R.NeuralRenderer.render_masked).parameters
    assert list(sig) == ["self", "mask", "values", "rgba8", "rgb"]
    assert (sig["values"].default, sig["rgba8"].default, sig["rgb"].default) == (1, None, None)
    sig = inspect.signature(R.NeuralRenderer.reproject_rerender).parameters
    assert list(sig) == ["self", "dst_pos", "dst_rot", "rerender", "fill", "acc_min"] and sig["rerender"].default == "holes"
    assert list(inspect.signature(R.NeuralRenderer.reproject).parameters) == ["self", "dst_pos", "dst_rot", "fill", "acc_min"]      # as it was
    assert R.RERENDER_VALUES == {None: 0, "holes": 1, "unsourced": 5}


def test_cli_accepts_rerender_only_with_reproject(lib):
    cli = adanerf_amd.build.build_cli()
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--rerender holes|unsourced" in usage
    for bad in ("x", "hole", "", "1"):
        out = subprocess.run([cli, "m", "--reproject", "3", "--rerender", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "--rerender must be holes or unsourced" in out.stdout, bad
    out = subprocess.run([cli, "m", "--rerender"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "missing value after --rerender" in out.stdout
    for alone in (["--rerender", "holes"], ["--rerender", "unsourced", "--reproject", "1"], ["--reproject", "1", "--rerender", "holes"]):
        out = subprocess.run([cli, "m"] + alone, capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "only with --reproject K, K > 1" in out.stdout, alone
    for good in (["--reproject", "3", "--rerender", "holes"], ["--rerender", "unsourced", "--reproject", "2"]):
        out = subprocess.run([cli, os.path.join(str(ROOT), "no_such_model")] + good + ["--dry-run", "--frames", "1"], capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and "config.ini" in out.stdout and "Argument parsing failed" not in out.stdout, good


def test_evaluator_accepts_rerender_only_with_reproject_stride(tmp_path):
    from adanerf_amd import evaluate as E
    ap = E.build_parser()
    assert ap.parse_args(["m", "d"]).rerender is None
    a = ap.parse_args(["m", "d", "--reproject-stride", "3", "--rerender", "unsourced"])
    assert a.reproject_stride == 3 and a.rerender == "unsourced"
    with pytest.raises(SystemExit):
        ap.parse_args(["m", "d", "--rerender", "all"])
    with pytest.raises(SystemExit):
        E.main(["m", "d", "--rerender", "holes"])
    sig = inspect.signature(E.evaluate).parameters
    assert sig["rerender"].default is None
    for kw in (dict(rerender="holes"), dict(rerender="all", reproject_stride=2), dict(rerender=1, reproject_stride=2)):
        with pytest.raises(ValueError):
            E.evaluate(str(tmp_path / "no_model"), str(tmp_path / "no_dataset"), **kw)
    # the summary: keys of a run without the option, plus the two new ones when a warped record carries the re-rendered score
    plain = [dict(frame=0, samples_per_ray=4.0, ms=1.0, mse=0.01, psnr=20.0, warped=False),
             dict(frame=1, mse=0.02, psnr=17.0, warped=True, hole_fraction=0.1)]
    again = [plain[0], dict(plain[1], rerendered_fraction=0.1, mse_rerendered=0.001, psnr_rerendered=30.0)]
    s0, s1 = E.summarise(plain, False), E.summarise(again, False)
    assert sorted(s1) == sorted(list(s0) + ["mean_psnr_warped_rerendered", "mean_rerendered_fraction"])
    assert all(s1[k] == s0[k] for k in s0) and (s1["mean_psnr_warped_rerendered"], s1["mean_rerendered_fraction"]) == (30.0, 0.1)
