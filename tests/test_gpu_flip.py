"""adanerf_flip (csrc/k_flip.hip.hpp: flip_kernel, one 32 x 32 tile per workgroup, + flip_mean_kernel) against the float64 restatement
tests/flip_reference.py on the fixtures of tools/gen_flip_golden.py, which pin both to the reference's own FLIP
(src/util/flip_loss.py:61-105 as src/evaluate.py:120-145 calls it).

Bound.  Each fixture stores ``ref_fp32_residual`` / ``ref_fp32_residual_mean``: how far the REFERENCE's fp32 map / mean sit from the
float64 restatement, i.e. the rounding error of the same computation in fp32.  The device does the same fp32 work in another order, so
its map must stay within 4 x that figure of the restatement, its mean within 4 x the mean's.  The measured maxima go to
$ADANERF_MEASURED_LOG (profiles/flip_measured.log).

Cases: 1x1, 7x5 (smaller than either radius), 130x9 (one dimension below the radius), 32x32 and 33x33 (the tile and one more), 37x23,
97x61 (several tiles, ragged), 64x48 at 30 pixels per degree (radii 5 / 4: run-time radii), 45x41 at 140 (radii 19 / 18, the largest
supported: the only case whose LDS image exceeds 64 KB).  Further: identical images give exact zeros; two calls give the same bits; a NaN
pixel reaches the map only within the larger filter radius (a clamp at the wrong stage, or tiles reading each other's halo, would show);
every output lies between two 4 KiB canary regions; each invalid argument is refused on the host; the evaluator reports the same
number as NeuralRenderer.flip.  Contexts come from a golden scene; the networks do not matter here."""
import ctypes as C
import json

import numpy as np
import pytest

import adanerf_oracle as O
import flip_reference as F
from conftest import load_case, record

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

PAD = 4096
EINVAL = -1


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    adanerf_amd.build_library()
    z, meta, sc = load_case("synthetic_fixed8")
    d = str(tmp_path_factory.mktemp("flip_model"))
    O.write_model_dir(d, sc, O.synthetic_weights(1))
    return d, sc


@pytest.fixture(scope="module")
def r(model):
    with R.NeuralRenderer(R.Settings(model[0], 64, 48), precision="fp32") as ren:
        yield ren


class Guarded:
    """A device output of `nbytes` between two 4 KiB canary regions; body and canaries start as 0xA5 bytes (the sentinel)."""

    def __init__(self, r, nbytes):
        self.r, self.n = r, int(nbytes)
        self.buf = R.DeviceArray(r, (PAD + self.n + PAD,), np.uint8)
        self.buf.upload(np.full(PAD + self.n + PAD, 0xA5, np.uint8))
        self.ptr = self.buf.ptr + PAD

    def body(self, what, dtype=np.uint8):
        a = self.buf.numpy()
        assert (a[:PAD] == 0xA5).all(), what + ": wrote before the buffer"
        assert (a[PAD + self.n:] == 0xA5).all(), what + ": wrote past the buffer"
        out = a[PAD:PAD + self.n].copy().view(dtype)
        self.buf.free()
        return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def device_flip(r, test, ref, ppd=None, want_map=True, want_mean=True, what="flip"):
    """(mean or None, map [h, w] fp32 or None) of two [h, w, 3] images; the map is written into a guarded exact-size buffer"""
    h, w = test.shape[:2]
    ins = [R.DeviceArray(r, (h * w, 3), np.float32).upload(np.ascontiguousarray(a, np.float32).reshape(-1, 3)) for a in (test, ref)]
    g = Guarded(r, h * w * 4) if want_map else None
    mean = r.flip_device(ins[0], ins[1], w, h, ppd, g.ptr if g else None, mean=want_mean)
    r.sync()
    m = g.body(what, np.float32).reshape(h, w) if g else None
    for b in ins:
        b.free()
    return mean, m


@pytest.mark.parametrize("name", F.FIXTURES)
def test_fixture_against_fp64(r, name):
    z = F.load_fixture(name)
    meta = z["meta"]
    mean, m = device_flip(r, z["test"], z["ref"], z["ppd_arg"], what=name)
    err = float(np.max(np.abs(m.astype(np.float64) - z["map64"])))
    err_mean = abs(mean - z["mean64"])
    vs_ref = float(np.max(np.abs(m.astype(np.float64) - z["ref_map"].astype(np.float64))))
    record("flip_fixture", fixture=name, radii=meta["radii"], map_err=err, map_bound=4 * meta["ref_fp32_residual"], mean_err=err_mean,
           mean_bound=4 * meta["ref_fp32_residual_mean"], map_vs_reference_fp32=vs_ref, mean=mean)
    print("%s: map %.3e (bound %.3e)  mean %.3e (bound %.3e)  vs reference fp32 %.3e" %
          (name, err, 4 * meta["ref_fp32_residual"], err_mean, 4 * meta["ref_fp32_residual_mean"], vs_ref))
    assert np.isfinite(m).all()
    assert err <= 4 * meta["ref_fp32_residual"], (name, err, meta["ref_fp32_residual"])
    assert err_mean <= 4 * meta["ref_fp32_residual_mean"], (name, err_mean, meta["ref_fp32_residual_mean"])


def test_identical_images_give_exact_zeros(r):
    z = F.load_fixture("flip_97x61")
    mean, m = device_flip(r, z["test"], z["test"])
    assert mean == 0.0 and not m.any()


def test_two_calls_give_the_same_bits(r):
    z = F.load_fixture("flip_97x61")
    a, b = device_flip(r, z["test"], z["ref"]), device_flip(r, z["test"], z["ref"])
    assert same_bits(a[1], b[1]) and same_bits(np.float32(a[0]), np.float32(b[0]))


def test_a_nan_pixel_stays_within_the_filter_radius(r):
    z = F.load_fixture("flip_64x48_ppd30")      # its images, at the default pixels per degree: radii 10 and 9
    radius = max(F.radii(F.DEFAULT_PPD))
    py, px = 30, 33                              # next to a tile corner: its neighbourhood spans four workgroups
    clean_mean, clean = device_flip(r, z["test"], z["ref"])
    t = z["test"].copy()
    t[py, px, 1] = np.nan
    mean, m = device_flip(r, t, z["ref"])
    far = np.maximum(np.abs(np.arange(48)[:, None] - py), np.abs(np.arange(64)[None, :] - px)) > radius
    assert far.sum() > 1000
    assert same_bits(m[far], clean[far])
    assert not np.isfinite(m[py, px])
    assert np.isnan(mean) and np.isfinite(clean_mean)
    assert same_bits(np.isnan(m), np.isnan(F.flip_map(t, z["ref"])))      # and exactly where the restatement has it


def test_optional_outputs(r):
    z = F.load_fixture("flip_37x23")
    mean, m = device_flip(r, z["test"], z["ref"])
    only_mean, none = device_flip(r, z["test"], z["ref"], want_map=False)
    assert none is None and same_bits(np.float32(only_mean), np.float32(mean))
    no_mean, only_map = device_flip(r, z["test"], z["ref"], want_mean=False)      # device_flip syncs before it reads the map
    assert no_mean is None and same_bits(only_map, m)


def test_host_arrays_and_flat_layout(r):
    z = F.load_fixture("flip_37x23")
    mean, m = device_flip(r, z["test"], z["ref"])
    mean2, m2 = r.flip(z["test"], z["ref"], return_map=True)
    assert same_bits(m2, m) and mean2 == mean
    assert r.flip(z["test"].reshape(-1, 3), z["ref"].reshape(-1, 3), width=37, height=23) == mean
    with pytest.raises(ValueError):
        r.flip(z["test"].reshape(-1, 3), z["ref"].reshape(-1, 3), width=36, height=23)


@pytest.mark.parametrize("what,kw", [("test image NULL", dict(test=None)), ("reference image NULL", dict(ref=None)), ("width 0", dict(w=0)),
                                     ("width negative", dict(w=-3)), ("height 0", dict(h=0)), ("height negative", dict(h=-1)),
                                     ("width * height = 2^32", dict(w=65536, h=65536)), ("width * height = 2^30 + 2^15", dict(w=32768, h=32769)),
                                     ("5 pixels per degree", dict(ppd=5.0)), ("200 pixels per degree", dict(ppd=200.0)),
                                     ("NaN pixels per degree", dict(ppd=float("nan")))])
def test_invalid_arguments_are_refused_on_the_host(r, what, kw):
    """refused before anything touches the device: the image pointers are never read (the sizes named here are not the buffers')"""
    a = R.DeviceArray(r, (16, 3), np.float32).upload(np.zeros((16, 3), np.float32))
    g = Guarded(r, 64)
    mean = C.c_float(-7.0)
    args = dict(test=a.ptr, ref=a.ptr, w=4, h=4, ppd=0.0)
    args.update(kw)
    rc = r.lib.adanerf_flip(r.handle, args["test"], args["ref"], args["w"], args["h"], args["ppd"], g.ptr, C.byref(mean))
    assert rc == EINVAL, what
    msg = r.lib.adanerf_last_error(r.handle).decode()
    assert "adanerf_flip" in msg and len(msg) > 20, (what, msg)
    r.sync()
    assert (g.body(what) == 0xA5).all() and mean.value == -7.0, what
    assert r.lib.adanerf_flip(None, a.ptr, a.ptr, 4, 4, 0.0, None, None) == EINVAL
    a.free()


def test_evaluator_reports_flip(model, tmp_path):
    from adanerf_amd.evaluate import evaluate
    from adanerf_amd.png import read_png, write_png
    d, sc = model
    w, h = 64, 48
    poses = [(np.array(sc.view_cell_center, np.float32), O.camera_rotation(100.0, 0.0)),
             (np.array(sc.view_cell_center, np.float32) + np.float32([0.1, 0.05, -0.02]), O.camera_rotation(60.0, -8.0))]
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[w, h], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    bump = (12 * ((xx // 8 + yy // 8) % 2) + (xx % 5 == 0) * 20).astype(np.int16)      # the fixed perturbation: a checkerboard and thin lines
    frames, rendered, truth = [], [], []
    with R.NeuralRenderer(R.Settings(d, w, h), precision="fp32") as ren:
        for i, (pose, rot) in enumerate(poses):
            m = np.eye(4, dtype=np.float32)
            m[:3, :3], m[:3, 3] = rot, pose
            frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
            ren.set_camera(pose, rot)
            rgb, rgba, _ = ren.render_numpy()
            gt8 = np.clip(rgba[:, :3].reshape(h, w, 3).astype(np.int16) + bump[:, :, None], 0, 255).astype(np.uint8)
            write_png(str(ds / "test" / ("%05d.png" % i)), gt8)
            rendered.append(rgb.copy())
            truth.append(gt8.astype(np.float32).reshape(-1, 3) / 255.0)
        json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
        expect = [ren.flip(rendered[i], truth[i], w, h, return_map=True) for i in range(2)]
    out = tmp_path / "pred"
    summary, results = evaluate(d, str(ds), "test", str(out), precision="fp32", quiet=True, metrics=("psnr", "flip"))
    assert [x["flip"] for x in results] == [e[0] for e in expect]
    assert all(0.01 < x["flip"] < 1.0 for x in results)
    assert summary["mean_flip"] == float(np.mean([e[0] for e in expect])) and "mean_psnr" in summary
    for i in range(2):
        png = read_png(str(out / ("%05d_flip.png" % i)))
        assert png.shape == (h, w, 1) and np.array_equal(png[:, :, 0], np.rint(expect[i][1] * 255.0).astype(np.uint8))
    # default metrics: the records and the summary of the evaluator before FLIP, key for key
    s0, r0 = evaluate(d, str(ds), "test", None, precision="fp32", quiet=True)
    assert sorted(s0) == ["frames", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    assert all(sorted(x) == ["frame", "image", "ms", "mse", "psnr", "samples_per_ray"] for x in r0)
    assert [x["psnr"] for x in r0] == [x["psnr"] for x in results]
    with pytest.raises(ValueError):
        evaluate(d, str(ds), "test", None, quiet=True, metrics=("ssim",))
