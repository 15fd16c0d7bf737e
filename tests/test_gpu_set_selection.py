"""adanerf_set_selection on the GPU: after a change of the sample budget N and / or the selection threshold a context must be
indistinguishable from a context created with those two options -- every output, every selection buffer, adanerf_info and the sample
total, byte for byte (the library is deterministic, so there is no tolerance anywhere in this file).  Frame: 97 x 61 = 5 917 rays, no
multiple of 32, 128 or the 256-sample shading tile.  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

W, H = 97, 61
EINVAL, EUNSUPPORTED = -1, -4
GUARD_FROM_NONE = 0


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """name -> (fixture arrays, model directory), written here from the seeded scenes and weights of the golden fixtures"""
    out = {}
    for name in ("classroom_n8_thr02", "syn_w40_w70_skip1", "classroom_pdf_n8"):
        z, meta, sc = load_case(name)
        d = str(tmp_path_factory.mktemp("sel_" + name))
        O.write_model_dir(d, sc, case_weights(meta))
        out[name] = (z, d)
    return out


class Ctx:
    """A renderer with every output attached, and a snapshot of all a frame leaves behind."""

    def __init__(self, d, z, n, thr, w=W, h=H, **kw):
        self.r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=kw.pop("batch_size", -1)), num_samples=n, threshold=thr, **kw)
        self.r.init()
        self.r.set_camera(z["pose"], z["rot"])
        nl = self.r.info.rays_local
        self.aux = [self.r.empty((nl,), np.float32) for _ in range(3)]
        self.r.set_aux_outputs(self.aux[0], self.aux[1])
        self.r.set_disp_output(self.aux[2])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.r.close()

    def frame(self):
        r = self.r
        for a in self.aux:      # a ray the frame does not write must not pass for equal by accident
            a.upload(np.full(a.shape, -7.0, np.float32))
        rgb, rgba, st = r.render_numpy()
        info = r.refresh_info()
        nl, nb = info.rays_local, info.batch_rays
        last = nl - ((nl - 1) // nb) * nb if nl else 0      # the buffers hold the frame's last batch
        out = dict(rgba=rgba, rgb=rgb, depth=self.aux[0].numpy(), acc=self.aux[1].numpy(), disp=self.aux[2].numpy(),
                   counts=r.buffer(R.BUF_RAY_COUNTS, np.int32, (last,)), offsets=r.buffer(R.BUF_RAY_OFFSETS, np.int32, (last,)),
                   total=r.buffer(R.BUF_TOTAL, np.int32, (1,)), info=np.frombuffer(bytes(info), np.uint8).copy(),
                   total_samples=np.int64(st.total_samples), refined=np.int64(st.rays_refined))
        if not info.dense:      # dense mode: keys are implicit and the weights are the oracle buffer; neither array is written
            s = int(out["total"][0])
            out["key"] = r.buffer(R.BUF_SAMPLE_KEY, np.uint32, (s,))
            out["w"] = r.buffer(R.BUF_SAMPLE_W, np.float32, (s,))
        return out


def same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def fresh(d, z, n, thr, **kw):
    with Ctx(d, z, n, thr, **kw) as c:
        return c.frame()


WALK = [(4, 0.35), (16, 0.05), (17, 0.05), (40, 0.1), (128, 0.0), (8, 0.2)]


@pytest.mark.parametrize("sampling,precision", [("split", "bf16"), ("fp32", "bf16"), ("fp16", "bf16"), ("split", "fp32")])
def test_walk_through_every_dispatch_branch(models, sampling, precision):
    """(8, 0.2) -> smaller N -> the fused selection's upper edge -> the first N on select_kernel (buffers grow) -> wave-per-ray compositing
    -> dense (implicit keys, oracle buffer as weights) -> back.  After every step: a context created with that pair; at the end also the
    first frame's own bytes."""
    z, d = models["classroom_n8_thr02"]
    kw = dict(sampling=sampling, precision=precision)
    with Ctx(d, z, 8, 0.2, **kw) as c:
        first = c.frame()
        same(first, fresh(d, z, 8, 0.2, **kw), "start")
        assert len(np.unique(first["counts"])) > 1 and 1 <= first["counts"].min() and first["counts"].max() <= 8      # the threshold does select
        for n, thr in WALK:
            info = c.r.set_selection(n, thr)
            assert (info.num_samples, info.threshold, info.dense) == (n, np.float32(thr), int(thr == 0)) and c.r.info is info
            got = c.frame()
            same(got, fresh(d, z, n, thr, **kw), "after set_selection(%d, %g)" % (n, thr))
            assert got["counts"].max() <= n
        same(got, first, "back at (8, 0.2)")


GUARD = dict(sampling="guarded", precision="bf16", guard_eps=1e-2, guard_eps_pair=1.5e-2, guard_cache=False)      # the header's default band


def test_guarded_mode_follows_the_pair(models):
    """Explicit bounds and no calibration record, so nothing calibrates: frames and re-evaluated rays per frame equal the fresh guarded
    context's (the audit starts over with the pair, as the fresh context's does); N = 24 leaves the fused path, where the mode is the
    split engine alone."""
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z, 8, 0.2, **GUARD) as c:
        a0 = c.frame()
        assert 0 < a0["refined"] < W * H
        same(a0, fresh(d, z, 8, 0.2, **GUARD), "guarded start")
        c.frame()      # the audit moves on; a change must start it over
        for n, thr in ((4, 0.3), (8, 0.2)):
            c.r.set_selection(n, thr)
            got = c.frame()
            same(got, fresh(d, z, n, thr, **GUARD), "guarded (%d, %g)" % (n, thr))
            assert got["refined"] > 0
        same(got, a0, "guarded, back at (8, 0.2)")
    with Ctx(d, z, 8, 0.2, **GUARD) as c:
        c.frame()
        c.r.set_selection(24, 0.2)
        got = c.frame()
        same(got, fresh(d, z, 24, 0.2, **GUARD), "guarded (24, 0.2)")
        same({k: v for k, v in got.items() if k not in ("info", "refined")},
             {k: v for k, v in fresh(d, z, 24, 0.2, sampling="split", precision="bf16").items() if k not in ("info", "refined")}, "guarded (24, 0.2) vs split")
        assert got["refined"] == 0


def test_guarded_calibration_key_follows_the_pair(models, tmp_path, monkeypatch):
    """Without bounds in the options the band comes from the new pair's record (or a calibration at the next guarded frame): the record's
    path is the fresh context's and the source is back to "none".  Nothing is rendered, so nothing calibrates."""
    z, d = models["classroom_n8_thr02"]
    monkeypatch.setenv("ADANERF_GUARD_CACHE_DIR", str(tmp_path / "cache"))
    kw = dict(sampling="guarded", precision="bf16")
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), num_samples=8, threshold=0.2, **kw) as r:
        start = r.guard_calibration_file()
        info = r.set_selection(4, 0.3)
        moved = r.guard_calibration_file()
        assert info.guard_calib_source == GUARD_FROM_NONE and info.guard_eps == 0.0
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), num_samples=4, threshold=0.3, **kw) as r:
        assert moved == r.guard_calibration_file() and moved != start and moved.startswith(str(tmp_path / "cache"))
        assert r.info.guard_calib_source == GUARD_FROM_NONE


def test_run_time_shaped_topology(models):
    z, d = models["syn_w40_w70_skip1"]
    with Ctx(d, z, 8, 0.2) as c:
        same(c.frame(), fresh(d, z, 8, 0.2), "start")
        for n, thr in ((12, 0.1), (20, 0.1)):
            c.r.set_selection(n, thr)
            same(c.frame(), fresh(d, z, n, thr), "run-time-shaped (%d, %g)" % (n, thr))


def test_batched_and_sharded(models):
    """batch_rays = 2048 and two ranks on the one GPU: after a change on both, the assembled frame is the unsharded fresh context's, and
    every rank equals a fresh rank."""
    z, d = models["classroom_n8_thr02"]
    for n, thr in ((8, 0.2), (20, 0.1), (4, 0.35)):
        want = fresh(d, z, n, thr)["rgba"]
        kw = dict(batch_size=2048, shard_world=2, strip_rows=8)
        ranks = [Ctx(d, z, 8, 0.2, shard_rank=k, **kw) for k in range(2)]
        try:
            parts = []
            for k, c in enumerate(ranks):
                c.frame()
                c.r.set_selection(n, thr)
                got = c.frame()
                same(got, fresh(d, z, n, thr, shard_rank=k, **kw), "rank %d at (%d, %g)" % (k, n, thr))
                pad = np.zeros((c.r.info.rays_local_max, 4), np.uint8)
                pad[:got["rgba"].shape[0]] = got["rgba"]
                parts.append(pad)
            r0 = ranks[0].r
            img = r0.empty((W * H, 4), np.uint8)
            r0.assemble_strips(r0.to_device(np.concatenate(parts)), img)
            r0.sync()
            assert np.array_equal(img.numpy(), want), (n, thr)
        finally:
            for c in ranks:
                c.r.close()


def test_keep_semantics_and_failures(models):
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z, 8, 0.2) as c:
        lib, h = c.r.lib, c.r.handle
        before = c.frame()
        assert lib.adanerf_set_selection(h, 0, -1.0) == 0
        same(c.frame(), before, "(0, -1) is a no-op")
        assert lib.adanerf_set_selection(h, 0, 0.3) == 0      # only the threshold moves
        same(c.frame(), fresh(d, z, 8, 0.3), "(0, 0.3)")
        assert lib.adanerf_set_selection(h, 5, -1.0) == 0     # only N moves
        same(c.frame(), fresh(d, z, 5, 0.3), "(5, -1)")
        held = c.frame()
        # what adanerf_create refuses, with its code and message; then the context renders as before
        for n, thr, code in ((129, 0.2, EINVAL), (8, float("nan"), EINVAL), (8, 0.0, EUNSUPPORTED), (0, 0.0, EUNSUPPORTED)):
            assert lib.adanerf_set_selection(h, n, thr) == code, (n, thr)
            msg = lib.adanerf_last_error(h).decode()
            assert len(msg) > 10, (n, thr, msg)
            if not math.isnan(thr):
                with pytest.raises(R.AdaNeRFError) as e:
                    adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), num_samples=n or 5, threshold=thr).init()
                assert msg in str(e.value) and "(%d)" % code in str(e.value)
            same(c.frame(), held, "after the refused (%s, %s)" % (n, thr))
        with pytest.raises(R.AdaNeRFError):
            c.r.set_selection(200, None)
        assert (c.r.refresh_info().num_samples, c.r.info.threshold) == (5, np.float32(0.3))
    # the inverse-CDF sampler: adanerf_create ignores options.threshold, so a threshold is refused; N is the override create honours
    z, d = models["classroom_pdf_n8"]
    with Ctx(d, z, 8, -1.0) as c:
        assert c.r.info.sampler_mode == R.SAMPLER_PDF
        before = c.frame()
        assert c.r.lib.adanerf_set_selection(c.r.handle, 8, 0.2) == EUNSUPPORTED
        assert "threshold" in c.r.lib.adanerf_last_error(c.r.handle).decode()
        same(c.frame(), before, "PDF sampler after the refused threshold")
        c.r.set_selection(6, None)
        same(c.frame(), fresh(d, z, 6, -1.0), "PDF sampler, N = 6")


def test_no_leak_no_creep(models):
    """200 alternating changes with a frame each: the device's free memory after the first two rounds and after the last is the same."""
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z, 8, 0.2) as c:
        out = c.r.empty((W * H, 4), np.uint8)
        base, total = None, {}
        for i in range(200):
            n, thr = ((4, 0.3), (16, 0.05))[i & 1]
            c.r.set_selection(n, thr)
            st = c.r.render(out, None, stats=(i < 2 or i >= 198))
            if st:
                total.setdefault((n, thr), []).append(int(st.total_samples))
            if i == 1:
                c.r.sync()
                base = free_bytes()
        c.r.sync()
        assert free_bytes() == base
        assert all(len(v) == 2 and v[0] == v[1] for v in total.values()), total      # round 100 selects what round 1 selected
        same(c.frame(), fresh(d, z, 16, 0.05), "after 200 changes")


def _cli_rotation(yaw, pitch):
    """Camera::getRotMatrix of the C++ host, operation for operation in float64"""
    deg = 3.14159265358979323846 / 180.0
    y, p = yaw * deg, pitch * deg
    f = [math.cos(y) * math.cos(p), math.sin(y) * math.cos(p), math.sin(p)]
    n = math.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
    f = [v / n for v in f]
    rt = [f[1] * 1.0 - f[2] * 0.0, f[2] * 0.0 - f[0] * 1.0, 0.0]
    n = math.sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2])
    rt = [v / n for v in rt]
    up = [rt[1] * f[2] - rt[2] * f[1], rt[2] * f[0] - rt[0] * f[2], rt[0] * f[1] - rt[1] * f[0]]
    return np.array([[rt[i], up[i], -f[i]] for i in range(3)], np.float64).astype(np.float32)


def _bmp_pixels(path, w, h):
    bmp = open(path, "rb").read()
    off = int.from_bytes(bmp[10:14], "little")
    row_bytes = (w * 3 + 3) & ~3
    px = np.frombuffer(bmp[off:off + row_bytes * h], dtype=np.uint8).reshape(h, row_bytes)[:, :w * 3].reshape(h, w, 3)
    return px[::-1, :, ::-1].reshape(-1, 3)


def test_cli_script_tokens_equal_the_python_host(models, tmp_path):
    """`adanerf --script` with `n` / `thr` tokens, written with -w: out.bmp holds a session's last frame, so the session is replayed up to
    each of its lines in turn; every one of those frames equals what NeuralRenderer.set_selection renders at the logged pose."""
    z, d = models["classroom_n8_thr02"]
    exe = adanerf_amd.build.build_cli()
    lines = ["thr 0.3 +w", "n 4", "n 20 thr 0.05 -w", "thr 0 n 128"]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="bf16") as r:
        for k in range(1, len(lines) + 1):
            script = tmp_path / ("session%d.txt" % k)
            script.write_text("\n".join(lines[:k]) + "\n")
            out = subprocess.run([exe, d, "-s", str(W), str(H), "-w", "--script", str(script), "--log-camera"], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            cam = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
            assert len(cam) == k
            pos = np.array([float(v) for v in cam[-1][3:6]], np.float32)
            # this line's tokens are one request to the library, as the host makes it before the frame
            words = lines[k - 1].split()
            n = [int(words[i + 1]) for i, t in enumerate(words) if t == "n"]
            thr = [float(words[i + 1]) for i, t in enumerate(words) if t == "thr"]
            r.set_selection(n[-1] if n else None, thr[-1] if thr else None)
            r.set_camera(pos, _cli_rotation(float(cam[-1][7]), float(cam[-1][9])))
            _, rgba, _ = r.render_numpy()
            assert np.array_equal(_bmp_pixels(os.path.join(d, "out.bmp"), W, H), rgba[:, :3]), "frame %d (%s)" % (k, lines[k - 1])
    os.remove(os.path.join(d, "out.bmp"))
    bad = tmp_path / "bad.txt"
    bad.write_text("n 500\n")      # parses; the library refuses the pair when the frame is rendered
    out = subprocess.run([exe, d, "-s", str(W), str(H), "--script", str(bad)], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "numRaymarchSamples must be in 1..128" in out.stdout


def test_evaluator_sweep_equals_plain_runs(tmp_path):
    """evaluate(..., sweep_thresholds=[0.1, 0.3]) on a synthetic 12 x 10 dataset: per setting, the records and means of a plain run over a
    model directory whose config.ini carries that threshold."""
    import dataclasses
    from adanerf_amd.evaluate import evaluate, sweep_dir_name
    from adanerf_amd.png import read_png, write_png
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    wts = O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3)
    w, h = 12, 10
    dirs = {}
    for thr in (0.2, 0.1, 0.3):
        dirs[thr] = str(tmp_path / ("model_t%g" % thr))
        O.write_model_dir(dirs[thr], dataclasses.replace(sc, threshold=thr), wts)
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[w, h], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    poses = [(np.array(sc.view_cell_center, np.float32), O.camera_rotation(100.0, 0.0)),
             (np.array(sc.view_cell_center, np.float32) + np.float32([0.1, 0.05, -0.02]), O.camera_rotation(60.0, -8.0))]
    frames = []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        write_png(str(ds / "test" / ("%05d.png" % i)), np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    out = tmp_path / "pred"
    summary, results = evaluate(dirs[0.2], str(ds), "test", str(out), precision="bf16", quiet=True, metrics=("psnr", "flip"), sweep_thresholds=[0.1, 0.3])
    assert sorted(summary) == ["frames", "sweep"] and summary["frames"] == 2 and len(summary["sweep"]) == 2 and len(results) == 4
    for k, thr in enumerate((0.1, 0.3)):
        plain_dir = tmp_path / ("plain_t%g" % thr)
        s1, r1 = evaluate(dirs[thr], str(ds), "test", str(plain_dir), precision="bf16", quiet=True, metrics=("psnr", "flip"))
        e = summary["sweep"][k]
        assert sorted(e) == ["mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray", "num_samples", "threshold"]
        assert (e["num_samples"], e["threshold"]) == (8, thr) and e["mean_ms"] > 0
        for key in ("mean_psnr", "mean_mse", "mean_samples_per_ray", "mean_flip"):
            assert e[key] == s1[key], (thr, key)
        for a, b in zip(results[2 * k:2 * k + 2], r1):
            assert (a["num_samples"], a["threshold"]) == (8, thr)
            assert all(a[key] == b[key] for key in ("frame", "image", "samples_per_ray", "mse", "psnr", "flip")), (thr, a, b)
        sub = out / sweep_dir_name(8, thr)
        for name in ("00000.png", "00001.png", "00000_flip.png", "00001_flip.png"):
            assert np.array_equal(read_png(str(sub / name)), read_png(str(plain_dir / name))), (thr, name)
    assert sorted(os.listdir(out)) == ["n8_t0.1", "n8_t0.3"]
    # both axes: N outermost
    s2, r2 = evaluate(dirs[0.2], str(ds), "test", None, precision="bf16", quiet=True, sweep_thresholds=[0.3, 0.1], sweep_samples=[4, 16])
    assert [(e["num_samples"], e["threshold"]) for e in s2["sweep"]] == [(4, 0.3), (4, 0.1), (16, 0.3), (16, 0.1)] and len(r2) == 8
    assert all("mean_flip" not in e for e in s2["sweep"])
