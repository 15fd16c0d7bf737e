"""adanerf_present on the GPU: every case is exact equality with tests/present_reference.py (the integer definition in
include/adanerf_hip.h).  Images are random bytes with 0 and 255 planted; a canary sits before and after the destination and the source
is checked unmodified.  The kernel writes four adjacent pixels with one 16-byte store where the address allows, so destination widths
1, 2, 3, 5 and 67 and a destination offset by one pixel from a 16-byte boundary are cases of their own.  Run with `pytest -m gpu` on an
MI355X box."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import present_reference as P
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL = -1
PAD = 64      # canary pixels on either side of the destination


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    z, meta, sc = load_case("classroom_n8_thr02")
    d = str(tmp_path_factory.mktemp("present_model"))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, d


@pytest.fixture(scope="module")
def ctx(model):
    """one small context for the whole module: adanerf_present is independent of its frame size"""
    z, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 12)) as r:
        yield r


def image(w, h, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    flat = img.reshape(-1)
    flat[rng.integers(0, flat.size, max(2, flat.size // 7))] = 0
    flat[rng.integers(0, flat.size, max(2, flat.size // 7))] = 255
    flat[0], flat[-1] = 255, 0
    return img


def run(r, src, dw, dh, flags=0, offset_px=0):
    """present src to dw x dh through the C ABI, the destination `offset_px` pixels past an allocation boundary with canaries around it;
    returns uint8 [dh, dw, 4]"""
    sh, sw = src.shape[:2]
    d_src = R.DeviceArray(r, src.shape, np.uint8).upload(src)
    total = PAD + offset_px + dw * dh + PAD
    canary = np.full((total, 4), 0xA5, np.uint8)
    d_dst = R.DeviceArray(r, (total, 4), np.uint8).upload(canary)
    try:
        first = PAD + offset_px
        rc = r.lib.adanerf_present(r.handle, d_src.ptr, sw, sh, d_dst.ptr + 4 * first, dw, dh, flags)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        r.sync()
        got = d_dst.numpy()
        assert np.all(got[:first] == 0xA5) and np.all(got[first + dw * dh:] == 0xA5), "wrote outside the destination"
        assert np.array_equal(d_src.numpy(), src), "source modified"
        return got[first:first + dw * dh].reshape(dh, dw, 4)
    finally:
        d_src.free()
        d_dst.free()


def check(r, sw, sh, dw, dh, flags=0, offset_px=0, seed=0):
    src = image(sw, sh, seed + 1000 * sw + sh)
    got = run(r, src, dw, dh, flags, offset_px)
    want = P.present(src, dw, dh, flags)
    assert np.array_equal(got, want), "%dx%d -> %dx%d flags %d offset %d: %d of %d bytes differ" % (
        sw, sh, dw, dh, flags, offset_px, int(np.count_nonzero(got != want)), want.size)
    return src, got


SIZES = [(1, 1, 5, 3), (7, 5, 14, 10), (7, 5, 13, 11), (97, 61, 64, 48), (33, 9, 40, 7), (8, 8, 8, 20), (3, 3, 16384, 1), (1, 16384, 2, 2),
         (800, 800, 1920, 1080)]


@pytest.mark.parametrize("sw,sh,dw,dh", SIZES, ids=["%dx%d-%dx%d" % s for s in SIZES])
def test_sizes_by_the_rule(ctx, sw, sh, dw, dh):
    check(ctx, sw, sh, dw, dh)


def test_the_rule_is_the_reference_s(ctx):
    """linear on both axes if the destination is wider, nearest otherwise -- whatever the heights do"""
    assert P.uses_linear(33, 40) and not P.uses_linear(8, 8) and not P.uses_linear(97, 64)
    for sw, sh, dw, dh in ((33, 9, 40, 7), (8, 8, 8, 20), (97, 61, 64, 48), (7, 5, 14, 10)):
        src = image(sw, sh, 5)
        by_rule = run(ctx, src, dw, dh, 0)
        forced = run(ctx, src, dw, dh, P.LINEAR if dw > sw else P.NEAREST)
        other = P.present(src, dw, dh, P.NEAREST if dw > sw else P.LINEAR)
        assert np.array_equal(by_rule, forced) and not np.array_equal(by_rule, other), (sw, sh, dw, dh)


@pytest.mark.parametrize("flags", [P.NEAREST, P.LINEAR], ids=["nearest", "linear"])
def test_equal_sizes_are_the_identity(ctx, flags):
    src, got = check(ctx, 7, 5, 7, 5, flags)
    assert np.array_equal(got, src)


@pytest.mark.parametrize("dw", [1, 2, 3, 5, 67])
@pytest.mark.parametrize("offset_px", [0, 1])
def test_ragged_widths_and_unaligned_destinations(ctx, dw, offset_px):
    """rows that start at every phase of a 16-byte boundary, groups cut short by the row end, both filters, both directions of y"""
    for sw, sh, dh in ((9, 7, 6), (131, 5, 9)):
        for flags in (P.NEAREST, P.LINEAR, P.LINEAR | P.FLIP_Y):
            check(ctx, sw, sh, dw, dh, flags, offset_px)


@pytest.mark.parametrize("offset_px", [1, 2, 3])
def test_aligned_width_at_every_pointer_phase(ctx, offset_px):
    check(ctx, 33, 9, 64, 12, P.LINEAR, offset_px)
    check(ctx, 33, 9, 64, 12, P.NEAREST | P.FLIP_Y, offset_px)


@pytest.mark.parametrize("flags", [P.FLIP_Y, P.FLIP_Y | P.NEAREST, P.FLIP_Y | P.LINEAR, P.NEAREST, P.LINEAR])
def test_flags(ctx, flags):
    for sw, sh, dw, dh in ((7, 5, 13, 11), (97, 61, 64, 48)):
        src, got = check(ctx, sw, sh, dw, dh, flags)
        if flags & P.FLIP_Y:
            assert np.array_equal(got[::-1], P.present(src, dw, dh, flags & ~P.FLIP_Y))


def test_refused_arguments(ctx):
    r = ctx
    src = R.DeviceArray(r, (8 * 8, 4), np.uint8).upload(np.zeros((64, 4), np.uint8))
    dst = R.DeviceArray(r, (16 * 16, 4), np.uint8).upload(np.full((256, 4), 7, np.uint8))
    try:
        call = lambda s, sw, sh, d, dw, dh, fl: r.lib.adanerf_present(r.handle, s, sw, sh, d, dw, dh, fl)
        assert call(src.ptr, 8, 8, dst.ptr, 16, 16, 0) == 0
        for args in ((src.ptr, 0, 8, dst.ptr, 16, 16, 0), (src.ptr, 8, 0, dst.ptr, 16, 16, 0), (src.ptr, 8, 8, dst.ptr, 0, 16, 0),
                     (src.ptr, 8, 8, dst.ptr, 16, 0, 0), (src.ptr, 8, 8, dst.ptr, 16, -3, 0),
                     (src.ptr, 16385, 1, dst.ptr, 16, 16, 0), (src.ptr, 1, 16385, dst.ptr, 16, 16, 0), (src.ptr, 8, 8, dst.ptr, 16385, 1, 0),
                     (src.ptr, 8, 8, dst.ptr, 1, 16385, 0),
                     (None, 8, 8, dst.ptr, 16, 16, 0), (src.ptr, 8, 8, None, 16, 16, 0),
                     (src.ptr, 8, 8, dst.ptr, 16, 16, P.NEAREST | P.LINEAR), (src.ptr, 8, 8, dst.ptr, 16, 16, P.NEAREST | P.LINEAR | P.FLIP_Y),
                     (dst.ptr, 8, 8, dst.ptr, 16, 16, 0),                       # the same start
                     (dst.ptr + 4 * 255, 1, 1, dst.ptr, 16, 16, 0),             # the source is the destination's last pixel
                     (dst.ptr, 16, 16, dst.ptr + 4 * 255, 1, 1, 0),
                     (dst.ptr, 8, 8, dst.ptr + 4 * 63, 8, 8, 0)):               # one pixel shared
            assert call(*args) == EINVAL, args
            assert "adanerf_present" in r.lib.adanerf_last_error(r.handle).decode()
        assert r.lib.adanerf_present(None, src.ptr, 8, 8, dst.ptr, 16, 16, 0) == EINVAL
        assert call(dst.ptr, 8, 8, dst.ptr + 4 * 64, 8, 8, 0) == 0               # adjacent ranges do not overlap
        r.sync()
        with pytest.raises(ValueError):
            r.present_device(src, 8, 8, dst, 16, 16, filter="cubic")
    finally:
        src.free()
        dst.free()


def test_two_calls_give_the_same_bytes(ctx):
    src = image(97, 61, 3)
    assert np.array_equal(run(ctx, src, 203, 117, 0), run(ctx, src, 203, 117, 0))


def test_python_render_then_present(model):
    z, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 64, 48, window_width=128, window_height=96)) as r:
        r.set_camera(z["pose"], z["rot"])
        _, rgba, _ = r.render_numpy()
        frame = rgba.reshape(48, 64, 4)
        assert len(np.unique(frame[:, :, :3])) > 16 and np.all(frame[:, :, 3] == 255)
        assert np.array_equal(r.present(), P.present(frame, 128, 96))                  # the window of the settings, linear by the rule
        assert np.array_equal(r.present(40, 30, flip_y=True), P.present(frame, 40, 30, P.FLIP_Y))
        assert np.array_equal(r.present(128, 96, filter="nearest"), P.present(frame, 128, 96, P.NEAREST))
        r.set_frame_size(32, 24)                                                       # dynamic resolution: the window stays
        assert (r.settings.window_width, r.settings.window_height) == (128, 96)
        with pytest.raises(R.AdaNeRFError):
            r.present()                                                                # no frame of the new size yet
        _, rgba, _ = r.render_numpy()
        assert np.array_equal(r.present(), P.present(rgba.reshape(24, 32, 4), 128, 96))


def _bmp(path, w, h):
    bmp = open(path, "rb").read()
    assert int.from_bytes(bmp[18:22], "little") == w and int.from_bytes(bmp[22:26], "little") == h, path
    off = int.from_bytes(bmp[10:14], "little")
    row_bytes = (w * 3 + 3) & ~3
    px = np.frombuffer(bmp[off:off + row_bytes * h], dtype=np.uint8).reshape(h, row_bytes)[:, :w * 3].reshape(h, w, 3)
    return np.ascontiguousarray(px[::-1, :, ::-1])      # top-down RGB


def _rgba(rgb):
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)


def test_cli_writes_the_window_image(model):
    z, d = model
    exe = adanerf_amd.build.build_cli()
    out = subprocess.run([exe, d, "-s", "64", "48", "-ws", "128", "96", "-w", "--write-window", "--frames", "1"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    try:
        frame = _bmp(os.path.join(d, "out.bmp"), 64, 48)
        window = _bmp(os.path.join(d, "out_window.bmp"), 128, 96)
        assert len(np.unique(frame)) > 16
        assert np.array_equal(window, P.present(_rgba(frame), 128, 96)[:, :, :3])
    finally:
        for name in ("out.bmp", "out_window.bmp"):
            if os.path.exists(os.path.join(d, name)):
                os.remove(os.path.join(d, name))


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


def test_cli_size_token_equals_fresh_contexts(model, tmp_path):
    """`adanerf --script` with a `size` token mid-replay, written with -w --write-window: out.bmp holds a session's last frame, so the
    session is replayed up to each of its lines in turn; every frame equals a fresh context's at that size and the logged pose, and the
    window image stays at the window's size."""
    z, d = model
    exe = adanerf_amd.build.build_cli()
    lines = ["+w", "size 32 24", "-w", "size 97 61 +d"]
    sizes = [(64, 48), (32, 24), (32, 24), (97, 61)]
    try:
        for k in range(1, len(lines) + 1):
            script = tmp_path / ("session%d.txt" % k)
            script.write_text("\n".join(lines[:k]) + "\n")
            out = subprocess.run([exe, d, "-s", "64", "48", "-ws", "80", "60", "-w", "--write-window", "--script", str(script), "--log-camera"],
                                 capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            cam = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
            assert len(cam) == k
            w, h = sizes[k - 1]
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
                r.set_camera(np.array([float(v) for v in cam[-1][3:6]], np.float32), _cli_rotation(float(cam[-1][7]), float(cam[-1][9])))
                _, rgba, _ = r.render_numpy()
            frame = _bmp(os.path.join(d, "out.bmp"), w, h)
            assert np.array_equal(frame, rgba[:, :3].reshape(h, w, 3)), "frame %d (%s)" % (k, lines[k - 1])
            assert np.array_equal(_bmp(os.path.join(d, "out_window.bmp"), 80, 60), P.present(_rgba(frame), 80, 60)[:, :, :3])
        bad = tmp_path / "bad.txt"
        bad.write_text("size 8192 4096\n")      # parses; the library refuses the size when the frame is rendered
        out = subprocess.run([exe, d, "-s", "64", "48", "--script", str(bad)], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "width*height must be < 2^25" in out.stdout
        # a share layout that cannot hold the size: 50 rows in strips of 8 over two shares
        bad.write_text("size 64 50\n")
        out = subprocess.run([exe, d, "-s", "64", "48", "--gpus", "2", "--same-device", "--sub-shares", "1", "--script", str(bad)],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "do not split into strips" in out.stdout
    finally:
        for name in ("out.bmp", "out_window.bmp"):
            if os.path.exists(os.path.join(d, name)):
                os.remove(os.path.join(d, name))


def test_evaluator_sweep_scales(tmp_path):
    """evaluate(..., sweep_scales=[0.5, 1]) on a synthetic 12 x 10 dataset: the scale-1 entry is the plain run scored from its 8-bit
    frame, the 0.5 entry's image is the reference presentation of the 6 x 5 frame a fresh context renders."""
    from adanerf_amd.evaluate import evaluate, psnr_from_mse, sweep_dir_name
    from adanerf_amd.png import read_png, write_png
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    w, h = 12, 10
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[w, h], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    poses = [(np.array(sc.view_cell_center, np.float32), O.camera_rotation(100.0, 0.0)),
             (np.array(sc.view_cell_center, np.float32) + np.float32([0.1, 0.05, -0.02]), O.camera_rotation(60.0, -8.0))]
    frames, gts = [], []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        gts.append(np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
        write_png(str(ds / "test" / ("%05d.png" % i)), gts[-1])
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    out, plain = tmp_path / "pred", tmp_path / "plain"
    summary, results = evaluate(md, str(ds), "test", str(out), precision="bf16", quiet=True, sweep_scales=[0.5, 1])
    s1, r1 = evaluate(md, str(ds), "test", str(plain), precision="bf16", quiet=True)
    assert sorted(s1) == ["frames", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    assert sorted(summary) == ["frames", "sweep"] and [e["scale"] for e in summary["sweep"]] == [0.5, 1.0] and len(results) == 4
    assert sorted(os.listdir(out)) == [sweep_dir_name(8, 0.2, 0.5), sweep_dir_name(8, 0.2, 1.0)] == ["n8_t0.2_s0.5", "n8_t0.2_s1"]
    for e in summary["sweep"]:
        assert sorted(e) == ["mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray", "num_samples", "scale", "threshold"]
    # scale 1: the plain run's frames, scored from the 8-bit image
    full = summary["sweep"][1]
    mses = []
    for i in range(2):
        img = read_png(str(plain / ("%05d.png" % i)))
        assert np.array_equal(read_png(str(out / "n8_t0.2_s1" / ("%05d.png" % i))), img)
        ref = gts[i].astype(np.float32).reshape(-1, 3) / 255.0
        mses.append(float(np.mean((img.reshape(-1, 3).astype(np.float32) / 255.0 - ref.astype(np.float64)) ** 2)))
        assert results[2 + i]["mse"] == mses[-1] and results[2 + i]["psnr"] == psnr_from_mse(mses[-1]) and results[2 + i]["scale"] == 1.0
        assert results[2 + i]["samples_per_ray"] == r1[i]["samples_per_ray"]
    assert full["mean_mse"] == float(np.mean(mses)) and full["mean_samples_per_ray"] == s1["mean_samples_per_ray"]
    # scale 0.5: a fresh 6 x 5 context's frame, presented to 12 x 10 by the reference
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, 6, 5)) as r:
        for i, (pose, rot) in enumerate(poses):
            r.set_camera(pose, rot)
            _, rgba, st = r.render_numpy()
            want = P.present(rgba.reshape(5, 6, 4), w, h)[:, :, :3]
            assert np.array_equal(read_png(str(out / "n8_t0.2_s0.5" / ("%05d.png" % i))), want), i
            assert results[i]["scale"] == 0.5 and results[i]["samples_per_ray"] == st.total_samples / 30.0
