"""adanerf_reproject on the GPU: every geometric case is exact equality with tests/reproject_reference.py (reproject_f32, the definition
in include/adanerf_hip.h in numpy float32) for all four outputs -- colour, depth, mask and the hole count.  Source images are random
bytes over a synthetic wall + box depth scene with far pixels of every kind planted; canaries sit before and after every output and
the sources are checked unmodified.  tests/test_reproject_cpu.py holds the condition that makes equality a fair demand (float32 and
float64 agree on the winners of these inputs).  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import reproject_reference as RR
from conftest import case_weights, load_case, record

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
PAD = 64                       # canary elements on either side of every output
CANARY_F32 = np.float32(-1234.5)


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def _model(tmp_path_factory, name):
    z, meta, sc = load_case(name)
    d = str(tmp_path_factory.mktemp("reproject_" + name))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, sc, d


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _model(tmp_path_factory, "classroom_n8_thr02")


@pytest.fixture(scope="module")
def ctx(model):
    """one small context for the adaptive sampler; the tests move its frame size (the scratch grows from 16 x 12)"""
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 12)) as r:
        yield r


@pytest.fixture(scope="module")
def ctx_cf(tmp_path_factory):
    z, sc, d = _model(tmp_path_factory, "classroom_coarse_fine_16_24")
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 12)) as r:
        assert r.info.sampler_mode == R.SAMPLER_COARSE_FINE
        yield r, sc


def _f(v, n):
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(n)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


class Buffers:
    """the device side of one call: sources, canaried outputs"""

    def __init__(self, r, n, rgba, depth, acc):
        self.r, self.n = r, n
        self.src = [R.DeviceArray(r, (n, 4), np.uint8).upload(rgba.reshape(n, 4)), R.DeviceArray(r, (n,), np.float32).upload(depth),
                    R.DeviceArray(r, (n,), np.float32).upload(acc)]
        self.host = [rgba.reshape(n, 4), depth, acc]
        t = PAD + n + PAD
        self.colour = R.DeviceArray(r, (t, 4), np.uint8).upload(np.full((t, 4), 0xA5, np.uint8))
        self.depth = R.DeviceArray(r, (t,), np.float32).upload(np.full(t, CANARY_F32, np.float32))
        self.mask = R.DeviceArray(r, (t,), np.uint8).upload(np.full(t, 0xA5, np.uint8))

    def call(self, src_pose, dst_pose, acc_min=RR.ACC_MIN, hole=RR.HOLE, flags=RR.FILL, depth=True, mask=True, holes=True, colour=True, src=(0, 1, 2),
             handle=True):
        """the C ABI itself; returns (rc, holes or None).  Keeps the float arrays alive over the call."""
        keep = [_f(src_pose[0], 3), _f(src_pose[1], 9), _f(dst_pose[0], 3), _f(dst_pose[1], 9)]
        n_holes = C.c_int32(-7)
        s = [self.src[k].ptr if k is not None else None for k in src]
        rc = self.r.lib.adanerf_reproject(self.r.handle if handle else None, s[0], s[1], s[2], keep[0][1], keep[1][1], keep[2][1], keep[3][1],
                                          float(acc_min), int(hole), int(flags), self.colour.ptr + 4 * PAD if colour else None,
                                          self.depth.ptr + 4 * PAD if depth else None, self.mask.ptr + PAD if mask else None,
                                          C.byref(n_holes) if holes else None)
        return rc, (n_holes.value if holes else None)

    def outputs(self):
        """(colour, depth, mask) after a sync, canaries and sources checked"""
        self.r.sync()
        n = self.n
        got = [self.colour.numpy(), self.depth.numpy(), self.mask.numpy()]
        for g, canary, what in zip(got, (0xA5, CANARY_F32, 0xA5), ("colour", "depth", "mask")):
            assert np.all(g[:PAD] == canary) and np.all(g[PAD + n:] == canary), "wrote outside the %s output" % what
        for d, h, what in zip(self.src, self.host, ("colour", "depth_map", "acc_map")):
            assert np.array_equal(d.numpy().view(np.uint8), np.ascontiguousarray(h).view(np.uint8)), "source %s modified" % what
        return [g[PAD:PAD + n] for g in got]

    def untouched(self):
        self.r.sync()
        return all(np.all(b.numpy() == c) for b, c in ((self.colour, 0xA5), (self.depth, CANARY_F32), (self.mask, 0xA5)))

    def free(self):
        for b in self.src + [self.colour, self.depth, self.mask]:
            b.free()


def check(r, sc, w, h, motion, flags, camera_origin=False, seed=1, depth=True, mask=True, holes=True):
    r.set_frame_size(w, h)
    n = w * h
    rgba, dm, acc, _ = RR.depth_scene(w, h, seed)
    src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS[motion])
    want = RR.reproject_f32(sc, w, h, camera_origin, rgba, dm, acc, src[0], src[1], dst[0], dst[1], RR.ACC_MIN, RR.HOLE, flags)
    b = Buffers(r, n, rgba, dm, acc)
    try:
        rc, got_holes = b.call(src, dst, flags=flags, depth=depth, mask=mask, holes=holes)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        colour, got_depth, got_mask = b.outputs()
        tag = "%dx%d %s flags %d" % (w, h, motion, flags)
        print("%s: holes %s (reference %d), filled %d, colour bytes differing %d, depth words differing %d, mask differing %d" % (
            tag, got_holes, want[3], int(np.count_nonzero(want[2] == 2)), int(np.count_nonzero(colour != want[0])),
            int(np.count_nonzero(got_depth.view(np.uint32) != want[1].view(np.uint32))) if depth else -1,
            int(np.count_nonzero(got_mask != want[2])) if mask else -1))
        assert np.array_equal(colour, want[0]), tag
        if depth:
            assert np.array_equal(got_depth.view(np.uint32), want[1].view(np.uint32)), tag
        else:
            assert np.all(got_depth == CANARY_F32)
        if mask:
            assert np.array_equal(got_mask, want[2]), tag
        else:
            assert np.all(got_mask == 0xA5)
        if holes:
            assert got_holes == want[3], tag
        return colour, got_depth, got_mask, got_holes
    finally:
        b.free()


@pytest.mark.parametrize("w,h", RR.SIZES, ids=["%dx%d" % s for s in RR.SIZES])
def test_every_motion_equals_the_definition(ctx, model, w, h):
    """colour, depth, mask and the hole count, with the fill and without"""
    for motion in RR.MOTIONS:
        for flags in (RR.FILL, 0):
            out = check(ctx, model[1], w, h, motion, flags)
            if motion == "identity":
                assert out[3] == 0 and np.all(out[2] == 1)
            if motion == "sees_none":
                assert out[3] == w * h and np.all(out[2] == 0) and np.all(out[1] == 0)
                assert np.all(out[0] == np.frombuffer(np.uint32(RR.HOLE).tobytes(), np.uint8))


def test_optional_outputs_may_be_null(ctx, model):
    w, h = RR.SIZES[0]
    check(ctx, model[1], w, h, "lateral", RR.FILL, depth=False)
    check(ctx, model[1], w, h, "lateral", RR.FILL, mask=False)
    check(ctx, model[1], w, h, "forward", RR.FILL, holes=False)
    check(ctx, model[1], w, h, "backward", 0, depth=False, mask=False, holes=False)


def test_coarse_fine_depths_count_from_the_camera(ctx_cf):
    r, sc = ctx_cf
    w, h = RR.SIZES[0]
    out = check(r, sc, w, h, "lateral", RR.FILL, camera_origin=True)
    # and the origin matters on this input: from the sphere exit the same frame warps differently
    rgba, dm, acc, _ = RR.depth_scene(w, h, 1)
    src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS["lateral"])
    other = RR.reproject_f32(sc, w, h, False, rgba, dm, acc, src[0], src[1], dst[0], dst[1])
    assert not np.array_equal(other[0], out[0])


def test_same_bits_on_every_call_and_across_frame_sizes(ctx, model):
    """the scratch is grown once, reused by a smaller frame, and holds nothing from one call to the next"""
    big, small = RR.SIZES[0], RR.SIZES[1]
    first = check(ctx, model[1], big[0], big[1], "backward", RR.FILL)
    again = check(ctx, model[1], big[0], big[1], "backward", RR.FILL)
    check(ctx, model[1], small[0], small[1], "lateral", RR.FILL)
    third = check(ctx, model[1], big[0], big[1], "backward", RR.FILL)
    for other in (again, third):
        assert np.array_equal(first[0], other[0]) and np.array_equal(first[1].view(np.uint32), other[1].view(np.uint32))
        assert np.array_equal(first[2], other[2]) and first[3] == other[3]


def _psnr8(a, b):
    mse = float(np.mean((a[:, :3].astype(np.float64) / 255.0 - b[:, :3].astype(np.float64) / 255.0) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def test_rendered_frame_warps_towards_the_new_render(model):
    """classroom_n8_thr02 at 48 x 32: warped to its own pose the frame comes back byte for byte; warped to a pose a tenth of the view
    cell away it is closer to that pose's render than the stale frame is.  Also NeuralRenderer.reproject against reproject_device."""
    z, sc, d = model
    w, h = 48, 32
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        with pytest.raises(R.AdaNeRFError):
            r.reproject(z["pose"], z["rot"])                    # nothing to warp yet
        r.enable_reprojection()
        r.set_camera(z["pose"], z["rot"])
        _, stale, _ = r.render_numpy()
        assert len(np.unique(stale[:, :3])) > 16
        same, mask, holes = r.reproject(z["pose"], z["rot"])
        assert holes == 0 and np.all(mask == 1) and np.array_equal(same, stale)
        pose2 = (np.asarray(z["pose"], np.float32) + np.float32(0.1) * np.asarray(sc.view_cell_size, np.float32)).astype(np.float32)
        warped, mask, holes = r.reproject(pose2, z["rot"])
        assert holes == int(np.count_nonzero(mask == 0)) and set(np.unique(mask).tolist()) <= {0, 1, 2}
        # the device entry point on the same frame, fill on and off
        dst, dmask = R.DeviceArray(r, (w * h, 4), np.uint8), R.DeviceArray(r, (w * h,), np.uint8)
        try:
            n = r.reproject_device(r._o_rgba, r._rp_depth, r._rp_acc, z["pose"], z["rot"], pose2, z["rot"], dst, None, dmask)
            assert n == holes and np.array_equal(dst.numpy(), warped) and np.array_equal(dmask.numpy(), mask)
            bare = r.reproject_device(r._o_rgba, r._rp_depth, r._rp_acc, z["pose"], z["rot"], pose2, z["rot"], dst, None, dmask, fill=False)
            assert bare >= holes and bare == int(np.count_nonzero(dmask.numpy() == 0))
            filled = r.reproject(pose2, z["rot"], fill=False)
            assert filled[2] == bare and np.array_equal(filled[0], dst.numpy())
            # against the definition, from the frame's own depth and acc
            want = RR.reproject_f32(sc, w, h, False, stale, r._rp_depth.numpy(), r._rp_acc.numpy(), z["pose"], z["rot"], pose2, z["rot"], 0.5, 0xFF000000, RR.FILL)
            assert np.array_equal(warped, want[0]) and np.array_equal(mask, want[2]) and holes == want[3]
        finally:
            dst.free()
            dmask.free()
        r.set_camera(pose2, z["rot"])
        _, fresh, _ = r.render_numpy()
        p_warp, p_stale = _psnr8(warped, fresh), _psnr8(stale, fresh)
        print("PSNR against the new pose's render: warped %.3f dB, stale %.3f dB, holes %d of %d" % (p_warp, p_stale, holes, w * h))
        record("reproject_rendered_frame", psnr_warped=p_warp, psnr_stale=p_stale, holes=holes, pixels=w * h)
        assert p_warp > p_stale
        # a frame size change drops the frame: nothing to warp until the next render
        r.set_frame_size(24, 16)
        with pytest.raises(R.AdaNeRFError):
            r.reproject(pose2, z["rot"])
        r.render_numpy()
        assert r.reproject(pose2, z["rot"])[0].shape == (24 * 16, 4)


def test_refused_arguments(ctx, model, tmp_path_factory):
    r, sc = ctx, model[1]
    w, h = RR.SIZES[1]
    r.set_frame_size(w, h)
    n = w * h
    rgba, dm, acc, _ = RR.depth_scene(w, h, 1)
    src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS["lateral"])
    b = Buffers(r, n, rgba, dm, acc)
    nan_pos, inf_rot = src[0].copy(), src[1].copy()
    nan_pos[1], inf_rot[2, 0] = np.nan, np.inf
    try:
        cases = [dict(src=(None, 1, 2)), dict(src=(0, None, 2)), dict(src=(0, 1, None)), dict(colour=False),
                 dict(src_pose=(nan_pos, src[1])), dict(src_pose=(src[0], inf_rot)), dict(dst_pose=(nan_pos, dst[1])), dict(dst_pose=(dst[0], inf_rot)),
                 dict(acc_min=float("nan")), dict(acc_min=-0.25), dict(flags=2), dict(flags=3), dict(flags=-1)]
        for kw in cases:
            args = dict(src_pose=src, dst_pose=dst)
            args.update(kw)
            rc, holes = b.call(args.pop("src_pose"), args.pop("dst_pose"), **args)
            assert rc == EINVAL and holes == -7, kw
            assert "adanerf_reproject" in r.lib.adanerf_last_error(r.handle).decode(), kw
            assert b.untouched(), kw
        # NULL poses, and a destination colour overlapping the source colour (the same start; one shared pixel at either end)
        f3, f9 = _f(src[0], 3), _f(src[1], 9)
        for poses in ((None, f9[1], f3[1], f9[1]), (f3[1], None, f3[1], f9[1]), (f3[1], f9[1], None, f9[1]), (f3[1], f9[1], f3[1], None)):
            assert r.lib.adanerf_reproject(r.handle, b.src[0].ptr, b.src[1].ptr, b.src[2].ptr, poses[0], poses[1], poses[2], poses[3], 0.5, 0, 1,
                                           b.colour.ptr + 4 * PAD, None, None, None) == EINVAL
            assert "adanerf_reproject" in r.lib.adanerf_last_error(r.handle).decode() and b.untouched()
        big = R.DeviceArray(r, (3 * n, 4), np.uint8).upload(np.full((3 * n, 4), 0x5A, np.uint8))
        try:
            for s_off, d_off in ((n, n), (n, 1), (n, 2 * n - 1)):
                rc = r.lib.adanerf_reproject(r.handle, big.ptr + 4 * s_off, b.src[1].ptr, b.src[2].ptr, f3[1], f9[1], f3[1], f9[1], 0.5, 0, 1,
                                             big.ptr + 4 * d_off, None, None, None)
                assert rc == EINVAL and "overlap" in r.lib.adanerf_last_error(r.handle).decode(), (s_off, d_off)
            r.sync()
            assert np.all(big.numpy() == 0x5A)
            assert r.lib.adanerf_reproject(r.handle, big.ptr + 4 * n, b.src[1].ptr, b.src[2].ptr, f3[1], f9[1], f3[1], f9[1], 0.5, 0, 1,
                                           big.ptr, None, None, None) == 0      # adjacent ranges do not overlap
            assert r.lib.adanerf_reproject(r.handle, big.ptr + 4 * n, b.src[1].ptr, b.src[2].ptr, f3[1], f9[1], f3[1], f9[1], 0.0, 0, 0,
                                           big.ptr + 8 * n, None, None, None) == 0      # acc_min 0 is legal
            r.sync()
        finally:
            big.free()
        assert b.call(src, dst, handle=False)[0] == EINVAL and b.untouched()
        rc, holes = b.call(src, dst)
        assert rc == 0 and holes >= 0
    finally:
        b.free()
    # a useNDC model; a context that renders one of two shards
    z, sc_ndc, d_ndc = _model(tmp_path_factory, "ndc_synthetic_n8")
    for d, kw, word in ((d_ndc, dict(), "NDC"), (model[2], dict(shard_world=2, shard_rank=0), "shard_world")):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, 16), **kw) as r2:
            b = Buffers(r2, w * 16, *RR.depth_scene(w, 16, 1)[:3])
            try:
                rc, holes = b.call(src, dst)
                assert rc == EUNSUPPORTED and holes == -7 and word in r2.lib.adanerf_last_error(r2.handle).decode()
                assert b.untouched()
            finally:
                b.free()


def _bmp(path):
    bmp = open(path, "rb").read()
    return bmp[int.from_bytes(bmp[10:14], "little"):]


def test_cli_reproject(model, tmp_path):
    """--reproject 1 is the CLI as it was, byte for byte; --reproject 3 over a script that holds the camera still shows an identity warp
    of the rendered frame: the same image"""
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    script = tmp_path / "still.txt"
    script.write_text("# still\n" * 3)
    base = [exe, d, "-s", "64", "48", "-ws", "80", "60", "-w", "--write-window", "--script", str(script), "--log-camera"]
    images, outputs = [], []
    try:
        for extra in ([], ["--reproject", "1"], ["--reproject", "3"]):
            for name in ("out.bmp", "out_window.bmp"):
                if os.path.exists(os.path.join(d, name)):
                    os.remove(os.path.join(d, name))
            out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            outputs.append([l for l in out.stdout.splitlines() if not l.startswith("NeuralRenderer iter")])
            images.append((open(os.path.join(d, "out.bmp"), "rb").read(), open(os.path.join(d, "out_window.bmp"), "rb").read()))
        assert images[0] == images[1] and outputs[0] == outputs[1]
        assert images[2] == images[0] and len(np.unique(np.frombuffer(_bmp(os.path.join(d, "out.bmp")), np.uint8))) > 16
        # many shares, or the debug view of the sampling network: nothing to warp
        out = subprocess.run([exe, d, "-s", "64", "48", "--gpus", "2", "--same-device", "--reproject", "2", "--frames", "2"], capture_output=True,
                             text=True, timeout=120)
        assert out.returncode != 0 and "--reproject warps whole frames" in out.stdout
    finally:
        for name in ("out.bmp", "out_window.bmp"):
            if os.path.exists(os.path.join(d, name)):
                os.remove(os.path.join(d, name))


def test_evaluator_reproject_stride(tmp_path):
    """evaluate(..., reproject_stride=2) on a synthetic 12 x 10 dataset of three poses: poses 0 and 2 are the plain run's frames, pose 1 is
    pose 0's frame warped by NeuralRenderer.reproject and scored from the 8-bit image; the summary keeps the two kinds apart."""
    import json
    from adanerf_amd.evaluate import evaluate, psnr_from_mse
    from adanerf_amd.png import read_png, write_png
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    w, h = 12, 10
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[w, h], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    centre = np.array(sc.view_cell_center, np.float32)
    poses = [(centre, O.camera_rotation(100.0, 0.0)), (centre + np.float32([0.05, 0.02, 0.0]), O.camera_rotation(103.0, 0.0)),
             (centre + np.float32([0.1, 0.05, -0.02]), O.camera_rotation(60.0, -8.0))]
    frames, gts = [], []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        gts.append(np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
        write_png(str(ds / "test" / ("%05d.png" % i)), gts[-1])
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    summary, recs = evaluate(md, str(ds), "test", str(tmp_path / "pred"), precision="bf16", quiet=True, metrics=("psnr", "flip"), reproject_stride=2)
    plain, precs = evaluate(md, str(ds), "test", str(tmp_path / "plain"), precision="bf16", quiet=True, metrics=("psnr", "flip"))
    assert sorted(plain) == ["frames", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    assert sorted(summary) == sorted(list(plain) + ["mean_psnr_rendered", "mean_psnr_warped", "mean_flip_rendered", "mean_flip_warped", "mean_hole_fraction"])
    assert [x["warped"] for x in recs] == [False, True, False]
    for i in (0, 2):
        assert np.array_equal(read_png(str(tmp_path / "pred" / ("%05d.png" % i))), read_png(str(tmp_path / "plain" / ("%05d.png" % i))))
        assert recs[i]["psnr"] == precs[i]["psnr"] and recs[i]["flip"] == precs[i]["flip"] and recs[i]["samples_per_ray"] == precs[i]["samples_per_ray"]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w, h)) as r:
        r.enable_reprojection()
        r.set_camera(*poses[0])
        r.render_numpy()
        want, mask, holes = r.reproject(*poses[1])
    assert np.array_equal(read_png(str(tmp_path / "pred" / "00001.png")), want[:, :3].reshape(h, w, 3))
    ref = gts[1].astype(np.float32).reshape(-1, 3) / 255.0
    mse = float(np.mean((want[:, :3].astype(np.float32) / 255.0 - ref.astype(np.float64)) ** 2))
    assert recs[1]["mse"] == mse and recs[1]["psnr"] == psnr_from_mse(mse) and recs[1]["hole_fraction"] == holes / float(w * h)
    assert "samples_per_ray" not in recs[1] and 0.0 <= recs[1]["flip"] <= 1.0
    assert summary["mean_psnr_warped"] == recs[1]["psnr"] and summary["mean_hole_fraction"] == recs[1]["hole_fraction"]
    assert summary["mean_psnr_rendered"] == float(np.mean([recs[0]["psnr"], recs[2]["psnr"]]))
    assert summary["mean_samples_per_ray"] == float(np.mean([precs[0]["samples_per_ray"], precs[2]["samples_per_ray"]]))
