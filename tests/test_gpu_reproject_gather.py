"""adanerf_reproject_gather on the GPU: every geometric case is exact equality with tests/reproject_gather_reference.py (gather_f32, the
definition in include/adanerf_hip.h in numpy float32) for all five outputs -- fp32 colour bits, the 8-bit image, depth bits, mask and
the hole count.  Colours are random fp32 with NaNs, +0 / -0 pairs and values outside [0, 1] planted, over the synthetic wall + box depth
scene of tests/reproject_reference.py with far pixels of every kind; canaries sit before and after every output and the sources are
checked unmodified.  tests/test_reproject_gather_cpu.py holds the condition that makes equality a fair demand (float32 and float64
agree on the mask and the final tap of these inputs).  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import reproject_gather_reference as G
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
    d = str(tmp_path_factory.mktemp("gather_" + name))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, sc, d


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _model(tmp_path_factory, "classroom_n8_thr02")


@pytest.fixture(scope="module")
def ctx(model):
    """one small context for the adaptive sampler; the tests move its frame size"""
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
    if v is None:
        return None, None
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(n)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


_INPUTS, _WANT = {}, {}


def inputs(w, h, seed=1):
    """(rgb, depth_map, acc_map): computed once per size, shared and never changed"""
    if (w, h, seed) not in _INPUTS:
        _, dm, acc, _ = RR.depth_scene(w, h, seed)
        arrays = (G.colours(w, h, seed), dm, acc)
        for a in arrays:
            a.setflags(write=False)
        _INPUTS[(w, h, seed)] = arrays
    return _INPUTS[(w, h, seed)]


def reference(sc, w, h, camera_origin, motion, iterations, flags, tol=G.DEPTH_TOL):
    key = (w, h, camera_origin, motion, iterations, flags, tol)
    if key not in _WANT:
        rgb, dm, acc = inputs(w, h)
        src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS[motion])
        _WANT[key] = G.gather_f32(sc, w, h, camera_origin, rgb, dm, acc, src[0], src[1], dst[0], dst[1], depth_tol=tol, iterations=iterations, flags=flags)
    return _WANT[key]


class Buffers:
    """the device side of one frame size: the three sources, four canaried outputs"""
    CANARIES = (CANARY_F32, 0xA5, CANARY_F32, 0xA5)
    NAMES = ("rgb", "rgba8", "depth", "mask")

    def __init__(self, r, n, arrays):
        self.r, self.n = r, n
        self.host = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        self.src = [R.DeviceArray(r, a.shape, a.dtype).upload(a) for a in self.host]
        t = PAD + n + PAD
        self.out = [R.DeviceArray(r, (t, 3), np.float32), R.DeviceArray(r, (t, 4), np.uint8), R.DeviceArray(r, (t,), np.float32), R.DeviceArray(r, (t,), np.uint8)]
        self.step = [12, 4, 4, 1]      # bytes per element
        self.reset()

    def reset(self):
        for b, c in zip(self.out, self.CANARIES):
            b.upload(np.full(b.shape, c, b.dtype))

    def call(self, src_pose, dst_pose, acc_min=RR.ACC_MIN, tol=G.DEPTH_TOL, iterations=G.ITERATIONS, hole=RR.HOLE, flags=0, src=(0, 1, 2), outs=(0, 1, 2, 3),
             holes=True, handle=True, src_ptr=None, out_ptr=None):
        """the C ABI itself; returns (rc, holes or None).  src_ptr / out_ptr: {index: address} in place of a buffer's own."""
        keep = [_f(src_pose[0], 3), _f(src_pose[1], 9), _f(dst_pose[0], 3), _f(dst_pose[1], 9)]
        n_holes = C.c_int32(-7)
        s = [self.src[k].ptr if k is not None else None for k in src]
        o = [self.out[k].ptr + self.step[k] * PAD if k in outs else None for k in range(4)]
        for k, p in (src_ptr or {}).items():
            s[k] = p
        for k, p in (out_ptr or {}).items():
            o[k] = p
        rc = self.r.lib.adanerf_reproject_gather(self.r.handle if handle else None, s[0], s[1], s[2], keep[0][1], keep[1][1], keep[2][1], keep[3][1],
                                                 float(acc_min), float(tol), int(iterations), int(hole), int(flags), o[0], o[1], o[2], o[3],
                                                 C.byref(n_holes) if holes else None)
        return rc, (n_holes.value if holes else None)

    def outputs(self):
        """(rgb, rgba8, depth, mask) after a sync, canaries and sources checked"""
        self.r.sync()
        n = self.n
        got = [b.numpy() for b in self.out]
        for g, canary, what in zip(got, self.CANARIES, self.NAMES):
            assert np.all(g[:PAD] == canary) and np.all(g[PAD + n:] == canary), "wrote outside the %s output" % what
        for d, hst, what in zip(self.src, self.host, ("src_rgb", "src_depth_map", "src_acc_map")):
            assert np.array_equal(d.numpy().view(np.uint8).reshape(-1), hst.view(np.uint8).reshape(-1)), "source %s modified" % what
        return [g[PAD:PAD + n] for g in got]

    def untouched(self):
        self.r.sync()
        return all(np.all(b.numpy() == c) for b, c in zip(self.out, self.CANARIES))

    def free(self):
        for b in self.src + self.out:
            b.free()


def check(b, sc, w, h, motion, iterations=G.ITERATIONS, flags=0, camera_origin=False, outs=(0, 1, 2, 3), holes=True):
    """one call against the definition; b: the Buffers of this size on a context whose frame size is (w, h)"""
    want = reference(sc, w, h, camera_origin, motion, iterations, flags)
    src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS[motion])
    b.reset()
    rc, got_holes = b.call(src, dst, iterations=iterations, flags=flags, outs=outs, holes=holes)
    assert rc == 0, b.r.lib.adanerf_last_error(b.r.handle).decode()
    rgb, rgba8, depth, mask = b.outputs()
    tag = "%dx%d %s iterations %d flags %d" % (w, h, motion, iterations, flags)
    n = w * h
    print("%s: holes %s (reference %d), mask 1 / 2: %d / %d, colour words differing %d, bytes %d, depth words %d, mask %d" % (
        tag, got_holes, want.holes, int(np.count_nonzero(want.mask == 1)), int(np.count_nonzero(want.mask == 2)),
        int(np.count_nonzero(rgb.view(np.uint32) != want.rgb.view(np.uint32))), int(np.count_nonzero(rgba8 != want.rgba8)) if 1 in outs else -1,
        int(np.count_nonzero(depth.view(np.uint32) != want.depth.view(np.uint32))) if 2 in outs else -1, int(np.count_nonzero(mask != want.mask)) if 3 in outs else -1))
    assert np.array_equal(rgb.view(np.uint32), np.ascontiguousarray(want.rgb).view(np.uint32)), tag
    for k, got, exp in ((1, rgba8, want.rgba8), (2, depth.view(np.uint32), want.depth.view(np.uint32)), (3, mask, want.mask)):
        if k in outs:
            assert np.array_equal(got, exp), (tag, Buffers.NAMES[k])
        else:
            assert np.all(b.out[k].numpy() == Buffers.CANARIES[k]), (tag, Buffers.NAMES[k])
    if holes:
        assert got_holes == want.holes, tag
    assert n == rgb.shape[0]
    return rgb, rgba8, depth, mask, got_holes


@pytest.mark.parametrize("w,h", G.GPU_SIZES, ids=["%dx%d" % s for s in G.GPU_SIZES])
def test_every_motion_equals_the_definition(ctx, model, w, h):
    """fp32 colour, 8-bit image, depth, mask and the hole count, at 1, 3 and 8 iterations, with ADANERF_GATHER_GUESS and without"""
    ctx.set_frame_size(w, h)
    b = Buffers(ctx, w * h, inputs(w, h))
    try:
        for motion in RR.MOTIONS:
            for iterations in (1, 3, 8):
                for flags in (0, G.GUESS):
                    out = check(b, model[1], w, h, motion, iterations, flags)
                    if motion == "identity":
                        assert out[4] == 0 and np.all(out[3] == 1)
                    if motion == "sees_none":
                        assert out[4] == w * h and np.all(out[3] == 0) and np.all(out[2] == 0) and np.all(out[0].view(np.uint32) == 0)
                        assert np.all(out[1] == np.frombuffer(np.uint32(RR.HOLE).tobytes(), np.uint8))
    finally:
        b.free()


def test_coarse_fine_depths_count_from_the_camera(ctx_cf):
    r, sc = ctx_cf
    w, h = RR.SIZES[0]
    r.set_frame_size(w, h)
    b = Buffers(r, w * h, inputs(w, h))
    try:
        out = check(b, sc, w, h, "lateral", 3, G.GUESS, camera_origin=True)
    finally:
        b.free()
    # and the origin matters on this input: from the sphere exit the same frame gathers differently
    other = reference(sc, w, h, False, "lateral", 3, G.GUESS)
    assert not np.array_equal(other.rgb.view(np.uint32), out[0].view(np.uint32))


def test_every_optional_output_may_be_null(ctx, model):
    w, h = 33, 9
    ctx.set_frame_size(w, h)
    b = Buffers(ctx, w * h, inputs(w, h))
    try:
        for given in itertools.product((False, True), repeat=4):      # rgba8, depth, mask, holes_out
            outs = (0,) + tuple(k + 1 for k in range(3) if given[k])
            check(b, model[1], w, h, "lateral", 3, G.GUESS, outs=outs, holes=given[3])
    finally:
        b.free()


def test_same_bits_on_every_call_and_across_frame_sizes(model):
    """a fresh context: the surface table is made at 16 x 12, grown for 97 x 61, reused by 16 x 12, and holds nothing from call to call"""
    z, sc, d = model
    big, small = RR.SIZES[0], RR.SIZES[1]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, small[0], small[1])) as r:
        seen = {}
        for (w, h) in (small, big, small, big):
            r.set_frame_size(w, h)
            b = Buffers(r, w * h, inputs(w, h))
            try:
                first = check(b, sc, w, h, "backward", 3, G.GUESS)
                again = check(b, sc, w, h, "backward", 3, G.GUESS)
            finally:
                b.free()
            for other in (again, seen.setdefault((w, h), first)):
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first[:4], other[:4])) and first[4] == other[4]


def test_refused_arguments(ctx, model, tmp_path_factory):
    r, sc = ctx, model[1]
    w, h = RR.SIZES[1]
    r.set_frame_size(w, h)
    n = w * h
    src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS["lateral"])
    b = Buffers(r, n, inputs(w, h))
    nan_pos, inf_rot = src[0].copy(), src[1].copy()
    nan_pos[1], inf_rot[2, 0] = np.nan, np.inf
    o = [b.out[k].ptr + b.step[k] * PAD for k in range(4)]
    s = [a.ptr for a in b.src]
    try:
        cases = [dict(src=(None, 1, 2)), dict(src=(0, None, 2)), dict(src=(0, 1, None)), dict(outs=(1, 2, 3)),
                 dict(src_pose=(None, src[1])), dict(src_pose=(src[0], None)), dict(dst_pose=(None, dst[1])), dict(dst_pose=(dst[0], None)),
                 dict(src_pose=(nan_pos, src[1])), dict(src_pose=(src[0], inf_rot)), dict(dst_pose=(nan_pos, dst[1])), dict(dst_pose=(dst[0], inf_rot)),
                 dict(acc_min=float("nan")), dict(acc_min=-0.25), dict(tol=float("nan")), dict(tol=-0.01),
                 dict(iterations=0), dict(iterations=9), dict(iterations=-1), dict(flags=2), dict(flags=3), dict(flags=-1),
                 # misaligned fp32 and uchar4 pointers
                 dict(src_ptr={0: s[0] + 2}), dict(src_ptr={1: s[1] + 1}), dict(src_ptr={2: s[2] + 3}), dict(out_ptr={0: o[0] + 2}), dict(out_ptr={1: o[1] + 1}),
                 dict(out_ptr={2: o[2] + 2}),
                 # an output over an input: the same start, one shared element at either end
                 dict(out_ptr={0: s[0]}), dict(out_ptr={0: s[0] + 12 * (n - 1)}), dict(out_ptr={2: s[1]}), dict(out_ptr={2: s[2] + 4 * (n - 1)}),
                 dict(out_ptr={1: s[2] - 4 * (n - 1)}), dict(out_ptr={3: s[1] + 4 * n - 1}), dict(out_ptr={3: s[0]}), dict(out_ptr={1: s[0] + 8 * n}),
                 # an output over another output
                 dict(out_ptr={1: o[0]}), dict(out_ptr={2: o[0] + 12 * n - 4}), dict(out_ptr={3: o[0] + 5}), dict(out_ptr={2: o[1]}), dict(out_ptr={3: o[1] + 4 * n - 1}),
                 dict(out_ptr={3: o[2]}), dict(out_ptr={1: o[3] - 4 * n + 4})]
        for kw in cases:
            args = dict(src_pose=src, dst_pose=dst)
            args.update(kw)
            rc, holes = b.call(args.pop("src_pose"), args.pop("dst_pose"), **args)
            assert rc == EINVAL and holes == -7, kw
            assert "adanerf_reproject_gather" in r.lib.adanerf_last_error(r.handle).decode(), kw
            assert b.untouched(), kw
            r.sync()
            assert all(np.array_equal(d.numpy().view(np.uint8).reshape(-1), hst.view(np.uint8).reshape(-1)) for d, hst in zip(b.src, b.host)), kw
        assert b.call(src, dst, handle=False)[0] == EINVAL and b.untouched()
        # adjacent ranges do not overlap; acc_min 0, depth_tol 0 and both ends of the iterations' range are legal
        big = R.DeviceArray(r, (5 * n,), np.float32)
        try:
            rc, holes = b.call(src, dst, acc_min=0.0, tol=0.0, iterations=1, out_ptr={0: big.ptr, 1: big.ptr + 12 * n, 2: big.ptr + 16 * n})
            assert rc == 0 and holes >= 0, r.lib.adanerf_last_error(r.handle).decode()
            rc, holes = b.call(src, dst, iterations=8, flags=G.GUESS)
            assert rc == 0 and holes >= 0
            r.sync()
        finally:
            big.free()
    finally:
        b.free()
    # a useNDC model; a context that renders one of two shards
    z, sc_ndc, d_ndc = _model(tmp_path_factory, "ndc_synthetic_n8")
    for d, kw, word in ((d_ndc, dict(), "NDC"), (model[2], dict(shard_world=2, shard_rank=0), "shard_world")):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, 16), **kw) as r2:
            b = Buffers(r2, w * 16, inputs(w, 16))
            try:
                rc, holes = b.call(src, dst)
                assert rc == EUNSUPPORTED and holes == -7 and word in r2.lib.adanerf_last_error(r2.handle).decode()
                assert b.untouched()
            finally:
                b.free()


def _psnr8(a, b):
    mse = float(np.mean((a[:, :3].astype(np.float64) / 255.0 - b[:, :3].astype(np.float64) / 255.0) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def test_rendered_frame_gathers_towards_the_new_render_and_holes_rerender(model):
    """classroom_n8_thr02 at 48 x 32, the pose of test_rendered_frame_warps_towards_the_new_render (a tenth of the view cell away): the
    gathered frame is nearer to that pose's render than the stale frame is -- the one assertion about quality; the gather's and the
    splat's PSNR and hole counts are recorded.  Then NeuralRenderer.reproject_gather against the definition and the device entry point,
    and reproject_gather_rerender("holes"): every mask-1 pixel keeps its bytes, every mask-0 pixel gets adanerf_render's at that pose."""
    z, sc, d = model
    w, h = 48, 32
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        with pytest.raises(R.AdaNeRFError):
            r.reproject_gather(z["pose"], z["rot"])                    # nothing to warp yet
        r.enable_reprojection()
        r.set_camera(z["pose"], z["rot"])
        stale_rgb, stale, _ = r.render_numpy()
        assert len(np.unique(stale[:, :3])) > 16
        rgb, same, mask, holes = r.reproject_gather(z["pose"], z["rot"])
        assert holes == 0 and np.all(mask == 1) and np.max(np.abs(same[:, :3].astype(int) - stale[:, :3].astype(int))) <= 1
        pose2 = (np.asarray(z["pose"], np.float32) + np.float32(0.1) * np.asarray(sc.view_cell_size, np.float32)).astype(np.float32)
        rgb, warped, mask, holes = r.reproject_gather(pose2, z["rot"])
        assert holes == int(np.count_nonzero(mask == 0)) and set(np.unique(mask).tolist()) <= {0, 1, 2}
        want = G.gather_f32(sc, w, h, False, stale_rgb, r._rp_depth.numpy(), r._rp_acc.numpy(), z["pose"], z["rot"], pose2, z["rot"], acc_min=0.5,
                            depth_tol=R.GATHER_DEPTH_TOL, iterations=R.GATHER_ITERATIONS, hole_rgba8=0xFF000000, flags=G.GUESS)
        assert np.array_equal(rgb.view(np.uint32), want.rgb.view(np.uint32)) and np.array_equal(warped, want.rgba8)
        assert np.array_equal(mask, want.mask) and holes == want.holes
        strict = r.reproject_gather(pose2, z["rot"], guess=False)
        assert np.array_equal(strict[2] == 1, mask == 1) and strict[3] == int(np.count_nonzero(mask != 1))
        splat, smask, sholes = r.reproject(pose2, z["rot"])
        _, _, bare = r.reproject(pose2, z["rot"], fill=False)
        # the holes rendered at the destination pose
        r.reproject_gather(pose2, z["rot"])
        rr, rmask, rholes, rerendered = r.reproject_gather_rerender(pose2, z["rot"], "holes")
        assert np.array_equal(rmask, mask) and rholes == holes == rerendered
        r.set_camera(pose2, z["rot"])
        _, fresh, _ = r.render_numpy()
        assert np.array_equal(rr[mask != 0], warped[mask != 0]) and np.array_equal(rr[mask == 0], fresh[mask == 0])
        p_gather, p_splat, p_stale = _psnr8(warped, fresh), _psnr8(splat, fresh), _psnr8(stale, fresh)
        print("PSNR against the new pose's render: gathered %.3f dB (mask 0: %d, mask 2: %d), splat %.3f dB (holes %d, unfilled %d), stale %.3f dB, of %d px" % (
            p_gather, holes, int(np.count_nonzero(mask == 2)), p_splat, sholes, bare, p_stale, w * h))
        record("reproject_gather_rendered_frame", psnr_gather=p_gather, psnr_splat=p_splat, psnr_stale=p_stale, holes_gather=holes,
               unverified_gather=int(np.count_nonzero(mask == 2)), holes_splat=sholes, holes_splat_unfilled=bare, pixels=w * h)
        assert p_gather > p_stale


def test_cli_gather_warp(model, tmp_path):
    """--reproject 3 --reproject-warp gather --rerender holes -w runs and writes frames; over a script that holds the camera still the
    warped frame is the rendered one up to the rounding of the fp32 colour"""
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    script = tmp_path / "still.txt"
    script.write_text("# still\n" * 3)
    base = [exe, d, "-s", "64", "48", "-w", "--script", str(script), "--log-camera"]
    images = []
    try:
        for extra in (["--reproject", "3"], ["--reproject", "3", "--reproject-warp", "gather", "--rerender", "holes"],
                      ["--reproject", "3", "--reproject-warp", "gather", "--reproject-iterations", "2", "--reproject-tol", "0.1"]):
            if os.path.exists(os.path.join(d, "out.bmp")):
                os.remove(os.path.join(d, "out.bmp"))
            out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            bmp = open(os.path.join(d, "out.bmp"), "rb").read()
            images.append(np.frombuffer(bmp[int.from_bytes(bmp[10:14], "little"):], np.uint8).astype(int))
            if "--rerender" in extra:
                assert "warped 1 holes 0 rerendered 0" in out.stdout and "warped 2 holes 0 rerendered 0" in out.stdout
        assert len(np.unique(images[0])) > 16
        for img in images[1:]:
            assert img.shape == images[0].shape and np.max(np.abs(img - images[0])) <= 1
    finally:
        if os.path.exists(os.path.join(d, "out.bmp")):
            os.remove(os.path.join(d, "out.bmp"))


def test_evaluator_gather_warp(tmp_path):
    """evaluate(..., reproject_stride=2, reproject_warp="gather") on the synthetic 12 x 10 dataset of test_evaluator_reproject_stride:
    pose 1 is pose 0's frame gathered by NeuralRenderer.reproject_gather; records carry `warp`, the summary keys are the splat run's"""
    from adanerf_amd.evaluate import evaluate, main
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
    frames = []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        write_png(str(ds / "test" / ("%05d.png" % i)), np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    summary, recs = evaluate(md, str(ds), "test", str(tmp_path / "gather"), precision="bf16", quiet=True, reproject_stride=2, reproject_warp="gather",
                             rerender="holes")
    splat, srecs = evaluate(md, str(ds), "test", str(tmp_path / "splat"), precision="bf16", quiet=True, reproject_stride=2, rerender="holes")
    assert sorted(summary) == sorted(splat)
    assert [x["warped"] for x in recs] == [False, True, False] and [x.get("warp") for x in recs] == [None, "gather", None]
    assert [x.get("warp") for x in srecs] == [None, "splat", None]
    for i in (0, 2):
        assert np.array_equal(read_png(str(tmp_path / "gather" / ("%05d.png" % i))), read_png(str(tmp_path / "splat" / ("%05d.png" % i))))
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w, h)) as r:
        r.enable_reprojection()
        r.set_camera(*poses[0])
        r.render_numpy()
        _, want, mask, holes = r.reproject_gather(*poses[1])
    assert np.array_equal(read_png(str(tmp_path / "gather" / "00001.png")), want[:, :3].reshape(h, w, 3))
    assert recs[1]["hole_fraction"] == holes / float(w * h) and recs[1]["rerendered_fraction"] == holes / float(w * h)
    # and the command line
    main([md, str(ds), "--reproject-stride", "2", "--reproject-warp", "gather", "--reproject-iterations", "2", "--reproject-tol", "0.1"])
