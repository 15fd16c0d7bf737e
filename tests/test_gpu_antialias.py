"""Anti-aliasing on the GPU: sub-pixel ray offsets (adanerf_set_pixel_offset), accumulation (adanerf_accumulate / adanerf_resolve_mean) and
the area filter of adanerf_present (ADANERF_PRESENT_AREA).  Every comparison is exact equality with tests/antialias_reference.py (numpy
integers, numpy float32, the float64 ray table with the offset as include/adanerf_hip.h defines it); canaries sit before and after every
output.  tests/test_antialias_cpu.py holds the properties of those restatements.  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import antialias_reference as AR
import present_reference as P
import reproject_reference as RR
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL = -1
PAD = 64                       # canary elements on either side of every output
CANARY_F32 = np.float32(-1234.5)
W, H = 16, 12


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def _model(tmp_path_factory, name):
    z, meta, sc = load_case(name)
    d = str(tmp_path_factory.mktemp("antialias_" + name))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, sc, d


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return _model(tmp_path_factory, "classroom_n8_thr02")


@pytest.fixture(scope="module")
def ctx(model):
    """one small context of the adaptive sampler; tests that move its frame size or offset put both back"""
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as r:
        r.set_camera(z["pose"], z["rot"])
        yield r


class Canaried:
    """a device array of n rows with PAD canary rows on either side"""

    def __init__(self, r, n, cols, dtype, canary):
        self.r, self.n, self.canary = r, n, canary
        shape = (PAD + n + PAD,) + ((cols,) if cols else ())
        self.a = R.DeviceArray(r, shape, dtype).upload(np.full(shape, canary, dtype))
        self.ptr = self.a.ptr + PAD * (cols or 1) * np.dtype(dtype).itemsize

    def get(self):
        """the n rows after a sync, canaries checked"""
        self.r.sync()
        g = self.a.numpy()
        assert np.all(g[:PAD] == self.canary) and np.all(g[PAD + self.n:] == self.canary), "wrote outside the output"
        return g[PAD:PAD + self.n]

    def untouched(self):
        self.r.sync()
        return bool(np.all(self.a.numpy() == self.canary))

    def free(self):
        self.a.free()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_f32(got, want):
    """every value the same float32: the same bits, or a NaN on both sides.  Which NaN an invalid operation makes is the platform's choice
    (inf - inf is 0xFFC00000 on the x86 host that runs numpy, 0x7FC00000 on the device): IEEE 754 fixes that it is a quiet NaN, not its
    sign.  Everything else, signed zeros, denormals and infinities included, is compared bit for bit."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


# ---- 1. the area filter ----------------------------------------------------------------------------------

def image(w, h, seed):
    rng = np.random.default_rng(seed + 1000 * w + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    flat = img.reshape(-1)
    flat[rng.integers(0, flat.size, max(2, flat.size // 7))] = 0
    flat[rng.integers(0, flat.size, max(2, flat.size // 7))] = 255
    flat[0], flat[-1] = 255, 0
    return img


def present(r, src, dw, dh, flags, offset_px=0):
    """adanerf_present through the C ABI, the destination `offset_px` pixels into a larger buffer with canaries around it"""
    sh, sw = src.shape[:2]
    d_src = R.DeviceArray(r, src.shape, np.uint8).upload(src)
    dst = Canaried(r, offset_px + dw * dh, 4, np.uint8, 0xA5)
    try:
        rc = r.lib.adanerf_present(r.handle, d_src.ptr, sw, sh, dst.ptr + 4 * offset_px, dw, dh, flags)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        got = dst.get()
        assert np.all(got[:offset_px] == 0xA5), "wrote in front of the destination"
        assert np.array_equal(d_src.numpy(), src), "source modified"
        return got[offset_px:].reshape(dh, dw, 4)
    finally:
        d_src.free()
        dst.free()


@pytest.mark.parametrize("sw,sh,dw,dh", AR.AREA_SIZES, ids=["%dx%d-%dx%d" % s for s in AR.AREA_SIZES])
def test_area_present_equals_the_definition(ctx, sw, sh, dw, dh):
    src = image(sw, sh, 11)
    for flip in (False, True):
        for offset_px in (0, 3):
            got = present(ctx, src, dw, dh, AR.AREA | (P.FLIP_Y if flip else 0), offset_px)
            want = AR.area_present(src, dw, dh, flip)
            assert np.array_equal(got, want), "%dx%d -> %dx%d flip %d offset %d: %d of %d bytes differ" % (
                sw, sh, dw, dh, flip, offset_px, int(np.count_nonzero(got != want)), want.size)
    if (sw, sh) == (dw, dh):
        assert np.array_equal(present(ctx, src, dw, dh, AR.AREA), src)
    white = np.full((sh, sw, 4), 255, np.uint8)
    assert np.all(present(ctx, white, dw, dh, AR.AREA) == 255)


def test_area_present_refusals_and_the_other_filters_unchanged(ctx):
    r = ctx
    src = R.DeviceArray(r, (300 * 20, 4), np.uint8).upload(np.zeros((6000, 4), np.uint8))
    dst = Canaried(r, 64 * 64, 4, np.uint8, 0xA5)
    try:
        call = lambda sw, sh, dw, dh, fl: r.lib.adanerf_present(r.handle, src.ptr, sw, sh, dst.ptr, dw, dh, fl)
        for args in ((17, 4, 2, 4, AR.AREA), (4, 17, 4, 2, AR.AREA), (300, 3, 37, 1, AR.AREA), (9, 9, 1, 1, AR.AREA | P.FLIP_Y),
                     (8, 8, 4, 4, AR.AREA | P.LINEAR), (8, 8, 4, 4, AR.AREA | P.NEAREST), (8, 8, 4, 4, AR.AREA | P.NEAREST | P.LINEAR),
                     (8, 8, 4, 4, AR.AREA | P.LINEAR | P.FLIP_Y), (8, 8, 4, 4, 16), (8, 8, 4, 4, AR.AREA | 16)):
            assert call(*args) == EINVAL, args
            assert "adanerf_present" in r.lib.adanerf_last_error(r.handle).decode()
            assert dst.untouched(), args
        assert "two steps" in (call(17, 4, 2, 4, AR.AREA), r.lib.adanerf_last_error(r.handle).decode())[1]
        assert call(16, 8, 2, 1, AR.AREA) == 0 and call(300, 3, 38, 1, AR.AREA) == 0      # a ratio of exactly 8, and just below it
        r.sync()
        with pytest.raises(ValueError):
            r.present_device(src, 8, 8, dst.a, 4, 4, filter="cubic")
    finally:
        src.free()
        dst.free()
    # flags 0 / _NEAREST / _LINEAR: the bytes of the present step as it was
    for sw, sh, dw, dh in ((97, 61, 41, 23), (7, 5, 13, 11), (8, 6, 4, 3)):
        img = image(sw, sh, 5)
        for flags in (0, P.NEAREST, P.LINEAR, P.FLIP_Y, P.LINEAR | P.FLIP_Y):
            assert np.array_equal(present(r, img, dw, dh, flags, 1), P.present(img, dw, dh, flags)), (sw, sh, dw, dh, flags)


# ---- 2. offsets reach the rays ---------------------------------------------------------------------------

def feature_rays(r, first, n):
    """d_rays_out of adanerf_ray_features for local rays first .. first + n"""
    out = Canaried(r, n, 8, np.float32, CANARY_F32)
    try:
        rc = r.lib.adanerf_ray_features(r.handle, first, n, None, out.ptr)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        return out.get()
    finally:
        out.free()


@pytest.mark.parametrize("w,h", AR.RAY_SIZES, ids=["%dx%d" % s for s in AR.RAY_SIZES])
def test_offsets_reach_the_rays(ctx, model, w, h):
    z, sc, d = model
    r = ctx
    try:
        r.set_frame_size(w, h)
        centre = None
        for dx, dy in AR.OFFSETS:
            r.set_pixel_offset(dx, dy)
            assert r.pixel_offset == (dx, dy)
            got = feature_rays(r, 0, w * h)
            want = AR.rays(sc, w, h, z["pose"], z["rot"], dx, dy)
            assert np.array_equal(bits(got), bits(want)), "%dx%d offset (%g, %g): %d of %d words differ" % (
                w, h, dx, dy, int(np.count_nonzero(bits(got) != bits(want))), want.size)
            centre = got if (dx, dy) == (0.0, 0.0) else centre
            assert (dx, dy) == (0.0, 0.0) or not np.array_equal(got, centre)
        if w * h > 40:      # a range that starts inside the frame
            r.set_pixel_offset(0.25, -0.25)
            assert np.array_equal(bits(feature_rays(r, 37, w * h - 40)), bits(AR.rays(sc, w, h, z["pose"], z["rot"], 0.25, -0.25)[37:w * h - 3]))
    finally:
        r.set_pixel_offset(0.0, 0.0)
        r.set_frame_size(W, H)


def test_refused_offsets_change_nothing(ctx):
    r = ctx
    r.set_pixel_offset(0.25, -0.5)
    try:
        for dx, dy in ((float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0), (0.0, -float("inf")), (1.5, 0.0), (0.0, -1.0001), (-1.0000001192092896, 0.0)):
            assert r.lib.adanerf_set_pixel_offset(r.handle, dx, dy) == EINVAL, (dx, dy)
            assert "adanerf_set_pixel_offset" in r.lib.adanerf_last_error(r.handle).decode()
            assert r.pixel_offset == (0.25, -0.5)
        assert r.lib.adanerf_get_pixel_offset(r.handle, None) == EINVAL
        for dx, dy in ((1.0, -1.0), (-1.0, 1.0)):      # the ends of the range are legal
            r.set_pixel_offset(dx, dy)
            assert r.pixel_offset == (dx, dy)
    finally:
        r.set_pixel_offset(0.0, 0.0)


def test_offsets_reach_the_rays_of_a_shard(model):
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), shard_world=2, shard_rank=1, strip_rows=4) as r:
        r.set_camera(z["pose"], z["rot"])
        n = r.info.rays_local
        assert n == 4 * W
        for dx, dy in AR.OFFSETS:
            r.set_pixel_offset(dx, dy)
            want = AR.rays(sc, W, H, z["pose"], z["rot"], dx, dy, strip_rows=4, world=2, rank=1)
            assert np.array_equal(bits(feature_rays(r, 0, n)), bits(want)), (dx, dy)


def test_offsets_reach_the_rays_of_a_coarse_fine_context(tmp_path_factory):
    z, sc, d = _model(tmp_path_factory, "classroom_coarse_fine_16_24")
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as r:
        assert r.info.sampler_mode == R.SAMPLER_COARSE_FINE
        r.set_camera(z["pose"], z["rot"])
        n, nc = W * H, r.info.num_samples_coarse
        off, cnt, total = (R.DeviceArray(r, (k,), np.int32) for k in (n, n, 16))
        key = R.DeviceArray(r, (n * nc,), np.uint32)
        try:
            for dx, dy in AR.OFFSETS:
                r.set_pixel_offset(dx, dy)
                rays = Canaried(r, n, 8, np.float32, CANARY_F32)
                try:
                    assert r.lib.adanerf_sample_uniform(r.handle, 0, n, rays.ptr, off.ptr, cnt.ptr, key.ptr, total.ptr) == 0
                    want = AR.rays(sc, W, H, z["pose"], z["rot"], dx, dy, camera_origin=True)
                    assert np.array_equal(bits(rays.get()), bits(want)), (dx, dy)
                finally:
                    rays.free()
        finally:
            for a in (off, cnt, total, key):
                a.free()


# ---- 3. the render path ------------------------------------------------------------------------------------

RENDER_PATHS = [("split", "classroom_n8_thr02", {}, -1), ("fp32", "classroom_n8_thr02", {}, -1), ("fp16", "classroom_n8_thr02", {}, -1),
                ("split", "syn_6x128_skip2", {}, -1), ("split", "classroom_n8_thr02", {}, 80)]


@pytest.mark.parametrize("sampling,case,kw,batch", RENDER_PATHS, ids=["split_fp16", "fp32", "fp16", "run_time_shaped", "batched_last_batch"])
def test_render_path_honours_the_offset(tmp_path_factory, sampling, case, kw, batch):
    z, sc, d = _model(tmp_path_factory, case)
    dx, dy = 0.25, -0.25
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H, batch_size=batch), sampling=sampling, **kw) as r:
        r.set_camera(z["pose"], z["rot"])
        r.set_pixel_offset(dx, dy)
        r.render_numpy()
        n = W * H
        want = AR.rays(sc, W, H, z["pose"], z["rot"], dx, dy)
        if batch > 0:      # ADANERF_BUF_RAYS holds the last batch
            assert r.info.batch_rays == batch and n % batch != 0
            first = (n // batch) * batch
            want, n = want[first:], n - first
        got = r.buffer(R.BUF_RAYS, np.float32, (n, 8))
        assert np.array_equal(bits(got), bits(want)), "%s: %d of %d words differ" % (sampling, int(np.count_nonzero(bits(got) != bits(want))), want.size)
        assert not np.array_equal(bits(want), bits(AR.rays(sc, W, H, z["pose"], z["rot"])[-n:]))


# ---- 4. / 5. back to the centre; a frame-size change ----------------------------------------------------------

def test_offset_zero_restores_the_frame(model):
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as fresh:
        fresh.set_camera(z["pose"], z["rot"])
        rgb0, rgba0, _ = fresh.render_numpy()
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as r:
        r.set_camera(z["pose"], z["rot"])
        r.set_pixel_offset(0.5, -0.25)
        rgb1, rgba1, _ = r.render_numpy()
        assert not np.array_equal(bits(rgb1), bits(rgb0))      # the offset shows in the frame
        r.set_pixel_offset(0.0, 0.0)
        rgb2, rgba2, _ = r.render_numpy()
    assert np.array_equal(bits(rgb2), bits(rgb0)) and np.array_equal(rgba2, rgba0)


def test_offset_survives_a_frame_size_change(ctx, model):
    z, sc, d = model
    r = ctx
    try:
        r.set_pixel_offset(0.25, -0.25)
        for w, h in ((97, 61), (W, H)):
            r.set_frame_size(w, h)
            assert r.pixel_offset == (0.25, -0.25)
            assert np.array_equal(bits(feature_rays(r, 0, w * h)), bits(AR.rays(sc, w, h, z["pose"], z["rot"], 0.25, -0.25))), (w, h)
    finally:
        r.set_pixel_offset(0.0, 0.0)
        r.set_frame_size(W, H)


# ---- 6. entry points that ignore the offset --------------------------------------------------------------------

def test_reproject_and_guard_calibration_ignore_the_offset(ctx, model):
    z, sc, d = model
    r = ctx
    n = W * H
    rgba, dm, acc, _ = RR.depth_scene(W, H, 1)
    src, dst = RR.src_pose(sc), RR.moved(sc, **RR.MOTIONS["lateral"])
    bufs = [R.DeviceArray(r, (n, 4), np.uint8).upload(rgba.reshape(n, 4)), R.DeviceArray(r, (n,), np.float32).upload(dm),
            R.DeviceArray(r, (n,), np.float32).upload(acc)]
    outs = []
    try:
        for dx, dy in ((0.0, 0.0), (0.5, 0.5)):
            r.set_pixel_offset(dx, dy)
            colour, depth, mask = Canaried(r, n, 4, np.uint8, 0xA5), Canaried(r, n, 0, np.float32, CANARY_F32), Canaried(r, n, 0, np.uint8, 0xA5)
            try:
                holes = r.reproject_device(bufs[0], bufs[1], bufs[2], src[0], src[1], dst[0], dst[1], colour.ptr, depth.ptr, mask.ptr, acc_min=RR.ACC_MIN,
                                           hole_rgba8=RR.HOLE)
                outs.append((colour.get().copy(), bits(depth.get()).copy(), mask.get().copy(), holes, r.calibrate_guard(2, 1, install=False, pair=True)))
            finally:
                for b in (colour, depth, mask):
                    b.free()
            assert r.pixel_offset == (dx, dy)      # the calibration puts the offset back
        a, b = outs
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
        want = RR.reproject_f32(sc, W, H, False, rgba, dm, acc, src[0], src[1], dst[0], dst[1])
        assert np.array_equal(a[0], want[0]) and a[3] == want[3]
        assert a[4] == b[4] and a[4][0] > 0.0
    finally:
        r.set_pixel_offset(0.0, 0.0)
        for b in bufs:
            b.free()


# ---- 7. accumulate and resolve --------------------------------------------------------------------------------

def frame_values(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 1.5, (n, 3)).astype(np.float32)      # below 0 and above 1 included
    flat = a.reshape(-1)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1e-40, 3e38, -3e38, 0.999999, 1.0 / 255.0]
    for k, v in enumerate(special[:flat.size]):
        flat[(7 * k + seed) % flat.size] = np.float32(v)
    return a


@pytest.mark.parametrize("n", [1, 85, 257, W * H])
def test_accumulate_and_resolve_equal_numpy_float32(ctx, n):
    r = ctx
    frames = [frame_values(n, seed) for seed in (1, 2, 3, 4)]
    d_frames = [R.DeviceArray(r, (n, 3), np.float32).upload(f) for f in frames]
    total = Canaried(r, n, 3, np.float32, CANARY_F32)
    try:
        want = None
        for k, (f, df) in enumerate(zip(frames, d_frames)):
            assert r.lib.adanerf_accumulate(r.handle, df.ptr, n, total.ptr, 1 if k == 0 else 0) == 0, r.lib.adanerf_last_error(r.handle).decode()
            want = AR.accumulate_f32(want, f, k == 0)
            assert same_f32(total.get(), want), "after frame %d" % k
            assert np.array_equal(bits(df.numpy()), bits(f)), "frame modified"
        assert np.isnan(want).any() and (n == 1 or np.isinf(want).any())
        for count in (1, 3, 4, 65536):
            mean, px = Canaried(r, n, 3, np.float32, CANARY_F32), Canaried(r, n, 4, np.uint8, 0xA5)
            try:
                assert r.lib.adanerf_resolve_mean(r.handle, total.ptr, n, count, px.ptr, mean.ptr) == 0
                want_m, want_px = AR.resolve_f32(want, count)
                got_m, got_px = mean.get(), px.get()
                assert same_f32(got_m, want_m) and np.array_equal(got_px, want_px), "frames %d: %d pixels differ" % (
                    count, int(np.count_nonzero(np.any(got_px != want_px, axis=1))))
                assert same_f32(total.get(), want), "sum modified"
                # either output alone
                mean2, px2 = Canaried(r, n, 3, np.float32, CANARY_F32), Canaried(r, n, 4, np.uint8, 0xA5)
                try:
                    assert r.lib.adanerf_resolve_mean(r.handle, total.ptr, n, count, None, mean2.ptr) == 0
                    assert r.lib.adanerf_resolve_mean(r.handle, total.ptr, n, count, px2.ptr, None) == 0
                    assert same_f32(mean2.get(), want_m) and np.array_equal(px2.get(), want_px)
                finally:
                    mean2.free()
                    px2.free()
            finally:
                mean.free()
                px.free()
        # in place: the mean over the sum itself
        px = Canaried(r, n, 4, np.uint8, 0xA5)
        try:
            assert r.lib.adanerf_resolve_mean(r.handle, total.ptr, n, 3, px.ptr, total.ptr) == 0
            want_m, want_px = AR.resolve_f32(want, 3)
            assert same_f32(total.get(), want_m) and np.array_equal(px.get(), want_px)
        finally:
            px.free()
        # sum = sum + sum is legal too (identical ranges)
        assert r.lib.adanerf_accumulate(r.handle, total.ptr, n, total.ptr, 0) == 0
        assert same_f32(total.get(), AR.accumulate_f32(want_m, want_m, False))
    finally:
        total.free()
        for df in d_frames:
            df.free()


def test_one_frame_resolves_to_its_own_rgba8(ctx):
    r = ctx
    rgb, rgba, _ = r.render_numpy()
    n = r.info.rays_local
    assert len(np.unique(rgba[:, :3])) > 16
    px = Canaried(r, n, 4, np.uint8, 0xA5)
    try:
        r.resolve_mean_device(r._o_rgb, n, 1, px.ptr, None)
        assert np.array_equal(px.get(), rgba)
        assert np.array_equal(AR.rgba8_of(rgb), rgba)      # and the restatement states the same contract
    finally:
        px.free()


def test_accumulate_and_resolve_refusals(ctx):
    r = ctx
    n = 32
    big = Canaried(r, 4 * n, 3, np.float32, CANARY_F32)
    px = Canaried(r, n, 4, np.uint8, 0xA5)
    acc, res = r.lib.adanerf_accumulate, r.lib.adanerf_resolve_mean
    b, stride = big.ptr, n * 12
    try:
        bad_acc = [(None, n, b, 1), (b, n, None, 1), (b, -1, b + stride, 1), (b, 0x7fffffff // 3 + 1, b + stride, 1), (b + 2, n, b + stride, 1),
                   (b, n, b + stride + 1, 1), (b, n, b + 12, 0), (b + 12, n, b, 0), (b, n, b + stride - 4, 1)]
        for args in bad_acc:
            assert acc(r.handle, *args) == EINVAL, args
            assert "adanerf_accumulate" in r.lib.adanerf_last_error(r.handle).decode()
        bad_res = [(None, n, 1, px.ptr, b), (b, n, 1, None, None), (b, -1, 1, px.ptr, None), (b, 0x7fffffff // 3 + 1, 1, px.ptr, None),
                   (b, n, 0, px.ptr, None), (b, n, -4, px.ptr, None), (b, n, 65537, px.ptr, None), (b + 1, n, 1, px.ptr, None), (b, n, 1, px.ptr + 2, None),
                   (b, n, 1, None, b + stride + 2), (b, n, 1, None, b + 12), (b, n, 1, None, b + stride - 4), (b, n, 1, b + 8, None),
                   (b, n, 1, b + stride + 16, b + stride)]
        for args in bad_res:
            assert res(r.handle, *args) == EINVAL, args
            assert "adanerf_resolve_mean" in r.lib.adanerf_last_error(r.handle).decode()
        assert acc(None, b, n, b + stride, 1) == EINVAL and res(None, b, n, 1, px.ptr, None) == EINVAL
        assert big.untouched() and px.untouched()
        # n_rays == 0 does nothing; adjacent ranges do not overlap
        assert acc(r.handle, b, 0, b + stride, 1) == 0 and res(r.handle, b, 0, 1, px.ptr, None) == 0
        assert big.untouched() and px.untouched()
        assert acc(r.handle, b, n, b + stride, 1) == 0 and res(r.handle, b + stride, n, 65536, px.ptr, b + 2 * stride) == 0
        r.sync()
    finally:
        big.free()
        px.free()


# ---- 8. end to end ----------------------------------------------------------------------------------------

def test_render_supersampled_is_the_mean_of_its_frames(model):
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as r:
        r.set_camera(z["pose"], z["rot"])
        r.set_pixel_offset(0.125, -0.375)
        mean, rgba, st = r.render_supersampled(2)
        assert r.pixel_offset == (0.125, -0.375)      # the offset that was in force
        total, ms, samples = None, 0.0, 0
        for k, (dx, dy) in enumerate(AR.subpixel_grid(2)):
            r.set_pixel_offset(dx, dy)
            rgb, _, s1 = r.render_numpy()
            total = AR.accumulate_f32(total, rgb, k == 0)
            samples += s1.total_samples
        want_m, want_px = AR.resolve_f32(total, 4)
        assert np.array_equal(bits(mean), bits(want_m)) and np.array_equal(rgba, want_px)
        assert st.total_samples == samples // 4 and st.rays == W * H and st.batches == 4 and st.ms_total > 0
        assert len(np.unique(rgba[:, :3])) > 16
        # present() shows the resolved frame
        r.set_pixel_offset(0.0, 0.0)
        mean, rgba, _ = r.render_supersampled(2)
        assert np.array_equal(r.present(8, 6, filter="area"), AR.area_present(rgba.reshape(H, W, 4), 8, 6))
        one, rgba1, _ = r.render_supersampled(1)
        plain, rgba_plain, _ = r.render_numpy()
        assert np.array_equal(bits(one), bits(plain)) and np.array_equal(rgba1, rgba_plain)


def _bmp(path, w, h):
    bmp = open(path, "rb").read()
    assert int.from_bytes(bmp[18:22], "little") == w and int.from_bytes(bmp[22:26], "little") == h, path
    off = int.from_bytes(bmp[10:14], "little")
    row_bytes = (w * 3 + 3) & ~3
    px = np.frombuffer(bmp[off:off + row_bytes * h], dtype=np.uint8).reshape(h, row_bytes)[:, :w * 3].reshape(h, w, 3)
    return np.ascontiguousarray(px[::-1, :, ::-1])      # top-down RGB


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


def test_cli_supersample_and_present_filter(model):
    """`adanerf --supersample 2 -w` writes the library's resolved frame; `--present-filter area -s 32 24 -ws 16 12 --write-window` the
    area-filtered window image of the frame it rendered"""
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    names = ("out.bmp", "out_window.bmp")
    try:
        out = subprocess.run([exe, d, "-s", str(W), str(H), "--supersample", "2", "-w", "--frames", "1"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as r:
            r.set_camera(np.asarray(r.info.view_cell_center, np.float32), _cli_rotation(-80.0, 0.0))
            _, rgba, _ = r.render_supersampled(2)
        assert np.array_equal(_bmp(os.path.join(d, "out.bmp"), W, H), rgba[:, :3].reshape(H, W, 3)) and len(np.unique(rgba[:, :3])) > 16
        out = subprocess.run([exe, d, "-s", "32", "24", "-ws", "16", "12", "-w", "--write-window", "--present-filter", "area", "--frames", "1"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        frame = _bmp(os.path.join(d, "out.bmp"), 32, 24)
        rgba = np.concatenate([frame, np.full((24, 32, 1), 255, np.uint8)], axis=2)
        window = _bmp(os.path.join(d, "out_window.bmp"), 16, 12)
        assert np.array_equal(window, AR.area_present(rgba, 16, 12)[:, :, :3])
        assert not np.array_equal(window, P.present(rgba, 16, 12, 0)[:, :, :3])      # the default decimates
        for extra, word in ((["--reproject", "2"], "--reproject"), (["--oracle"], "--oracle"), (["--gpus", "2", "--same-device"], "--gpus 1")):
            out = subprocess.run([exe, d, "-s", str(W), str(H), "--supersample", "2", "--frames", "1"] + extra, capture_output=True, text=True, timeout=120)
            assert out.returncode != 0 and "--supersample" in out.stdout and word in out.stdout, extra
    finally:
        for name in names:
            if os.path.exists(os.path.join(d, name)):
                os.remove(os.path.join(d, name))


def test_evaluator_supersample(tmp_path):
    """evaluate(..., supersample=2) on a synthetic 12 x 10 dataset: every image is render_supersampled(2) of its pose, scored from the
    fp32 mean; records and summary carry `supersample`; a plain run keeps its keys"""
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
    poses = [(centre, O.camera_rotation(100.0, 0.0)), (centre + np.float32([0.05, 0.02, 0.0]), O.camera_rotation(103.0, 0.0))]
    frames, gts = [], []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        gts.append(np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
        write_png(str(ds / "test" / ("%05d.png" % i)), gts[-1])
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    summary, recs = evaluate(md, str(ds), "test", str(tmp_path / "pred"), precision="bf16", quiet=True, supersample=2)
    plain, precs = evaluate(md, str(ds), "test", None, precision="bf16", quiet=True)
    assert sorted(plain) == ["frames", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"] and "supersample" not in precs[0]
    assert sorted(summary) == sorted(list(plain) + ["supersample"]) and summary["supersample"] == 2
    assert [x["supersample"] for x in recs] == [2, 2]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w, h)) as r:
        for i, (pose, rot) in enumerate(poses):
            r.set_camera(pose, rot)
            mean, rgba, st = r.render_supersampled(2)
            assert np.array_equal(read_png(str(tmp_path / "pred" / ("%05d.png" % i))), rgba[:, :3].reshape(h, w, 3))
            ref = gts[i].astype(np.float32).reshape(-1, 3) / 255.0
            mse = float(np.mean((mean.astype(np.float64) - ref) ** 2))
            assert recs[i]["mse"] == mse and recs[i]["psnr"] == psnr_from_mse(mse)
            assert recs[i]["samples_per_ray"] == st.total_samples / float(w * h)
    # the scale sweep with the area filter: a frame rendered at 2 x, averaged to the dataset's size
    sweep, srecs = evaluate(md, str(ds), "test", None, precision="bf16", quiet=True, sweep_scales=[2.0], present_filter="area", max_frames=1)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, 2 * w, 2 * h)) as r:
        r.set_camera(*poses[0])
        _, rgba, _ = r.render_numpy()
        small = AR.area_present(rgba.reshape(2 * h, 2 * w, 4), w, h)
    ref = gts[0].astype(np.float32).reshape(-1, 3) / 255.0
    mse = float(np.mean(((small[:, :, :3].reshape(-1, 3).astype(np.float32) / 255.0).astype(np.float64) - ref) ** 2))
    assert srecs[0]["mse"] == mse and sweep["sweep"][0]["scale"] == 2.0
