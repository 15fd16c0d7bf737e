"""adanerf_temporal_upsample on the GPU: every case is exact equality with tests/upsample_reference.py (upsample_f32, the definition in
include/adanerf_hip.h in numpy float32) for all six outputs -- colour bits, depth bits, count, the 8-bit image, mask and the rejected
count.  The inputs are those of the temporal tests (random fp32 colours with NaNs, +0 / -0 pairs and values outside [0, 1]; the wall + box
depth scene with far pixels of every kind) at the render size, and a history of the output size with counts 0, 1, 254 and 255 planted;
canaries sit before and after every output and the sources are checked unmodified.  tests/test_upsample_cpu.py holds the conditions that
make equality a fair demand.  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import antialias_reference as AR
import reproject_reference as RR
import upsample_reference as UR
from conftest import case_weights, load_case, record

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
PAD = 64                       # canary elements on either side of every output
CANARY_F32 = np.float32(-1234.5)
COMBOS = UR.COMBOS             # history depth, history count, clamp
CASES = [(w, h, s) for (w, h) in RR.SIZES for s in UR.SCALES[(w, h)]]


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def _model(tmp_path_factory, name):
    z, meta, sc = load_case(name)
    d = str(tmp_path_factory.mktemp("upsample_" + name))
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


_INPUTS = {}


def inputs(sc, w, h, s, camera_origin):
    """(current rgb / depth / acc at w x h, history rgb / depth / count at s w x s h, the history's pose): computed once, shared, never changed"""
    key = (w, h, s, camera_origin)
    if key not in _INPUTS:
        hist = UR.history_at(sc, w, h, s, camera_origin, UR.SEED)
        arrays = UR.current_at(sc, w, h, UR.SEED) + hist[:3]
        for a in arrays:
            a.setflags(write=False)
        _INPUTS[key] = (arrays, hist[3])
    return _INPUTS[key]


_WANT = {}


def reference(sc, w, h, s, camera_origin, motion, offset, with_depth, with_count, clamp, tol, with_hist=True, alpha=UR.ALPHA):
    key = (w, h, s, camera_origin, motion, offset, with_depth, with_count, clamp, tol, with_hist, alpha)
    if key not in _WANT:
        (cr, cd, ca, hr, hd, hc), (pp, pr) = inputs(sc, w, h, s, camera_origin)
        dst = RR.moved(sc, **RR.MOTIONS[motion])
        _WANT[key] = UR.upsample_f32(sc, w, h, s, camera_origin, cr, cd, ca, offset[0], offset[1], dst[0], dst[1], hr if with_hist else None,
                                     hd if with_depth else None, hc if with_count else None, pp, pr, alpha=alpha, depth_tol=tol,
                                     flags=UR.CLAMP if clamp else 0)
    return _WANT[key]


class Buffers:
    """the device side of one render size and scale: the six sources, five canaried outputs of the output size"""
    CANARIES = (CANARY_F32, CANARY_F32, 0xA5, 0xA5, 0xA5)
    NAMES = ("rgb", "depth", "count", "rgba8", "mask")

    def __init__(self, r, s, n_out, arrays):
        self.r, self.s, self.n = r, s, n_out
        dt = (np.float32, np.float32, np.float32, np.float32, np.float32, np.uint8)
        self.host = [np.ascontiguousarray(a, dtype=t) for a, t in zip(arrays, dt)]
        self.src = [R.DeviceArray(r, a.shape, a.dtype).upload(a) for a in self.host]
        t = PAD + n_out + PAD
        self.out = [R.DeviceArray(r, (t, 3), np.float32), R.DeviceArray(r, (t,), np.float32), R.DeviceArray(r, (t,), np.uint8),
                    R.DeviceArray(r, (t, 4), np.uint8), R.DeviceArray(r, (t,), np.uint8)]
        self.step = [12, 4, 1, 4, 1]      # bytes per element
        self.reset()

    def reset(self):
        for b, c in zip(self.out, self.CANARIES):
            b.upload(np.full(b.shape, c, b.dtype))

    def call(self, cur_pose, prev_pose, offset=(0.0, 0.0), scale=None, alpha=UR.ALPHA, tol=UR.TEST_TOL, acc_min=UR.ACC_MIN, flags=UR.CLAMP,
             src=(0, 1, 2, 3, 4, 5), outs=(0, 1, 2, 3, 4), rejected=True, handle=True):
        """the C ABI itself; returns (rc, rejected or None).  Keeps the float arrays alive over the call."""
        keep = [_f(cur_pose[0], 3), _f(cur_pose[1], 9), _f(prev_pose[0], 3), _f(prev_pose[1], 9)]
        n_rej = C.c_int32(-7)
        s = [self.src[k].ptr if k is not None else None for k in src]
        o = [self.out[k].ptr + self.step[k] * PAD if k in outs else None for k in range(5)]
        rc = self.r.lib.adanerf_temporal_upsample(self.r.handle if handle else None, self.s if scale is None else scale, s[0], s[1], s[2], float(offset[0]),
                                                  float(offset[1]), keep[0][1], keep[1][1], s[3], s[4], s[5], keep[2][1], keep[3][1], float(alpha),
                                                  float(tol), float(acc_min), int(flags), o[0], o[1], o[2], o[3], o[4],
                                                  C.byref(n_rej) if rejected else None)
        return rc, (n_rej.value if rejected else None)

    def outputs(self):
        """(rgb, depth, count, rgba8, mask) after a sync, canaries and sources checked"""
        self.r.sync()
        n = self.n
        got = [b.numpy() for b in self.out]
        for g, canary, what in zip(got, self.CANARIES, self.NAMES):
            assert np.all(g[:PAD] == canary) and np.all(g[PAD + n:] == canary), "wrote outside the %s output" % what
        for d, hst, what in zip(self.src, self.host, ("cur_rgb", "cur_depth_map", "cur_acc_map", "hist_rgb", "hist_depth", "hist_count")):
            assert np.array_equal(d.numpy().view(np.uint8), hst.view(np.uint8)), "source %s modified" % what
        return [g[PAD:PAD + n] for g in got]

    def untouched(self):
        self.r.sync()
        return all(np.all(b.numpy() == c) for b, c in zip(self.out, self.CANARIES))

    def free(self):
        for b in self.src + self.out:
            b.free()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare(got, got_rejected, want, tag, outs=(0, 1, 2, 3, 4), rejected=True):
    wants = (want.rgb, want.depth, want.count, want.rgba8, want.mask)
    diff = []
    for k, name in enumerate(Buffers.NAMES):
        if k in outs:
            g, v = (bits(got[k]), bits(wants[k])) if k < 2 else (got[k], wants[k])
            diff.append("%s %d" % (name, int(np.count_nonzero(g != v))))
        else:
            assert np.all(got[k] == Buffers.CANARIES[k]), "%s: NULL %s output written" % (tag, name)
    print("%s: rejected %s (reference %d of %d); values differing: %s" % (tag, got_rejected, want.rejected, want.mask.size, ", ".join(diff)))
    for k, name in enumerate(Buffers.NAMES):
        if k in outs:
            g, v = (bits(got[k]), bits(wants[k])) if k < 2 else (got[k], wants[k])
            assert np.array_equal(g, v), "%s: %s" % (tag, name)
    if rejected:
        assert got_rejected == want.rejected, tag


def check(b, sc, w, h, s, motion, offset=(0.0, 0.0), with_depth=True, with_count=True, clamp=True, tol=UR.TEST_TOL, with_hist=True,
          camera_origin=False, outs=(0, 1, 2, 3, 4), rejected=True, alpha=UR.ALPHA):
    offset = (float(offset[0]), float(offset[1]))
    want = reference(sc, w, h, s, camera_origin, motion, offset, with_depth, with_count, clamp, tol, with_hist, alpha=alpha)
    dst = RR.moved(sc, **RR.MOTIONS[motion])
    prev = inputs(sc, w, h, s, camera_origin)[1]
    b.reset()
    src = (0, 1, 2, 3 if with_hist else None, 4 if with_depth else None, 5 if with_count else None)
    rc, got_rejected = b.call(dst, prev if with_hist else (None, None), offset=offset, alpha=alpha, tol=tol, flags=UR.CLAMP if clamp else 0, src=src,
                              outs=outs, rejected=rejected)
    assert rc == 0, b.r.lib.adanerf_last_error(b.r.handle).decode()
    got = b.outputs()
    tag = "%dx%d x%d %s offset (%g, %g) depth %d count %d clamp %d tol %g" % (w, h, s, motion, offset[0], offset[1], with_depth, with_count, clamp, tol)
    compare(got, got_rejected, want, tag, outs, rejected)
    return got, got_rejected, want


@pytest.fixture(scope="module")
def sized(ctx, model):
    """device buffers per render size and scale, made on first use"""
    made = {}

    def get(w, h, s):
        ctx.set_frame_size(w, h)
        if (w, h, s) not in made:
            made[(w, h, s)] = Buffers(ctx, s, s * w * s * h, inputs(model[1], w, h, s, False)[0])
        return made[(w, h, s)]
    yield get
    for b in made.values():
        b.free()


@pytest.mark.parametrize("w,h,s", CASES, ids=["%dx%d_x%d" % c for c in CASES])
def test_every_motion_and_offset_equals_the_definition(ctx, model, sized, w, h, s):
    """every motion x (history depth, history count, clamp on and off), the offsets taken in turn; and every offset -- the grid's own,
    (0.37, -0.81), (1, -1), (0, 0) -- on the lateral move with everything on"""
    b = sized(w, h, s)
    for motion, offset, with_depth, with_count, clamp in UR.geometric_cases(s):
        got, rej, want = check(b, model[1], w, h, s, motion, offset, with_depth, with_count, clamp)
        if motion == "sees_none":
            assert rej == s * w * s * h and np.all(got[4] == 0)


def test_what_the_inputs_hold(ctx, model, sized):
    """far pixels of every kind, NaNs, signed zeros, the counts 0, 1, 254 and 255, all three mask values: so that the equality above says
    something about them"""
    w, h, s = 16, 12, 2
    b = sized(w, h, s)
    got, rej, want = check(b, model[1], w, h, s, "identity", AR.subpixel_grid(s)[3], tol=UR.DEPTH_TOL)
    cr, cd, ca, hr, hd, hc = b.host
    assert np.isnan(cr).any() and np.isnan(hr).any() and (cr < 0).any() and (cr > 1).any()
    for img in (cr, hr):
        z = bits(img)
        assert (z == 0x80000000).any() and (z == 0).any()
    assert np.isnan(cd).any() and np.isinf(cd).any() and (cd < 0).any() and np.isnan(ca).any() and (ca == 0).any() and ((ca > 0) & (ca < UR.ACC_MIN)).any()
    assert np.isinf(got[1]).any() and np.isinf(hd).any() and np.isfinite(got[1]).any()
    for v in (0, 1, 254, 255):
        assert (hc == v).any()
    assert set(np.unique(got[4])) == {0, 1, 2} and (got[2] == 255).any() and (got[2] == 0).any()
    live = got[4] == 1
    tapped = hc[np.maximum(want.tap, 0)]
    assert np.all(got[2][live] == np.minimum(tapped[live].astype(int) + want.inside[live], 255)) and np.all(tapped[got[4] == 2] == 0)
    assert np.all(got[2][~live] == want.inside[~live]) and want.inside.sum() == w * h      # one output pixel in s^2 holds the frame's own sample


def test_optional_outputs_may_be_null(ctx, model, sized):
    w, h, s = 16, 12, 3
    b = sized(w, h, s)
    check(b, model[1], w, h, s, "lateral", (0.37, -0.81), outs=(0,))
    check(b, model[1], w, h, s, "lateral", (0.37, -0.81), outs=(0, 1, 2), rejected=False)
    check(b, model[1], w, h, s, "forward", outs=(0, 3))
    check(b, model[1], w, h, s, "backward", outs=(0, 4), rejected=False)


@pytest.mark.parametrize("w,h,s", [(16, 12, 2), (1, 1, 4), (97, 61, 3)], ids=["16x12_x2", "1x1_x4", "97x61_x3"])
def test_no_history_shows_the_nearest_sample(ctx, model, sized, w, h, s):
    b = sized(w, h, s)
    for clamp in (True, False):
        for offset in ((0.0, 0.0), (0.37, -0.81)):
            got, rej, want = check(b, model[1], w, h, s, "lateral", offset, clamp=clamp, with_hist=False, with_depth=False, with_count=False)
            i = (want.iy[:, None] * w + want.ix[None, :]).reshape(-1)
            assert rej == s * w * s * h and np.all(got[4] == 0) and np.array_equal(got[2], want.inside.astype(np.uint8))
            assert np.array_equal(bits(got[0]), bits(b.host[0].reshape(-1, 3)[i]))
    # the history's depth and count alone are not a history, and the previous pose is not read: NULL, or not finite
    b.reset()
    dst = RR.moved(model[1], **RR.MOTIONS["lateral"])
    bad = (np.full(3, np.nan, np.float32), np.full(9, np.inf, np.float32))
    for prev in ((None, None), bad):
        rc, rej = b.call(dst, prev, src=(0, 1, 2, None, 4, 5))
        assert rc == 0 and rej == s * w * s * h
        b.outputs()


def test_coarse_fine_depths_count_from_the_camera(ctx_cf):
    r, sc = ctx_cf
    w, h, s = 16, 12, 2
    r.set_frame_size(w, h)
    b = Buffers(r, s, s * w * s * h, inputs(sc, w, h, s, True)[0])
    try:
        for motion in ("identity", "lateral", "forward"):
            for with_depth, with_count, clamp in COMBOS[:2]:
                got, rej, want = check(b, sc, w, h, s, motion, (0.25, -0.25), with_depth, with_count, clamp, camera_origin=True)
        # and the origin matters on this input: from the sphere exit the same frame resolves differently
        (cr, cd, ca, hr, hd, hc), (pp, pr) = inputs(sc, w, h, s, True)
        dst = RR.moved(sc, **RR.MOTIONS["lateral"])
        other = UR.upsample_f32(sc, w, h, s, False, cr, cd, ca, 0.25, -0.25, dst[0], dst[1], hr, hd, hc, pp, pr, depth_tol=UR.TEST_TOL)
        got, rej, want = check(b, sc, w, h, s, "lateral", (0.25, -0.25), camera_origin=True)
        assert not np.array_equal(bits(other.depth), bits(got[1]))
    finally:
        b.free()


def test_same_bits_on_every_call_and_across_frame_sizes(ctx, model, sized):
    big, small = (97, 61, 2), (16, 12, 4)
    first = check(sized(*big), model[1], *big, "backward", (0.37, -0.81))
    again = check(sized(*big), model[1], *big, "backward", (0.37, -0.81))
    check(sized(*small), model[1], *small, "lateral")      # the scratch buffer is the larger one's
    third = check(sized(*big), model[1], *big, "backward", (0.37, -0.81))
    for other in (again, third):
        assert first[1] == other[1]
        for a, c in zip(first[0], other[0]):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(c).view(np.uint8))


def test_refused_arguments(ctx, model, sized, tmp_path_factory):
    r, sc = ctx, model[1]
    w, h, s = 16, 12, 2
    b = sized(w, h, s)
    b.reset()
    n, N = w * h, s * w * s * h
    cur, prev = RR.moved(sc, **RR.MOTIONS["lateral"]), inputs(sc, w, h, s, False)[1]
    nan_pos, inf_rot = cur[0].copy(), cur[1].copy()
    nan_pos[1], inf_rot[2, 0] = np.nan, np.inf
    cases = [dict(src=(None, 1, 2, 3, 4, 5)), dict(src=(0, None, 2, 3, 4, 5)), dict(src=(0, 1, None, 3, 4, 5)), dict(outs=(1, 2, 3, 4)),
             dict(cur_pose=(nan_pos, cur[1])), dict(cur_pose=(cur[0], inf_rot)), dict(prev_pose=(nan_pos, prev[1])), dict(prev_pose=(prev[0], inf_rot)),
             dict(cur_pose=(None, cur[1])), dict(cur_pose=(cur[0], None)), dict(prev_pose=(None, prev[1])), dict(prev_pose=(prev[0], None)),
             dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.0000001), dict(alpha=float("nan")), dict(alpha=float("inf")),
             dict(tol=-0.01), dict(tol=float("nan")), dict(acc_min=float("nan")), dict(acc_min=-0.25), dict(flags=2), dict(flags=3), dict(flags=-1),
             dict(scale=0), dict(scale=5), dict(scale=-2), dict(offset=(1.0000001, 0.0)), dict(offset=(0.0, -1.5)), dict(offset=(float("nan"), 0.0)),
             dict(offset=(0.0, float("inf")))]
    for kw in cases:
        args = dict(cur_pose=cur, prev_pose=prev)
        args.update(kw)
        rc, rej = b.call(args.pop("cur_pose"), args.pop("prev_pose"), **args)
        assert rc == EINVAL and rej == -7, kw
        assert "adanerf_temporal_upsample" in r.lib.adanerf_last_error(r.handle).decode(), kw
        assert b.untouched(), kw
    f = [_f(cur[0], 3), _f(cur[1], 9), _f(prev[0], 3), _f(prev[1], 9)]
    lib = r.lib

    def raw(cur_rgb, hist_rgb, hist_depth, hist_count, out_rgb, out_depth=None, out_count=None, out_rgba8=None, cur_depth=None, cur_acc=None):
        return lib.adanerf_temporal_upsample(r.handle, s, cur_rgb, cur_depth or b.src[1].ptr, cur_acc or b.src[2].ptr, 0.25, -0.25, f[0][1], f[1][1], hist_rgb,
                                             hist_depth, hist_count, f[2][1], f[3][1], 0.1, 0.02, 0.5, 1, out_rgb, out_depth, out_count, out_rgba8, None, None)
    big = R.DeviceArray(r, (4 * N, 3), np.float32).upload(np.full((4 * N, 3), 0.25, np.float32))
    small = R.DeviceArray(r, (4 * N,), np.float32).upload(np.full(4 * N, 2.5, np.float32))
    try:
        p = [q.ptr for q in b.src]
        # misaligned pointers
        for kw in (dict(cur_rgb=p[0] + 2), dict(hist_rgb=p[3] + 1), dict(hist_depth=p[4] + 2), dict(out_rgb=big.ptr + 1), dict(out_depth=small.ptr + 2),
                   dict(out_rgba8=small.ptr + 3), dict(cur_depth=p[1] + 2)):
            args = dict(cur_rgb=p[0], hist_rgb=p[3], hist_depth=p[4], hist_count=p[5], out_rgb=big.ptr)
            args.update(kw)
            assert raw(**args) == EINVAL and "aligned" in lib.adanerf_last_error(r.handle).decode(), kw
        # an output overlapping what it is gathered from: the history (the output's size) and the current frame (the render size), by the
        # same start and by one shared pixel at either end
        for off in (N, 1, 2 * N - 1):
            assert raw(p[0], big.ptr + 12 * N, p[4], p[5], big.ptr + 12 * off) == EINVAL and "overlap" in lib.adanerf_last_error(r.handle).decode(), off
            assert raw(p[0], p[3], small.ptr + 4 * N, p[5], big.ptr, out_depth=small.ptr + 4 * off) == EINVAL, off
            assert raw(p[0], p[3], p[4], small.ptr + N, big.ptr, out_count=small.ptr + off) == EINVAL, off
        for off in (N, N + n - 1, 1):
            assert raw(big.ptr + 12 * N, p[3], p[4], p[5], big.ptr + 12 * off) == EINVAL and "overlap" in lib.adanerf_last_error(r.handle).decode(), off
            assert raw(p[0], p[3], p[4], p[5], big.ptr, out_depth=small.ptr + 4 * off, cur_depth=small.ptr + 4 * N) == EINVAL, off
            assert raw(p[0], p[3], p[4], p[5], big.ptr, out_depth=small.ptr + 4 * off, cur_acc=small.ptr + 4 * N) == EINVAL, off
        r.sync()
        assert np.all(big.numpy() == 0.25) and np.all(small.numpy() == 2.5) and b.untouched()
        # adjacent ranges do not overlap; alpha 1, depth_tol 0, acc_min 0 and an offset of exactly +-1 are legal
        assert raw(p[0], big.ptr + 12 * N, p[4], p[5], big.ptr) == 0 and raw(p[0], big.ptr + 12 * N, p[4], p[5], big.ptr + 24 * N) == 0
        assert raw(big.ptr + 12 * N, p[3], p[4], p[5], big.ptr) == 0 and raw(big.ptr + 12 * N, p[3], p[4], p[5], big.ptr + 12 * (N + n)) == 0
        assert lib.adanerf_temporal_upsample(r.handle, s, p[0], p[1], p[2], 1.0, -1.0, f[0][1], f[1][1], p[3], p[4], p[5], f[2][1], f[3][1], 1.0, 0.0, 0.0, 0,
                                             big.ptr, None, None, None, None, None) == 0
        r.sync()
    finally:
        big.free()
        small.free()
    assert b.call(cur, prev, handle=False)[0] == EINVAL and b.untouched()
    rc, rej = b.call(cur, prev)
    assert rc == 0 and rej >= 0
    # an output of 2^25 pixels: refused by its size, before anything is read (a context with a small batch, so that the 2048 x 1024 render
    # size costs it no memory)
    settings = adanerf_amd.Settings(model[2], w, h)
    settings.batch_size = 256
    with adanerf_amd.NeuralRenderer(settings) as r3:
        r3.set_frame_size(2048, 1024)
        b3 = Buffers(r3, 4, N, inputs(sc, w, h, s, False)[0])
        try:
            rc, rej = b3.call(cur, prev, scale=4)
            assert rc == EINVAL and rej == -7 and "2^25" in r3.lib.adanerf_last_error(r3.handle).decode()
            assert b3.untouched()
        finally:
            b3.free()
    # a useNDC model; a context that renders one of two shards
    z, sc_ndc, d_ndc = _model(tmp_path_factory, "ndc_synthetic_n8")
    for d, kw, word in ((d_ndc, dict(), "NDC"), (model[2], dict(shard_world=2, shard_rank=0), "shard_world")):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, 16), **kw) as r2:
            b2 = Buffers(r2, s, s * w * s * 16, inputs(sc, w, 16, s, False)[0])
            try:
                rc, rej = b2.call(cur, prev)
                assert rc == EUNSUPPORTED and rej == -7 and word in r2.lib.adanerf_last_error(r2.handle).decode()
                assert b2.untouched()
            finally:
                b2.free()


# ---- rendered frames ---------------------------------------------------------------------------------------

def _psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


RENDER, SCALE = (24, 16), 2
LATERAL_STEP = 0.01      # of the view cell's size per frame


def test_rendered_frames_on_a_lateral_path_equal_the_definition(model):
    """Eight frames along a short lateral path at render size 24 x 16, s = 2: render_upsampled equals upsample_f32 fed the same
    device-rendered frames, bit for bit on every frame, history depth and count included"""
    z, sc, d = model
    w, h = RENDER
    s = SCALE
    size = np.asarray(sc.view_cell_size, np.float32)
    poses = [(np.asarray(z["pose"], np.float32) + np.float32(LATERAL_STEP * k) * size * np.float32([1, 1, 0])).astype(np.float32) for k in range(8)]
    rot = np.asarray(z["rot"], np.float32)
    grid = AR.subpixel_grid(s)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        with pytest.raises(R.AdaNeRFError):
            r.render_upsampled()                                  # not enabled
        r.enable_temporal_upsample(scale=s)
        ref = None      # the definition's history: (rgb, depth, count, pos)
        for k, pos in enumerate(poses):
            r.set_camera(pos, rot)
            rgb, rgba8, mask, rej, st = r.render_upsampled()
            assert rgb.shape == (s * w * s * h, 3) and rgba8.shape == (s * w * s * h, 4) and st.rays == w * h
            cur, dm, acc = r._o_rgb.numpy(), r._rp_depth.numpy(), r._rp_acc.numpy()      # the jittered frame the resolve was fed with
            hist = (None, None, None, None) if ref is None else ref
            dx, dy = grid[k % len(grid)]
            want = UR.upsample_f32(sc, w, h, s, False, cur, dm, acc, dx, dy, pos, rot, hist[0], hist[1], hist[2], hist[3], rot)
            ref = (want.rgb, want.depth, want.count, pos)
            assert np.array_equal(bits(rgb), bits(want.rgb)) and np.array_equal(mask, want.mask) and rej == want.rejected, k
            assert np.array_equal(rgba8, want.rgba8), k
            side = r._tu_hist[0]
            assert np.array_equal(bits(r._tu_sets[side][1].numpy()), bits(want.depth)) and np.array_equal(r._tu_sets[side][2].numpy(), want.count), k
            print("frame %d: rejected %d of %d" % (k, rej, mask.size))
        assert r.pixel_offset == (0.0, 0.0)
        assert r.present(96, 64).shape == (64, 96, 4)      # the upsampled frame is the one presented
        # a cut, and a frame size change, drop the history
        r.reset_upsample()
        assert r.render_upsampled()[3] == s * w * s * h and r.render_upsampled()[3] < s * w * s * h
        r.set_frame_size(12, 8)
        out = r.render_upsampled()
        assert out[3] == s * 12 * s * 8 and out[0].shape == (s * 12 * s * 8, 3)


def _at_rest(model, clamp):
    """(PSNR of the upsampled 8-bit frame after s^2 calls at rest, PSNR of the un-jittered render enlarged by adanerf_present's linear
    filter, rejected per call), both against the native render of the output size"""
    z, sc, d = model
    w, h = RENDER
    s = SCALE
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, s * w, s * h)) as r:
        r.set_camera(z["pose"], z["rot"])
        native = r.render_numpy()[1].reshape(s * h, s * w, 4)[..., :3].astype(np.float64) / 255.0
        r.set_frame_size(w, h)
        r.render_numpy()
        enlarged = r.present(s * w, s * h, filter="linear")[..., :3].astype(np.float64) / 255.0
        r.enable_temporal_upsample(scale=s, clamp=clamp)
        rejected = []
        for k in range(s * s):
            rgb, rgba8, mask, rej, st = r.render_upsampled()
            rejected.append(rej)
        assert np.all(r._tu_sets[r._tu_hist[0]][2].numpy() == 1)      # every output pixel has had its own sample once
        up = rgba8.reshape(s * h, s * w, 4)[..., :3].astype(np.float64) / 255.0
    return _psnr(up, native), _psnr(enlarged, native), rejected


def test_rendered_frames_at_rest_beat_the_enlarged_small_render(model):
    """classroom_n8_thr02, render size 24 x 16, s = 2, the camera at rest from a cut, the clamp off: after 4 calls the PSNR of d_out_rgba8
    against a native 48 x 32 render exceeds that of the un-jittered 24 x 16 render enlarged by adanerf_present (linear).  The same pair
    with the clamp on is recorded, not asserted."""
    p_up, p_plain, rejected = _at_rest(model, clamp=False)
    c_up, c_plain, c_rejected = _at_rest(model, clamp=True)
    print("PSNR against the native 48 x 32 render: upsampled (clamp off) %.3f dB, (clamp on) %.3f dB, enlarged 24 x 16 render %.3f dB; rejected per call "
          "%s (clamp on: %s)" % (p_up, c_up, p_plain, rejected, c_rejected))
    record("upsample_at_rest", psnr_upsampled=p_up, psnr_upsampled_clamp=c_up, psnr_enlarged=p_plain, rejected=rejected)
    assert rejected[0] == SCALE * RENDER[0] * SCALE * RENDER[1] and all(v == 0 for v in rejected[1:])
    assert p_up > p_plain


# ---- hosts -----------------------------------------------------------------------------------------------------

def _bmp(path):
    bmp = open(path, "rb").read()
    return int.from_bytes(bmp[18:22], "little"), int.from_bytes(bmp[22:26], "little"), bmp[int.from_bytes(bmp[10:14], "little"):]


def test_cli_taau(model, tmp_path, tmp_path_factory):
    """--taau 2 over a script that holds the camera still runs end to end and writes the 2 W x 2 H frame (-w) and the window image made from
    it; with --taau 1 and a `cut` in front of the last frame that frame is the CLI's plain frame, byte for byte; a useNDC model is refused"""
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    still, cut = tmp_path / "still.txt", tmp_path / "cut.txt"
    still.write_text("# still\n" * 5)
    cut.write_text("# still\n" * 4 + "cut\n")
    base = [exe, d, "-s", "32", "24", "-ws", "80", "60", "-w", "--write-window", "--log-camera"]
    images = []
    try:
        for extra in (["--script", str(still)], ["--script", str(cut), "--taau", "1"], ["--script", str(still), "--taau", "2:0.1:0.05"]):
            for name in ("out.bmp", "out_window.bmp"):
                if os.path.exists(os.path.join(d, name)):
                    os.remove(os.path.join(d, name))
            out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            images.append((_bmp(os.path.join(d, "out.bmp")), _bmp(os.path.join(d, "out_window.bmp"))))
        assert images[1] == images[0] and images[0][0][:2] == (32, 24)
        assert images[2][0][:2] == (64, 48) and images[2][1][:2] == (80, 60)
        up = np.frombuffer(images[2][0][2], np.uint8)
        assert len(np.unique(up)) > 16 and images[2][1][2] != images[0][1][2]
    finally:
        for name in ("out.bmp", "out_window.bmp"):
            if os.path.exists(os.path.join(d, name)):
                os.remove(os.path.join(d, name))
    d_ndc = _model(tmp_path_factory, "ndc_synthetic_n8")[2]
    out = subprocess.run([exe, d_ndc, "-s", "32", "24", "--taau", "2", "--frames", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--taau: the depth of a useNDC model is NDC depth" in out.stdout


def test_evaluator_temporal_upsample(tmp_path):
    """evaluate(..., temporal_upsample=2) on a synthetic 12 x 10 dataset of three poses: the upsampled keys are what
    NeuralRenderer.render_upsampled gives per pose at rest from a cut, the plain frame is the 6 x 5 render enlarged by the linear present"""
    from adanerf_amd.evaluate import evaluate, psnr_from_mse
    from adanerf_amd.png import read_png, write_png
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    w, h, s = 12, 10, 2
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[w, h], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    centre = np.array(sc.view_cell_center, np.float32)
    poses = [(centre, O.camera_rotation(100.0, 0.0)), (centre + np.float32([0.01, 0.005, 0.0]), O.camera_rotation(100.5, 0.0)),
             (centre + np.float32([0.02, 0.01, 0.0]), O.camera_rotation(101.0, 0.0))]
    frames, gts = [], []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        gts.append(np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
        write_png(str(ds / "test" / ("%05d.png" % i)), gts[-1])
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    with pytest.raises(ValueError):
        evaluate(md, str(ds), "test", None, precision="bf16", quiet=True, temporal_upsample=4)      # 12 x 10 does not divide by 4
    plain_keys = ["frames", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    for kw, k_frames in ((dict(temporal_upsample=s), s * s), (dict(temporal_upsample=s, temporal_upsample_frames=6), 6)):
        out = str(tmp_path / ("pred_%d" % k_frames))
        summary, recs = evaluate(md, str(ds), "test", out, precision="bf16", quiet=True, metrics=("psnr", "flip"), **kw)
        assert sorted(summary) == sorted(plain_keys + ["mean_psnr_upsampled", "mean_flip_upsampled", "mean_rejected_fraction", "temporal_upsample",
                                                       "temporal_upsample_frames"])
        assert summary["temporal_upsample"] == s and summary["temporal_upsample_frames"] == k_frames
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w // s, h // s)) as r:
            r.enable_temporal_upsample(scale=s)
            for i, (pose, rot) in enumerate(poses):
                r.set_camera(pose, rot)
                small, _, st = r.render_numpy()
                enlarged = r.present(w, h, filter="linear")
                r.reset_upsample()
                for _ in range(k_frames):
                    rgb, rgba8, mask, rejected, _ = r.render_upsampled()
                ref = gts[i].astype(np.float32).reshape(-1, 3) / 255.0
                mse = float(np.mean((rgb.astype(np.float64) - ref) ** 2))
                assert recs[i]["mse_upsampled"] == mse and recs[i]["psnr_upsampled"] == psnr_from_mse(mse), (kw, i)
                assert recs[i]["rejected_fraction"] == rejected / float(w * h) == 0.0 and 0.0 <= recs[i]["flip_upsampled"] <= 1.0
                assert np.array_equal(read_png(os.path.join(out, "%05d_upsampled.png" % i)), rgba8[:, :3].reshape(h, w, 3))
                assert np.array_equal(read_png(os.path.join(out, "%05d.png" % i)), enlarged[..., :3])
                shown = enlarged[..., :3].reshape(-1, 3).astype(np.float32) / 255.0      # scored from the 8-bit image, as the evaluator's sweeps are
                assert recs[i]["mse"] == float(np.mean((shown.astype(np.float64) - ref) ** 2)) and recs[i]["samples_per_ray"] == st.total_samples / float((w // s) * (h // s))
        assert summary["mean_psnr_upsampled"] == float(np.mean([x["psnr_upsampled"] for x in recs]))
        assert summary["mean_rejected_fraction"] == 0.0
