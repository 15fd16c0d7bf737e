"""adanerf_temporal_resolve on the GPU: every case is exact equality with tests/temporal_reference.py (temporal_f32, the definition in
include/adanerf_hip.h in numpy float32) for all six outputs -- colour bits, depth bits, count, the 8-bit image, mask and the rejected
count.  Colours are random fp32 with NaNs, +0 / -0 pairs and values outside [0, 1] planted in the current frame and in the history, over
the synthetic wall + box depth scene of tests/reproject_reference.py with far pixels of every kind; canaries sit before and after every
output and the sources are checked unmodified.  tests/test_temporal_cpu.py holds the condition that makes equality a fair demand
(float32 and float64 agree on the accepted pixels and nearest taps of these inputs).  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import reproject_reference as RR
import temporal_reference as TR
from conftest import case_weights, load_case, record

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
PAD = 64                       # canary elements on either side of every output
CANARY_F32 = np.float32(-1234.5)
LOOSE_TOL = 0.3                # a depth tolerance at which the moved cases accept a good share of their pixels (the history is not the
                               # current scene seen from elsewhere, only one like it)


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def _model(tmp_path_factory, name):
    z, meta, sc = load_case(name)
    d = str(tmp_path_factory.mktemp("temporal_" + name))
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


def inputs(sc, w, h, camera_origin, seed=1):
    """(current rgb / depth / acc, history rgb / depth / count, the history's pose): computed once per size, shared and never changed"""
    key = (w, h, camera_origin, seed)
    if key not in _INPUTS:
        hist = TR.history_at(sc, w, h, camera_origin, seed)
        arrays = TR.current_at(sc, w, h, seed) + hist[:3]
        for a in arrays:
            a.setflags(write=False)
        _INPUTS[key] = (arrays, hist[3])
    return _INPUTS[key]


_WANT = {}


def reference(sc, w, h, camera_origin, motion, clamp, with_depth, with_count, tol, with_hist=True, seed=1, alpha=TR.ALPHA):
    key = (w, h, camera_origin, motion, clamp, with_depth, with_count, tol, with_hist, seed, alpha)
    if key not in _WANT:
        (cr, cd, ca, hr, hd, hc), (pp, pr) = inputs(sc, w, h, camera_origin, seed)
        dst = RR.moved(sc, **RR.MOTIONS[motion])
        _WANT[key] = TR.temporal_f32(sc, w, h, camera_origin, cr, cd, ca, dst[0], dst[1], hr if with_hist else None, hd if with_depth else None,
                                     hc if with_count else None, pp, pr, alpha=alpha, depth_tol=tol, flags=TR.CLAMP if clamp else 0)
    return _WANT[key]


class Buffers:
    """the device side of one frame size: the six sources, five canaried outputs"""
    CANARIES = (CANARY_F32, CANARY_F32, 0xA5, 0xA5, 0xA5)
    NAMES = ("rgb", "depth", "count", "rgba8", "mask")

    def __init__(self, r, n, arrays):
        self.r, self.n = r, n
        dt = (np.float32, np.float32, np.float32, np.float32, np.float32, np.uint8)
        self.host = [np.ascontiguousarray(a, dtype=t) for a, t in zip(arrays, dt)]
        self.src = [R.DeviceArray(r, a.shape, a.dtype).upload(a) for a in self.host]
        t = PAD + n + PAD
        self.out = [R.DeviceArray(r, (t, 3), np.float32), R.DeviceArray(r, (t,), np.float32), R.DeviceArray(r, (t,), np.uint8),
                    R.DeviceArray(r, (t, 4), np.uint8), R.DeviceArray(r, (t,), np.uint8)]
        self.step = [12, 4, 1, 4, 1]      # bytes per element
        self.reset()

    def reset(self):
        for b, c in zip(self.out, self.CANARIES):
            b.upload(np.full(b.shape, c, b.dtype))

    def call(self, cur_pose, prev_pose, alpha=TR.ALPHA, tol=TR.DEPTH_TOL, acc_min=TR.ACC_MIN, flags=TR.CLAMP, src=(0, 1, 2, 3, 4, 5), outs=(0, 1, 2, 3, 4),
             rejected=True, handle=True):
        """the C ABI itself; returns (rc, rejected or None).  Keeps the float arrays alive over the call."""
        keep = [_f(cur_pose[0], 3), _f(cur_pose[1], 9), _f(prev_pose[0], 3), _f(prev_pose[1], 9)]
        n_rej = C.c_int32(-7)
        s = [self.src[k].ptr if k is not None else None for k in src]
        o = [self.out[k].ptr + self.step[k] * PAD if k in outs else None for k in range(5)]
        rc = self.r.lib.adanerf_temporal_resolve(self.r.handle if handle else None, s[0], s[1], s[2], keep[0][1], keep[1][1], s[3], s[4], s[5], keep[2][1],
                                                 keep[3][1], float(alpha), float(tol), float(acc_min), int(flags), o[0], o[1], o[2], o[3], o[4],
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


def check(b, sc, w, h, motion, clamp=True, with_depth=True, with_count=True, tol=TR.DEPTH_TOL, with_hist=True, camera_origin=False,
          outs=(0, 1, 2, 3, 4), rejected=True, alpha=TR.ALPHA):
    want = reference(sc, w, h, camera_origin, motion, clamp, with_depth, with_count, tol, with_hist, alpha=alpha)
    dst = RR.moved(sc, **RR.MOTIONS[motion])
    prev = inputs(sc, w, h, camera_origin)[1]
    b.reset()
    src = (0, 1, 2, 3 if with_hist else None, 4 if with_depth else None, 5 if with_count else None)
    rc, got_rejected = b.call(dst, prev if with_hist else (None, None), alpha=alpha, tol=tol, flags=TR.CLAMP if clamp else 0, src=src, outs=outs,
                              rejected=rejected)
    assert rc == 0, b.r.lib.adanerf_last_error(b.r.handle).decode()
    got = b.outputs()
    tag = "%dx%d %s clamp %d depth %d count %d tol %g" % (w, h, motion, clamp, with_depth, with_count, tol)
    compare(got, got_rejected, want, tag, outs, rejected)
    return got, got_rejected, want


@pytest.fixture(scope="module")
def sized(ctx, model):
    """device buffers per frame size, made on first use"""
    made = {}

    def get(w, h):
        ctx.set_frame_size(w, h)
        if (w, h) not in made:
            made[(w, h)] = Buffers(ctx, w * h, inputs(model[1], w, h, False)[0])
        return made[(w, h)]
    yield get
    for b in made.values():
        b.free()


@pytest.mark.parametrize("w,h", RR.SIZES, ids=["%dx%d" % s for s in RR.SIZES])
def test_every_motion_equals_the_definition(ctx, model, sized, w, h):
    """every motion x clamp x history depth x count, at the hosts' depth tolerance; and at a loose one, where the moved cases blend a
    good share of their pixels through all four bilinear taps"""
    b = sized(w, h)
    blended = 0
    for motion in RR.MOTIONS:
        for clamp in (True, False):
            for with_depth in (True, False):
                for with_count in (True, False):
                    got, rej, want = check(b, model[1], w, h, motion, clamp, with_depth, with_count)
                    if motion == "sees_none":
                        assert rej == w * h and np.array_equal(bits(got[0]), bits(b.host[0])) and np.all(got[2] == 1)
                    if motion != "identity":
                        blended += w * h - rej
        check(b, model[1], w, h, motion, True, True, True, tol=LOOSE_TOL)
    if w * h > 100:
        assert blended > w * h      # the moved cases are not all rejection


def test_far_pixels_of_every_kind_and_counts_at_the_ceiling(ctx, model, sized):
    """what the inputs hold, so that the equality above says something about them"""
    w, h = RR.SIZES[0]
    b = sized(w, h)
    got, rej, want = check(b, model[1], w, h, "identity")
    cr, cd, ca, hr, hd, hc = b.host
    assert np.isnan(cr).any() and np.isnan(hr).any() and (cr < 0).any() and (cr > 1).any() and (hr < 0).any() and (hr > 1).any()
    for img in (cr, hr):
        z = bits(img)
        assert (z == 0x80000000).any() and (z == 0).any()
    assert np.isnan(cd).any() and np.isinf(cd).any() and (cd < 0).any() and np.isnan(ca).any() and (ca == 0).any() and ((ca > 0) & (ca < TR.ACC_MIN)).any()
    assert np.isinf(got[1]).any() and np.isinf(hd).any() and np.isfinite(got[1]).any()
    assert (hc == 254).any() and (hc == 255).any()
    ok = want.accepted
    assert np.all(got[2][ok & (hc[np.maximum(want.tap, 0)] >= 254)] == 255) and (got[2] == 255).any() and np.all(got[2][~ok] == 1)
    # a far pixel over a far history pixel is accepted, over a near one it is not
    far = np.isinf(got[1])
    assert (far & ok).any() and (far & ~ok).any() and np.all(np.isinf(hd[want.tap[far & ok]]))


def test_optional_outputs_may_be_null(ctx, model, sized):
    w, h = RR.SIZES[0]
    b = sized(w, h)
    check(b, model[1], w, h, "lateral", outs=(0,), tol=LOOSE_TOL)
    check(b, model[1], w, h, "lateral", outs=(0, 1, 2), rejected=False, tol=LOOSE_TOL)
    check(b, model[1], w, h, "forward", outs=(0, 3), tol=LOOSE_TOL)
    check(b, model[1], w, h, "backward", outs=(0, 4), rejected=False)


@pytest.mark.parametrize("w,h", RR.SIZES[:2] + RR.SIZES[3:], ids=["%dx%d" % s for s in RR.SIZES[:2] + RR.SIZES[3:]])
def test_no_history_copies_the_current_frame(ctx, model, sized, w, h):
    b = sized(w, h)
    for clamp in (True, False):
        got, rej, want = check(b, model[1], w, h, "lateral", clamp=clamp, with_hist=False, with_depth=False, with_count=False)
        assert rej == w * h and np.all(got[4] == 0) and np.all(got[2] == 1) and np.array_equal(bits(got[0]), bits(b.host[0]))
    # the history's depth and count alone are not a history, and the previous pose is not read: NULL, or not finite
    b.reset()
    dst = RR.moved(model[1], **RR.MOTIONS["lateral"])
    bad = (np.full(3, np.nan, np.float32), np.full(9, np.inf, np.float32))
    for prev in ((None, None), bad):
        rc, rej = b.call(dst, prev, src=(0, 1, 2, None, 4, 5))
        assert rc == 0 and rej == w * h
        assert np.array_equal(bits(b.outputs()[0]), bits(b.host[0]))


def test_coarse_fine_depths_count_from_the_camera(ctx_cf):
    r, sc = ctx_cf
    w, h = RR.SIZES[0]
    r.set_frame_size(w, h)
    b = Buffers(r, w * h, inputs(sc, w, h, True)[0])
    try:
        got, rej, want = check(b, sc, w, h, "lateral", camera_origin=True, tol=LOOSE_TOL)
        # and the origin matters on this input: from the sphere exit the same frame resolves differently
        (cr, cd, ca, hr, hd, hc), (pp, pr) = inputs(sc, w, h, True)
        dst = RR.moved(sc, **RR.MOTIONS["lateral"])
        other = TR.temporal_f32(sc, w, h, False, cr, cd, ca, dst[0], dst[1], hr, hd, hc, pp, pr, depth_tol=LOOSE_TOL)
        assert not np.array_equal(other.mask, got[4]) and not np.array_equal(bits(other.depth), bits(got[1]))
    finally:
        b.free()


def test_same_bits_on_every_call_and_across_frame_sizes(ctx, model, sized):
    big, small = RR.SIZES[0], RR.SIZES[1]
    first = check(sized(*big), model[1], big[0], big[1], "backward", tol=LOOSE_TOL)
    again = check(sized(*big), model[1], big[0], big[1], "backward", tol=LOOSE_TOL)
    check(sized(*small), model[1], small[0], small[1], "lateral")
    third = check(sized(*big), model[1], big[0], big[1], "backward", tol=LOOSE_TOL)
    for other in (again, third):
        assert first[1] == other[1]
        for a, c in zip(first[0], other[0]):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(c).view(np.uint8))


def test_refused_arguments(ctx, model, sized, tmp_path_factory):
    r, sc = ctx, model[1]
    w, h = RR.SIZES[1]
    b = sized(w, h)
    b.reset()
    n = w * h
    cur, prev = RR.moved(sc, **RR.MOTIONS["lateral"]), inputs(sc, w, h, False)[1]
    nan_pos, inf_rot = cur[0].copy(), cur[1].copy()
    nan_pos[1], inf_rot[2, 0] = np.nan, np.inf
    cases = [dict(src=(None, 1, 2, 3, 4, 5)), dict(src=(0, None, 2, 3, 4, 5)), dict(src=(0, 1, None, 3, 4, 5)), dict(outs=(1, 2, 3, 4)),
             dict(cur_pose=(nan_pos, cur[1])), dict(cur_pose=(cur[0], inf_rot)), dict(prev_pose=(nan_pos, prev[1])), dict(prev_pose=(prev[0], inf_rot)),
             dict(cur_pose=(None, cur[1])), dict(cur_pose=(cur[0], None)), dict(prev_pose=(None, prev[1])), dict(prev_pose=(prev[0], None)),
             dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.0000001), dict(alpha=float("nan")), dict(alpha=float("inf")),
             dict(tol=-0.01), dict(tol=float("nan")), dict(acc_min=float("nan")), dict(acc_min=-0.25), dict(flags=2), dict(flags=3), dict(flags=-1)]
    for kw in cases:
        args = dict(cur_pose=cur, prev_pose=prev)
        args.update(kw)
        rc, rej = b.call(args.pop("cur_pose"), args.pop("prev_pose"), **args)
        assert rc == EINVAL and rej == -7, kw
        assert "adanerf_temporal_resolve" in r.lib.adanerf_last_error(r.handle).decode(), kw
        assert b.untouched(), kw
    f = [_f(cur[0], 3), _f(cur[1], 9), _f(prev[0], 3), _f(prev[1], 9)]
    lib = r.lib

    def raw(cur_rgb, hist_rgb, hist_depth, hist_count, out_rgb, out_depth=None, out_count=None, out_rgba8=None, cur_depth=None):
        return lib.adanerf_temporal_resolve(r.handle, cur_rgb, cur_depth or b.src[1].ptr, b.src[2].ptr, f[0][1], f[1][1], hist_rgb, hist_depth, hist_count,
                                            f[2][1], f[3][1], 0.1, 0.02, 0.5, 1, out_rgb, out_depth, out_count, out_rgba8, None, None)
    big = R.DeviceArray(r, (4 * n, 3), np.float32).upload(np.full((4 * n, 3), 0.25, np.float32))
    small = R.DeviceArray(r, (4 * n,), np.float32).upload(np.full(4 * n, 2.5, np.float32))
    try:
        s = [p.ptr for p in b.src]
        # misaligned pointers
        for kw in (dict(cur_rgb=s[0] + 2), dict(hist_rgb=s[3] + 1), dict(hist_depth=s[4] + 2), dict(out_rgb=big.ptr + 1), dict(out_depth=small.ptr + 2),
                   dict(out_rgba8=small.ptr + 3), dict(cur_depth=s[1] + 2)):
            args = dict(cur_rgb=s[0], hist_rgb=s[3], hist_depth=s[4], hist_count=s[5], out_rgb=big.ptr)
            args.update(kw)
            assert raw(**args) == EINVAL and "aligned" in lib.adanerf_last_error(r.handle).decode(), kw
        # an output overlapping what it is gathered from: the same start; one shared pixel at either end
        for off in (n, 1, 2 * n - 1):
            assert raw(big.ptr + 12 * n, s[3], s[4], s[5], big.ptr + 12 * off) == EINVAL and "overlap" in lib.adanerf_last_error(r.handle).decode(), off
            assert raw(s[0], big.ptr + 12 * n, s[4], s[5], big.ptr + 12 * off) == EINVAL and "overlap" in lib.adanerf_last_error(r.handle).decode(), off
            assert raw(s[0], s[3], small.ptr + 4 * n, s[5], big.ptr, out_depth=small.ptr + 4 * off) == EINVAL, off
            assert raw(s[0], s[3], s[4], small.ptr + n, big.ptr, out_count=small.ptr + off) == EINVAL, off
        r.sync()
        assert np.all(big.numpy() == 0.25) and np.all(small.numpy() == 2.5) and b.untouched()
        # adjacent ranges do not overlap; alpha 1, depth_tol 0 and acc_min 0 are legal
        assert raw(big.ptr + 12 * n, s[3], s[4], s[5], big.ptr) == 0 and raw(big.ptr + 12 * n, s[3], s[4], s[5], big.ptr + 24 * n) == 0
        assert lib.adanerf_temporal_resolve(r.handle, s[0], s[1], s[2], f[0][1], f[1][1], s[3], s[4], s[5], f[2][1], f[3][1], 1.0, 0.0, 0.0, 0,
                                            big.ptr, None, None, None, None, None) == 0
        r.sync()
    finally:
        big.free()
        small.free()
    assert b.call(cur, prev, handle=False)[0] == EINVAL and b.untouched()
    rc, rej = b.call(cur, prev)
    assert rc == 0 and rej >= 0
    # a useNDC model; a context that renders one of two shards
    z, sc_ndc, d_ndc = _model(tmp_path_factory, "ndc_synthetic_n8")
    for d, kw, word in ((d_ndc, dict(), "NDC"), (model[2], dict(shard_world=2, shard_rank=0), "shard_world")):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, 16), **kw) as r2:
            b2 = Buffers(r2, w * 16, inputs(sc, w, 16, False)[0])
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


FRAME = (48, 32)


@pytest.fixture(scope="module")
def at_rest(model):
    """classroom_n8_thr02 at 48 x 32, the camera still: K = 16 render_temporal calls with grid 2 at the hosts' defaults, shared by the two
    tests below.  (the supersampled still, one un-jittered render, the 16th resolved frame, rejected per call)"""
    z, sc, d = model
    w, h = FRAME
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        with pytest.raises(R.AdaNeRFError):
            r.render_temporal()                                  # not enabled
        r.set_camera(z["pose"], z["rot"])
        still = r.render_supersampled(2)[0]
        plain = r.render_numpy()[0]
        r.enable_temporal(grid=2)
        assert r.pixel_offset == (0.0, 0.0)
        rejected = []
        for k in range(16):
            rgb, rgba8, mask, rej, st = r.render_temporal()
            rejected.append(rej)
            assert rej == int(np.count_nonzero(mask == 0)) and rgb.shape == (w * h, 3) and rgba8.shape == (w * h, 4)
        assert r.pixel_offset == (0.0, 0.0)
        # a cut, and a frame size change, drop the history
        r.reset_temporal()
        assert r.render_temporal()[3] == w * h and r.render_temporal()[3] == 0
        r.set_frame_size(24, 16)
        out = r.render_temporal()
        assert out[3] == 24 * 16 and out[0].shape == (24 * 16, 3)
        assert r.render_temporal()[3] == 0
        # a pose that differs, by however little, brings the disocclusion test back: the call is the plain device call with the history's depth
        moved = (np.asarray(z["pose"], np.float32) + np.float32(1e-3)).astype(np.float32)
        hist, prev = r._ta_sets[r._ta_hist[0]], r._ta_hist[1:]
        r.set_camera(moved, z["rot"])
        got = r.render_temporal()
        check = [r.empty((24 * 16, 3), np.float32), r.empty((24 * 16,), np.uint8)]
        n_rej = r.temporal_resolve_device(r._o_rgb, r._rp_depth, r._rp_acc, moved, z["rot"], hist[0], hist[1], hist[2], prev[0], prev[1], check[0],
                                          out_mask=check[1])
        assert n_rej == got[3] and np.array_equal(check[1].numpy(), got[2]) and np.array_equal(bits(check[0].numpy()), bits(got[0]))
        n_free = r.temporal_resolve_device(r._o_rgb, r._rp_depth, r._rp_acc, moved, z["rot"], hist[0], None, hist[2], prev[0], prev[1], check[0])
        print("24 x 16, pose moved by 1e-3: rejected %d with the history's depth tested, %d without" % (n_rej, n_free))
    return still, plain, rgb, rejected


def test_rendered_frames_at_rest_converge_to_the_supersampled_still(at_rest):
    """after 16 calls the resolved frame is closer to render_supersampled(2)'s mean than one un-jittered render is"""
    still, plain, rgb, rejected = at_rest
    p_taa, p_plain = _psnr(rgb, still), _psnr(plain, still)
    print("PSNR against the supersampled still: after 16 temporal frames %.3f dB, one un-jittered render %.3f dB; rejected per call %s" % (
        p_taa, p_plain, rejected))
    record("temporal_at_rest", psnr_temporal=p_taa, psnr_plain=p_plain, rejected=rejected)
    assert rejected[0] == FRAME[0] * FRAME[1]
    assert p_taa > p_plain


def test_rendered_frames_at_rest_reject_nothing_after_the_first_call(at_rest):
    """`rejected` is 0 from the second call on: while the pose is the history's own, render_temporal does not test the history's depth
    (nothing is uncovered while the camera rests).  With the test applied at rest, half a pixel of jitter alone moves the depth of
    382 .. 653 of these 1 536 pixels past the 2 % tolerance (profiles/temporal_measured.md)."""
    still, plain, rgb, rejected = at_rest
    print("rejected per call at rest: %s" % rejected)
    assert all(v == 0 for v in rejected[1:])


LATERAL_STEP = 0.01      # of the view cell's size per frame


def test_rendered_frames_on_a_lateral_path_stay_closer_to_the_still(model):
    """Eight frames along a short lateral path (LATERAL_STEP of the view cell per frame): the resolved frame at the last pose is closer to
    that pose's supersampled mean than the single jittered frame rendered there.  The definition fed with the same device-rendered
    frames must satisfy this first (a property of the method at this step, established on the CPU); the device result equals the
    definition's exactly."""
    z, sc, d = model
    w, h = FRAME
    n = w * h
    frames = 8
    size = np.asarray(sc.view_cell_size, np.float32)
    poses = [(np.asarray(z["pose"], np.float32) + np.float32(LATERAL_STEP * k) * size * np.float32([1, 1, 0])).astype(np.float32) for k in range(frames)]
    rot = np.asarray(z["rot"], np.float32)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        r.set_camera(poses[-1], rot)
        still = r.render_supersampled(2)[0]
        r.enable_temporal(grid=2)
        ref = None      # the definition's history: (rgb, depth, count, pos)
        for k, pos in enumerate(poses):
            r.set_camera(pos, rot)
            rgb, rgba8, mask, rej, st = r.render_temporal()
            cur, dm, acc = r._o_rgb.numpy(), r._rp_depth.numpy(), r._rp_acc.numpy()      # the jittered frame the resolve was fed with
            hist = (None, None, None, None) if ref is None else ref
            want = TR.temporal_f32(sc, w, h, False, cur, dm, acc, pos, rot, hist[0], hist[1], hist[2], hist[3], rot)
            ref = (want.rgb, want.depth, want.count, pos)
            assert np.array_equal(bits(rgb), bits(want.rgb)) and np.array_equal(mask, want.mask) and rej == want.rejected, k
            assert np.array_equal(rgba8, want.rgba8), k
            side = r._ta_hist[0]
            assert np.array_equal(bits(r._ta_sets[side][1].numpy()), bits(want.depth)) and np.array_equal(r._ta_sets[side][2].numpy(), want.count), k
        p_ref, p_dev, p_single = _psnr(want.rgb, still), _psnr(rgb, still), _psnr(cur, still)
        print("lateral path, step %g of the view cell, %d frames: PSNR against the last pose's supersampled still: definition %.3f dB, device %.3f dB, "
              "the single jittered frame %.3f dB; margin %.3f dB; rejected at the last pose %d of %d" % (
                  LATERAL_STEP, frames, p_ref, p_dev, p_single, p_ref - p_single, rej, n))
        record("temporal_lateral_path", step=LATERAL_STEP, frames=frames, psnr_definition=p_ref, psnr_device=p_dev, psnr_single=p_single, rejected=rej,
               pixels=n)
        assert p_ref > p_single      # the definition on device-rendered inputs, first
        assert p_dev > p_single and p_dev == p_ref


# ---- hosts -----------------------------------------------------------------------------------------------------

def _bmp(path):
    bmp = open(path, "rb").read()
    return bmp[int.from_bytes(bmp[10:14], "little"):]


def test_cli_taa(model, tmp_path):
    """--taa over a script that holds the camera still runs end to end and writes the resolved frame; with a one-offset cycle and a `cut`
    in front of the last frame that frame is the CLI's plain frame, byte for byte, window image included"""
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    still, cut = tmp_path / "still.txt", tmp_path / "cut.txt"
    still.write_text("# still\n" * 5)
    cut.write_text("# still\n" * 4 + "cut\n")
    base = [exe, d, "-s", "64", "48", "-ws", "80", "60", "-w", "--write-window", "--log-camera"]
    images = []
    try:
        for extra in (["--script", str(still)], ["--script", str(cut), "--taa", "0.1", "--taa-grid", "1"], ["--script", str(still), "--taa", "0.1:0.05"]):
            for name in ("out.bmp", "out_window.bmp"):
                if os.path.exists(os.path.join(d, name)):
                    os.remove(os.path.join(d, name))
            out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            images.append((_bmp(os.path.join(d, "out.bmp")), _bmp(os.path.join(d, "out_window.bmp"))))
        assert images[1] == images[0]
        plain, taa = (np.frombuffer(images[k][0], np.uint8).astype(np.float64) for k in (0, 2))
        assert images[2][0] != images[0][0] and len(np.unique(taa)) > 16
        print("CLI --taa 0.1:0.05 after 5 still frames against the plain frame: mean |difference| %.3f of 255" % float(np.mean(np.abs(taa - plain))))
        # many shares, or the debug view of the sampling network: nothing to resolve
        out = subprocess.run([exe, d, "-s", "64", "48", "--gpus", "2", "--same-device", "--taa", "0.1", "--frames", "2"], capture_output=True, text=True,
                             timeout=120)
        assert out.returncode != 0 and "--taa resolves whole frames" in out.stdout
        out = subprocess.run([exe, d, "-s", "64", "48", "--oracle", "--taa", "0.1", "--frames", "2"], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "not with --oracle" in out.stdout
    finally:
        for name in ("out.bmp", "out_window.bmp"):
            if os.path.exists(os.path.join(d, name)):
                os.remove(os.path.join(d, name))


def test_evaluator_temporal_and_temporal_still(tmp_path):
    """evaluate(..., temporal=0.2) and evaluate(..., temporal_still=3) on a synthetic 12 x 10 dataset of three poses: the plain keys and
    frames are those of a run without the option; the temporal ones are what NeuralRenderer.render_temporal gives over the same sequence"""
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
    plain, precs = evaluate(md, str(ds), "test", str(tmp_path / "plain"), precision="bf16", quiet=True, metrics=("psnr", "flip"))
    extra = ["mean_psnr_temporal", "mean_flip_temporal", "mean_rejected_fraction"]
    for kw, keys in ((dict(temporal=0.2), extra), (dict(temporal_still=3), extra + ["temporal_still"]), (dict(temporal=0.2, temporal_still=3), extra + ["temporal_still"])):
        out = str(tmp_path / ("pred_" + "_".join(sorted(kw))))
        summary, recs = evaluate(md, str(ds), "test", out, precision="bf16", quiet=True, metrics=("psnr", "flip"), **kw)
        assert sorted(summary) == sorted(list(plain) + keys)
        alpha, still = kw.get("temporal", 0.1), kw.get("temporal_still", 0)
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w, h)) as r:
            r.enable_temporal(alpha=alpha, grid=2)
            for i, (pose, rot) in enumerate(poses):
                r.set_camera(pose, rot)
                if still:
                    r.reset_temporal()
                for _ in range(still or 1):
                    rgb, rgba8, mask, rejected, st = r.render_temporal()
                ref = gts[i].astype(np.float32).reshape(-1, 3) / 255.0
                mse = float(np.mean((rgb.astype(np.float64) - ref) ** 2))
                assert recs[i]["mse_temporal"] == mse and recs[i]["psnr_temporal"] == psnr_from_mse(mse), (kw, i)
                assert recs[i]["rejected_fraction"] == rejected / float(w * h) and 0.0 <= recs[i]["flip_temporal"] <= 1.0
                assert np.array_equal(read_png(os.path.join(out, "%05d_temporal.png" % i)), rgba8[:, :3].reshape(h, w, 3))
                assert np.array_equal(read_png(os.path.join(out, "%05d.png" % i)), read_png(str(tmp_path / "plain" / ("%05d.png" % i))))
                for key in ("psnr", "mse", "flip", "samples_per_ray"):
                    assert recs[i][key] == precs[i][key], (kw, i, key)
        if not still:
            assert recs[0]["rejected_fraction"] == 1.0      # the first pose of the sequence has no history
        assert summary["mean_psnr_temporal"] == float(np.mean([x["psnr_temporal"] for x in recs]))
        assert summary["mean_rejected_fraction"] == float(np.mean([x["rejected_fraction"] for x in recs]))
        assert summary["mean_psnr"] == plain["mean_psnr"] and summary["mean_flip"] == plain["mean_flip"]
        if still:
            assert summary["temporal_still"] == 3
