"""adanerf_reproject_pair on the GPU: every case is exact equality with tests/reproject_pair_reference.py (pair_f32, the definition in
include/adanerf_hip.h in numpy float32) for all five outputs -- fp32 colour bits, the 8-bit image, depth bits, mask, source -- and the
hole count; against the library's own adanerf_reproject on the same inputs; canaries before and after every output, the sources read
back unmodified.  tests/test_reproject_pair_cpu.py holds the condition that makes equality a fair demand (float32 and float64 agree on
the winners and on the agree / disagree decision of these inputs).  Then the three hosts.  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import reproject_pair_reference as P
import reproject_reference as RR
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
PAD = 64                       # canary elements on either side of every output
CANARY_F32 = np.float32(-1234.5)
WEIGHTS, TOLS = (0.0, 0.3, 1.0), (0.0, 0.05)


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


def _model(tmp_path_factory, name):
    z, meta, sc = load_case(name)
    d = str(tmp_path_factory.mktemp("pair_" + name))
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


_WANT = {}


def reference(sc, w, h, camera_origin, name, weight_b, tol, flags):
    key = (id(sc), w, h, camera_origin, name, weight_b, tol, flags)
    if key not in _WANT:
        a, b, dp, dr = P.case(sc, w, h, camera_origin, name)
        _WANT[key] = P.pair_f32(sc, w, h, camera_origin, a, b, dp, dr, weight_b=weight_b, depth_tol=tol, flags=flags)
    return _WANT[key]


class Buffers:
    """the device side of one case: the six source images (A: 0..2, B: 3..5), five canaried outputs"""
    CANARIES = (CANARY_F32, 0xA5, CANARY_F32, 0xA5, 0xA5)
    NAMES = ("rgb", "rgba8", "depth", "mask", "source")

    def __init__(self, r, n, a, b):
        self.r, self.n = r, n
        self.poses = ((a.pos, a.rot), (b.pos, b.rot))
        self.host = [np.ascontiguousarray(x, dtype=np.float32) for x in (a.rgb, a.depth, a.acc, b.rgb, b.depth, b.acc)]
        self.src = [R.DeviceArray(r, x.shape, x.dtype).upload(x) for x in self.host]
        t = PAD + n + PAD
        self.out = [R.DeviceArray(r, (t, 3), np.float32), R.DeviceArray(r, (t, 4), np.uint8), R.DeviceArray(r, (t,), np.float32),
                    R.DeviceArray(r, (t,), np.uint8), R.DeviceArray(r, (t,), np.uint8)]
        self.step = [12, 4, 4, 1, 1]      # bytes per element
        self.reset()

    def reset(self):
        for b, c in zip(self.out, self.CANARIES):
            b.upload(np.full(b.shape, c, b.dtype))

    def call(self, dst_pose, weight_b=0.5, acc_min=RR.ACC_MIN, tol=P.DEPTH_TOL, hole=RR.HOLE, flags=0, src=(0, 1, 2, 3, 4, 5), outs=(0, 1, 2, 3, 4), holes=True,
             handle=True, a_pose=None, b_pose=None, src_ptr=None, out_ptr=None, null_pose=None):
        """the C ABI itself; returns (rc, holes or None).  src_ptr / out_ptr: {index: address} in place of a buffer's own; null_pose: the
        index (0..5: a_pos, a_rot, b_pos, b_rot, dst_pos, dst_rot) of a pose pointer handed over as NULL."""
        pa, pb = a_pose or self.poses[0], b_pose or self.poses[1]
        keep = [_f(pa[0], 3), _f(pa[1], 9), _f(pb[0], 3), _f(pb[1], 9), _f(dst_pose[0], 3), _f(dst_pose[1], 9)]
        fp = [None if k == null_pose else keep[k][1] for k in range(6)]
        n_holes = C.c_int32(-7)
        s = [self.src[k].ptr if k is not None else None for k in src]
        o = [self.out[k].ptr + self.step[k] * PAD if k in outs else None for k in range(5)]
        for k, p in (src_ptr or {}).items():
            s[k] = p
        for k, p in (out_ptr or {}).items():
            o[k] = p
        rc = self.r.lib.adanerf_reproject_pair(self.r.handle if handle else None, s[0], s[1], s[2], fp[0], fp[1], s[3], s[4], s[5], fp[2], fp[3], fp[4], fp[5],
                                               float(weight_b), float(acc_min), float(tol), int(hole), int(flags), o[0], o[1], o[2], o[3], o[4],
                                               C.byref(n_holes) if holes else None)
        return rc, (n_holes.value if holes else None)

    def outputs(self):
        """(rgb, rgba8, depth, mask, source) after a sync, canaries and sources checked"""
        self.r.sync()
        n = self.n
        got = [b.numpy() for b in self.out]
        for g, canary, what in zip(got, self.CANARIES, self.NAMES):
            assert np.all(g[:PAD] == canary) and np.all(g[PAD + n:] == canary), "wrote outside the %s output" % what
        self.sources_unmodified()
        return [g[PAD:PAD + n] for g in got]

    def sources_unmodified(self):
        for k, (d, hst) in enumerate(zip(self.src, self.host)):
            assert np.array_equal(d.numpy().view(np.uint8).reshape(-1), hst.view(np.uint8).reshape(-1)), "source image %d modified" % k

    def untouched(self):
        self.r.sync()
        return all(np.all(b.numpy() == c) for b, c in zip(self.out, self.CANARIES))

    def free(self):
        for b in self.src + self.out:
            b.free()


def check(b, sc, w, h, name, weight_b=0.3, tol=P.DEPTH_TOL, flags=RR.FILL, camera_origin=False, outs=(0, 1, 2, 3, 4), holes=True):
    """one call against the definition; b: the Buffers of this case on a context whose frame size is (w, h)"""
    want = reference(sc, w, h, camera_origin, name, weight_b, tol, flags)
    dst = P.case(sc, w, h, camera_origin, name)[2:4]
    b.reset()
    rc, got_holes = b.call(dst, weight_b=weight_b, tol=tol, flags=flags, outs=outs, holes=holes)
    assert rc == 0, b.r.lib.adanerf_last_error(b.r.handle).decode()
    got = b.outputs()
    exp = [np.ascontiguousarray(want.rgb).view(np.uint32), want.rgba8, want.depth.view(np.uint32), want.mask, want.source]
    got_cmp = [got[0].view(np.uint32), got[1], got[2].view(np.uint32), got[3], got[4]]
    tag = "%dx%d %s weight_b %g tol %g flags %d%s" % (w, h, name, weight_b, tol, flags, " camera origin" if camera_origin else "")
    print("%s: holes %s (reference %d), source 1 / 2 / 3: %d / %d / %d, mask 2: %d, differing %s" % (
        tag, got_holes, want.holes, int(np.count_nonzero(want.source == 1)), int(np.count_nonzero(want.source == 2)),
        int(np.count_nonzero(want.source == 3)), int(np.count_nonzero(want.mask == 2)),
        [int(np.count_nonzero(g != e)) if k in outs else -1 for k, (g, e) in enumerate(zip(got_cmp, exp))]))
    for k, (g, e) in enumerate(zip(got_cmp, exp)):
        if k in outs:
            assert np.array_equal(g, e), (tag, Buffers.NAMES[k])
        else:
            assert np.all(b.out[k].numpy() == Buffers.CANARIES[k]), (tag, Buffers.NAMES[k])
    if holes:
        assert got_holes == want.holes, tag
    return got + [got_holes]


def _every_combination(r, sc, w, h, camera_origin):
    r.set_frame_size(w, h)
    for name in P.CASE_NAMES:
        a, b2, _, _ = P.case(sc, w, h, camera_origin, name)
        b = Buffers(r, w * h, a, b2)
        try:
            for flags, weight_b, tol in itertools.product((0, RR.FILL), WEIGHTS, TOLS):
                check(b, sc, w, h, name, weight_b, tol, flags, camera_origin)
        finally:
            b.free()


@pytest.mark.parametrize("w,h", RR.SIZES, ids=["%dx%d" % s for s in RR.SIZES])
def test_every_case_equals_the_definition(ctx, model, w, h):
    """the three consistent motions and the two independent frames, with the fill and without, weight_b 0 / 0.3 / 1, depth_tol 0 / 0.05"""
    _every_combination(ctx, model[1], w, h, False)


@pytest.mark.parametrize("w,h", RR.SIZES, ids=["%dx%d" % s for s in RR.SIZES])
def test_coarse_fine_depths_count_from_the_camera(ctx_cf, w, h):
    r, sc = ctx_cf
    _every_combination(r, sc, w, h, True)


def test_the_origin_matters_on_these_inputs(ctx_cf):
    """from the sphere exit the same two frames splat differently: the coarse/fine test above would notice the wrong origin"""
    r, sc = ctx_cf
    w, h = RR.SIZES[0]
    a, b, dp, dr = P.case(sc, w, h, True, "independent")
    cam, exit_ = P.pair_f32(sc, w, h, True, a, b, dp, dr), P.pair_f32(sc, w, h, False, a, b, dp, dr)
    assert not np.array_equal(cam.winner_a, exit_.winner_a)


def _single_warp(r, b, which, dst, flags, with_depth):
    """adanerf_reproject of source A (0) or B (1) of the Buffers b on any RGBA8 image: (depth or None, mask, holes)"""
    n = b.n
    rgba = R.DeviceArray(r, (n, 4), np.uint8).upload(np.full((n, 4), 7, np.uint8))
    out = R.DeviceArray(r, (n, 4), np.uint8)
    depth = R.DeviceArray(r, (n,), np.float32) if with_depth else None
    mask = R.DeviceArray(r, (n,), np.uint8)
    try:
        pos, rot = b.poses[which]
        holes = r.reproject_device(rgba, b.src[3 * which + 1], b.src[3 * which + 2], pos, rot, dst[0], dst[1], out, depth, mask, acc_min=RR.ACC_MIN,
                                   hole_rgba8=RR.HOLE, fill=bool(flags & RR.FILL))
        return (depth.numpy() if with_depth else None), mask.numpy(), holes
    finally:
        for x in (rgba, out, depth, mask):
            if x is not None:
                x.free()


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_against_the_single_source_stage_on_the_same_inputs(ctx, model, name):
    """adanerf_reproject of A and of B: without the fill a pixel is a hole of the pair iff it is a hole of both; with B the same
    frame as A the pair's depth and mask are adanerf_reproject's bit for bit, with the fill and without"""
    sc = model[1]
    w, h = RR.SIZES[0]
    ctx.set_frame_size(w, h)
    a, b2, dp, dr = P.case(sc, w, h, False, name)
    b = Buffers(ctx, w * h, a, b2)
    try:
        got = check(b, sc, w, h, name, 0.3, P.DEPTH_TOL, 0)
        _, mask_a, holes_a = _single_warp(ctx, b, 0, (dp, dr), 0, False)
        _, mask_b, holes_b = _single_warp(ctx, b, 1, (dp, dr), 0, False)
        assert np.array_equal(got[3] == 0, (mask_a == 0) & (mask_b == 0)) and got[5] <= min(holes_a, holes_b)
        print("%s: holes of A alone %d, of B alone %d, of the pair %d" % (name, holes_a, holes_b, got[5]))
        for flags in (0, RR.FILL):
            depth_1, mask_1, holes_1 = _single_warp(ctx, b, 0, (dp, dr), flags, True)
            b.reset()
            rc, holes = b.call((dp, dr), weight_b=0.3, flags=flags, src=(0, 1, 2, 0, 1, 2), b_pose=b.poses[0])
            assert rc == 0, ctx.lib.adanerf_last_error(ctx.handle).decode()
            rgb, rgba8, depth, mask, source = b.outputs()
            assert holes == holes_1 and np.array_equal(mask, mask_1) and np.array_equal(depth.view(np.uint32), depth_1.view(np.uint32))
            assert np.all(source[mask == 1] == 3) and np.all(np.isin(source[mask == 2], (1,))) and np.all(source[mask == 0] == 0)
    finally:
        b.free()


def test_every_optional_output_may_be_null(ctx, model):
    sc = model[1]
    w, h = 33, 9
    ctx.set_frame_size(w, h)
    a, b2, _, _ = P.case(sc, w, h, False, "independent")
    b = Buffers(ctx, w * h, a, b2)
    try:
        for given in itertools.product((False, True), repeat=5):      # rgba8, depth, mask, source, holes_out
            outs = (0,) + tuple(k + 1 for k in range(4) if given[k])
            check(b, sc, w, h, "independent", outs=outs, holes=given[4])
    finally:
        b.free()


def test_same_bits_on_every_call_and_across_frame_sizes(model):
    """a fresh context: the two z-buffers are made at 16 x 12, grown for 97 x 61, reused by 16 x 12, and hold nothing from call to call;
    adanerf_reproject in between uses the first of them"""
    z, sc, d = model
    big, small = RR.SIZES[0], RR.SIZES[1]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, small[0], small[1])) as r:
        seen = {}
        for (w, h) in (small, big, small, big):
            r.set_frame_size(w, h)
            a, b2, dp, dr = P.case(sc, w, h, False, "forward")
            b = Buffers(r, w * h, a, b2)
            try:
                first = check(b, sc, w, h, "forward")
                _single_warp(r, b, 1, (dp, dr), RR.FILL, True)
                again = check(b, sc, w, h, "forward")
            finally:
                b.free()
            for other in (again, seen.setdefault((w, h), first)):
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first[:5], other[:5])) and first[5] == other[5]


def test_refused_arguments(ctx, model, tmp_path_factory):
    r, sc = ctx, model[1]
    w, h = RR.SIZES[1]
    r.set_frame_size(w, h)
    n = w * h
    a, b2, dp, dr = P.case(sc, w, h, False, "independent")
    dst = (dp, dr)
    b = Buffers(r, n, a, b2)
    nan_pos, inf_rot = np.array(a.pos, np.float32), np.array(a.rot, np.float32)
    nan_pos[1], inf_rot[2, 0] = np.nan, np.inf
    o = [b.out[k].ptr + b.step[k] * PAD for k in range(5)]
    s = [x.ptr for x in b.src]
    try:
        cases = [dict(src=tuple(None if k == j else k for k in range(6))) for j in range(6)] + [dict(outs=(1, 2, 3, 4))]
        cases += [dict(null_pose=k) for k in range(6)]
        cases += [dict(a_pose=(nan_pos, a.rot)), dict(a_pose=(a.pos, inf_rot)), dict(b_pose=(nan_pos, b2.rot)), dict(b_pose=(b2.pos, inf_rot)),
                  dict(dst_pose=(nan_pos, dr)), dict(dst_pose=(dp, inf_rot)),
                  dict(weight_b=float("nan")), dict(weight_b=-0.01), dict(weight_b=1.5), dict(weight_b=float("inf")),
                  dict(acc_min=float("nan")), dict(acc_min=-0.25), dict(tol=float("nan")), dict(tol=-0.01), dict(flags=2), dict(flags=3), dict(flags=-1),
                  # misaligned fp32 and uchar4 pointers
                  dict(src_ptr={0: s[0] + 2}), dict(src_ptr={1: s[1] + 1}), dict(src_ptr={2: s[2] + 3}), dict(src_ptr={3: s[3] + 2}), dict(src_ptr={4: s[4] + 1}),
                  dict(src_ptr={5: s[5] + 3}), dict(out_ptr={0: o[0] + 2}), dict(out_ptr={1: o[1] + 1}), dict(out_ptr={2: o[2] + 2}),
                  # an output over a source image of A or of B: the same start, one shared element at either end
                  dict(out_ptr={0: s[0]}), dict(out_ptr={0: s[3] + 12 * (n - 1)}), dict(out_ptr={2: s[1]}), dict(out_ptr={2: s[5] + 4 * (n - 1)}),
                  dict(out_ptr={1: s[2] - 4 * (n - 1)}), dict(out_ptr={3: s[4] + 4 * n - 1}), dict(out_ptr={3: s[0]}), dict(out_ptr={4: s[3] + 8 * n}),
                  dict(out_ptr={4: s[1] + 4 * n - 1}),
                  # an output over another output
                  dict(out_ptr={1: o[0]}), dict(out_ptr={2: o[0] + 12 * n - 4}), dict(out_ptr={3: o[0] + 5}), dict(out_ptr={2: o[1]}), dict(out_ptr={3: o[1] + 4 * n - 1}),
                  dict(out_ptr={3: o[2]}), dict(out_ptr={1: o[3] - 4 * n + 4}), dict(out_ptr={4: o[3]}), dict(out_ptr={4: o[3] + n - 1}), dict(out_ptr={4: o[0] + 7})]
        for kw in cases:
            args = dict(dst_pose=dst)
            args.update(kw)
            rc, holes = b.call(args.pop("dst_pose"), **args)
            assert rc == EINVAL and holes == -7, kw
            assert "adanerf_reproject_pair" in r.lib.adanerf_last_error(r.handle).decode(), kw
            assert b.untouched(), kw
            b.sources_unmodified()
        assert b.call(dst, handle=False)[0] == EINVAL and b.untouched()
        # adjacent ranges do not overlap; acc_min 0, depth_tol 0 and both ends of weight_b's range are legal; A and B may be the same buffers
        big = R.DeviceArray(r, (5 * n + n // 2,), np.float32)
        try:
            rc, holes = b.call(dst, weight_b=0.0, acc_min=0.0, tol=0.0, out_ptr={0: big.ptr, 1: big.ptr + 12 * n, 2: big.ptr + 16 * n, 3: big.ptr + 20 * n, 4: big.ptr + 21 * n})
            assert rc == 0 and holes >= 0, r.lib.adanerf_last_error(r.handle).decode()
            rc, holes = b.call(dst, weight_b=1.0, flags=RR.FILL, src=(0, 1, 2, 0, 1, 2))
            assert rc == 0 and holes >= 0
            r.sync()
        finally:
            big.free()
    finally:
        b.free()
    # a useNDC model; a context that renders one of two shards
    z, sc_ndc, d_ndc = _model(tmp_path_factory, "ndc_synthetic_n8")
    a, b2, dp, dr = P.case(sc, w, 16, False, "independent")
    for d, kw, word in ((d_ndc, dict(), "NDC"), (model[2], dict(shard_world=2, shard_rank=0), "shard_world")):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, 16), **kw) as r2:
            b = Buffers(r2, w * 16, a, b2)
            try:
                rc, holes = b.call((dp, dr))
                assert rc == EUNSUPPORTED and holes == -7 and word in r2.lib.adanerf_last_error(r2.handle).decode()
                assert b.untouched()
            finally:
                b.free()


def test_masked_render_takes_the_pairs_mask_unchanged(ctx, model):
    """adanerf_render_masked(d_dst_mask, 1, ..) after a pair call renders exactly `holes` rays; values 5 the filled pixels too"""
    z, sc, d = model
    w, h = RR.SIZES[0]
    ctx.set_frame_size(w, h)
    a, b2, dp, dr = P.case(sc, w, h, False, "yaw")
    b = Buffers(ctx, w * h, a, b2)
    image = R.DeviceArray(ctx, (w * h, 4), np.uint8)
    try:
        for flags in (0, RR.FILL):
            got = check(b, sc, w, h, "yaw", flags=flags)
            mask_ptr = b.out[3].ptr + PAD
            ctx.set_camera(dp, dr)
            m, _ = ctx.render_masked(mask_ptr, 1, rgba8=image)
            assert m == got[5] == int(np.count_nonzero(got[3] == 0))
            m5, _ = ctx.render_masked(mask_ptr, 5, rgba8=image)
            assert m5 == int(np.count_nonzero(got[3] != 1))
        assert got[5] == 0 and m5 > 0      # with the fill nothing is left of this case's holes; they are the mask-2 pixels
    finally:
        image.free()
        b.free()


# ---- the hosts -------------------------------------------------------------------------------------

def test_python_host_interpolates_between_two_keyframes(model):
    """render_keyframe twice, interpolate at the first keyframe's pose with weight_b = 0: the image is that keyframe wherever the pixel
    comes from A (source 1) or from both (source 3: cA + 0 * (cB - cA)) and the keyframe's colour is finite.  Then the definition on
    the host's own buffers, pair_weight as the default, interpolate_rerender and the frame-size rule."""
    z, sc, d = model
    w, h = 48, 32
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        with pytest.raises(R.AdaNeRFError):
            r.render_keyframe()                                        # not enabled
        r.enable_interpolation()
        pose_a = np.asarray(z["pose"], np.float32)
        pose_b = (pose_a + np.float32(0.1) * np.asarray(sc.view_cell_size, np.float32)).astype(np.float32)
        r.set_camera(pose_a, z["rot"])
        key_a, key_a8, st = r.render_keyframe()
        assert st.total_samples > 0 and len(np.unique(key_a8[:, :3])) > 16
        with pytest.raises(R.AdaNeRFError):
            r.interpolate(pose_a, z["rot"])                            # one keyframe only
        r.set_camera(pose_b, z["rot"])
        key_b, _, _ = r.render_keyframe()
        r.set_camera(pose_a, z["rot"])
        _, plain8, _ = r.render_numpy()
        assert np.array_equal(plain8, key_a8)                          # a keyframe is the frame render_numpy renders
        rgb, rgba8, mask, source, holes = r.interpolate(pose_a, z["rot"], weight_b=0.0)
        from_a = np.isin(source, (1, 3))[:, None] & np.isfinite(key_a)
        assert np.count_nonzero(from_a) > w * h and np.array_equal(rgb[from_a].view(np.uint32), key_a[from_a].view(np.uint32))
        assert holes == int(np.count_nonzero(mask == 0)) and np.count_nonzero(source == 3) > 0
        # the pose between: the default weight is pair_weight's, the result the definition's on the keyframes the host kept
        mid = (pose_a + np.float32(0.3) * (pose_b - pose_a)).astype(np.float32)
        (ka, pa, ra), (kb, pb, rb) = r._ip_keys
        sa = P.Source(key_a, r._ip_set(ka)[1].numpy(), r._ip_set(ka)[2].numpy(), pa, ra)
        sb = P.Source(key_b, r._ip_set(kb)[1].numpy(), r._ip_set(kb)[2].numpy(), pb, rb)
        assert np.array_equal(r._ip_set(ka)[0].numpy().view(np.uint32), key_a.view(np.uint32))
        wb = R.pair_weight(mid, pose_a, pose_b)
        assert abs(wb - 0.3) < 1e-5
        rgb, rgba8, mask, source, holes = r.interpolate(mid, z["rot"])
        want = P.pair_f32(sc, w, h, False, sa, sb, mid, z["rot"], weight_b=wb, acc_min=0.5, depth_tol=0.05, hole_rgba8=0xFF000000, flags=RR.FILL)
        assert np.array_equal(rgb.view(np.uint32), want.rgb.view(np.uint32)) and np.array_equal(rgba8, want.rgba8)
        assert np.array_equal(mask, want.mask) and np.array_equal(source, want.source) and holes == want.holes
        bare = r.interpolate(mid, z["rot"], fill=False)
        rr = r.interpolate_rerender(mid, z["rot"], "holes", fill=False)
        assert rr[5] == rr[4] == bare[4] and np.array_equal(rr[2], bare[2])
        r.set_camera(mid, z["rot"])
        _, fresh, _ = r.render_numpy()
        assert np.array_equal(rr[1][bare[2] != 0], bare[1][bare[2] != 0]) and np.array_equal(rr[1][bare[2] == 0], fresh[bare[2] == 0])
        print("48 x 32, a tenth of the view cell between the keyframes: holes without the fill %d, blended pixels %d of %d" % (
            bare[4], int(np.count_nonzero(bare[3] == 3)), w * h))
        # a frame size change drops both keyframes
        r.set_frame_size(24, 16)
        with pytest.raises(R.AdaNeRFError):
            r.interpolate(mid, z["rot"])


def _bmp(path):
    bmp = open(path, "rb").read()
    return bmp[int.from_bytes(bmp[10:14], "little"):]


def test_cli_interpolate(model, tmp_path):
    """--interpolate 3 --frames 8 -w over a script that holds the camera still writes the out.bmp a plain run writes: a still camera
    means identity warps of two identical keyframes"""
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    script = tmp_path / "still.txt"
    script.write_text("# still\n" * 8)      # a script sets the number of frames: one line each
    base = [exe, d, "-s", "64", "48", "-w", "--script", str(script), "--log-camera", "--frames", "8"]
    images = []
    try:
        for extra in ([], ["--interpolate", "3"], ["--interpolate", "3", "--rerender", "holes"]):
            if os.path.exists(os.path.join(d, "out.bmp")):
                os.remove(os.path.join(d, "out.bmp"))
            out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            images.append(_bmp(os.path.join(d, "out.bmp")))
            if extra:
                assert "interpolated 7 holes 0" in out.stdout, out.stdout      # frame 7 = 2 * 3 + 1: between the keyframes of calls 3 and 6
        assert len(np.unique(np.frombuffer(images[0], np.uint8))) > 16
        assert images[1] == images[0] and images[2] == images[0]
    finally:
        if os.path.exists(os.path.join(d, "out.bmp")):
            os.remove(os.path.join(d, "out.bmp"))


def test_evaluator_interpolate_stride(tmp_path):
    """evaluate(..., interpolate_stride=2) on the synthetic 12 x 10 dataset of test_evaluator_reproject_stride: poses 0 and 2 are the
    plain run's frames, pose 1 is NeuralRenderer.interpolate between them, scored from the fp32 result"""
    from adanerf_amd.evaluate import evaluate, main, psnr_from_mse
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
    summary, recs = evaluate(md, str(ds), "test", str(tmp_path / "pred"), precision="bf16", quiet=True, metrics=("psnr", "flip"), interpolate_stride=2)
    plain, precs = evaluate(md, str(ds), "test", str(tmp_path / "plain"), precision="bf16", quiet=True, metrics=("psnr", "flip"))
    assert sorted(plain) == ["frames", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    assert sorted(summary) == sorted(list(plain) + ["mean_psnr_rendered", "mean_psnr_interpolated", "mean_flip_rendered", "mean_flip_interpolated",
                                                    "mean_hole_fraction", "mean_blended_fraction"])
    assert [x.get("interpolated", False) for x in recs] == [False, True, False] and not any("warped" in x for x in recs)
    for i in (0, 2):
        assert np.array_equal(read_png(str(tmp_path / "pred" / ("%05d.png" % i))), read_png(str(tmp_path / "plain" / ("%05d.png" % i))))
        assert recs[i]["psnr"] == precs[i]["psnr"] and recs[i]["flip"] == precs[i]["flip"] and recs[i]["samples_per_ray"] == precs[i]["samples_per_ray"]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w, h)) as r:
        r.enable_interpolation()
        for k in (0, 2):
            r.set_camera(*poses[k])
            r.render_keyframe()
        rgb, rgba8, mask, source, holes = r.interpolate(*poses[1])
    assert np.array_equal(read_png(str(tmp_path / "pred" / "00001.png")), rgba8[:, :3].reshape(h, w, 3))
    ref = gts[1].astype(np.float32).reshape(-1, 3) / 255.0
    mse = float(np.mean((rgb.astype(np.float64) - ref) ** 2))
    assert recs[1]["mse"] == mse and recs[1]["psnr"] == psnr_from_mse(mse)
    assert recs[1]["hole_fraction"] == holes / float(w * h) and recs[1]["blended_fraction"] == np.count_nonzero(source == 3) / float(w * h)
    assert "samples_per_ray" not in recs[1] and 0.0 <= recs[1]["flip"] <= 1.0
    assert summary["mean_psnr_interpolated"] == recs[1]["psnr"] and summary["mean_hole_fraction"] == recs[1]["hole_fraction"]
    assert summary["mean_blended_fraction"] == recs[1]["blended_fraction"]
    assert summary["mean_psnr_rendered"] == float(np.mean([recs[0]["psnr"], recs[2]["psnr"]]))
    assert summary["mean_samples_per_ray"] == float(np.mean([precs[0]["samples_per_ray"], precs[2]["samples_per_ray"]]))
    with_rr, rrecs = evaluate(md, str(ds), "test", str(tmp_path / "rr"), precision="bf16", quiet=True, interpolate_stride=2, rerender="holes")
    assert sorted(with_rr) == sorted(["frames", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray", "mean_psnr_rendered", "mean_psnr_interpolated",
                                      "mean_hole_fraction", "mean_blended_fraction", "mean_psnr_interpolated_rerendered", "mean_rerendered_fraction"])
    assert rrecs[1]["rerendered_fraction"] == rrecs[1]["hole_fraction"]
    main([md, str(ds), "--interpolate-stride", "2"])      # and the command line
