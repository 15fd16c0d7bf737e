"""Foveated density over time on the GPU: the phased mask equals the host mask at all 64 phases; the phased fill and
adanerf_temporal_resolve_sparse equal tests/sparse_temporal_reference.py (the definitions of include/adanerf_hip.h in numpy float32) bit
for bit in every output, with no pixel excluded; canaries sit before and after every output and the sources are checked unmodified.  The
fill keeps tests/test_gpu_density.py's one allowance (where the reference itself computes a NaN any NaN agrees).  End to end,
render_foveated_temporal at rest converges on the full render and on a lateral path equals the reference chain.  Run with `pytest -m gpu`
on an MI355X box."""
import ctypes as C

import numpy as np
import pytest

import adanerf_oracle as O
import density_reference as DR
import reproject_reference as RR
import sparse_temporal_reference as SR
from conftest import case_weights, load_case, record
from test_gpu_density import IMAGES, MASK_CANARY, SETTINGS, Canaried, caller_mask, differing, setting, synthetic

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
PAD = 64
CANARY_F32 = np.float32(-1234.5)
MASK_SIZES = [(48, 40), (37, 29)]
FILL_PHASES = [(0, 0), (3, 5), (7, 7), (1, 0)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    z, meta, sc = load_case("classroom_n8_thr02")
    d = str(tmp_path_factory.mktemp("sparse_classroom_n8_thr02"))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, sc, d


@pytest.fixture(scope="module")
def ctx(model):
    """one small context; the tests move its frame size"""
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 12)) as r:
        r.set_camera(z["pose"], z["rot"])
        yield r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the phased mask ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", MASK_SIZES, ids=["%dx%d" % s for s in MASK_SIZES])
@pytest.mark.parametrize("skew", [0, 3], ids=["aligned", "misaligned"])
def test_device_mask_equals_the_host_mask_at_every_phase(ctx, w, h, skew):
    ctx.set_frame_size(w, h)
    m = Canaried(ctx, w * h, 1, np.uint8, MASK_CANARY, skew)
    try:
        for k in range(len(SETTINGS)):
            gaze, radius, stride, rings = setting(w, h, k)
            for f in range(64):
                phase = SR.phase_of(f)
                m.set(np.full((w * h, 1), MASK_CANARY, np.uint8))
                assert ctx.foveate_density_phased_device(gaze, rings, phase, m.ptr) == 0, ctx.lib.adanerf_last_error(ctx.handle).decode()
                ctx.sync()
                got = m.get("mask").reshape(-1)
                want = R.density_mask_phased(w, h, gaze, rings, phase)
                assert np.array_equal(got, want), (SETTINGS[k], phase, np.flatnonzero(got != want)[:8])
                if f % 9 == 0:      # the host mask against the brute-force rule: all 64 phases on the CPU side, a sample here
                    assert np.array_equal(want, SR.mask_phased(w, h, gaze, radius, stride, phase)), (SETTINGS[k], phase)
            m.set(np.full((w * h, 1), MASK_CANARY, np.uint8))      # phase (0, 0) is the unphased call
            assert ctx.foveate_density_device(gaze, rings, m.ptr) == 0
            ctx.sync()
            assert np.array_equal(m.get("mask").reshape(-1), R.density_mask_phased(w, h, gaze, rings, (0, 0)))
    finally:
        m.free()


# ---- the phased fill ----------------------------------------------------------------------------------------------

def check_fill(r, w, h, mask, phase, seed, use=(True, True, True), count=True, tag="", unphased=False):
    """one adanerf_fill_density_phased over canaried synthetic images against the reference; use: depth, acc, rgba8 given (else NULL);
    unphased: call adanerf_fill_density instead (phase must be (0, 0))"""
    n = w * h
    src = synthetic(w, h, mask, seed)
    d_mask = Canaried(r, n, 1, np.uint8, MASK_CANARY)
    d_mask.set(mask)
    bufs = [Canaried(r, n, k, dt, canary) for _, k, dt, canary in IMAGES]
    try:
        for b, a in zip(bufs, src):
            b.set(a)
        on = [True] + list(use)
        ptrs = [b.ptr if o else None for b, o in zip(bufs, on)]
        if unphased:
            rc, unfilled = r.fill_density_device(d_mask.ptr, w, h, *ptrs, count=count)
        else:
            rc, unfilled = r.fill_density_phased_device(d_mask.ptr, w, h, phase, *ptrs, count=count)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        r.sync()
        want = SR.fill_phased(mask, w, h, phase, src[0], src[1] if use[0] else None, src[2] if use[1] else None, src[3] if use[2] else None)
        one = np.zeros(n, bool)      # a value that is copied, not computed, is compared by its bits
        for p in np.flatnonzero(np.isin(mask, (2, 4, 8))).tolist():
            c = SR.used_corners(p % w, p // w, int(mask[p]), w, h, phase)
            one[p] = len(c) == 1 and mask[c[0]] == 0
        got_all = []
        for b, a, wnt, o, (name, _, _, _) in zip(bufs, src, want[:4], on, IMAGES):
            got = b.get(name)
            got_all.append(got)
            exp = wnt.reshape(got.shape) if o else a.reshape(got.shape)      # an image that was not passed keeps every byte
            diff = differing(got, exp)
            print("%s %s: %d of %d pixels differ (unfilled %s, reference %d)" % (tag, name, int(diff.sum()), n, unfilled, want[4]))
            assert not diff.any(), (tag, name, np.flatnonzero(diff)[:8])
            assert np.array_equal(got[one].view(np.uint8), exp[one].view(np.uint8)), (tag, name, "a copied value changed its bits")
            keep = ~np.isin(mask, (2, 4, 8))
            assert np.array_equal(got[keep].view(np.uint8), a.reshape(got.shape)[keep].view(np.uint8)), (tag, name, "a pixel of byte 0 or a foreign byte changed")
        assert np.array_equal(d_mask.get("mask").reshape(-1), mask), "mask modified"
        if count:
            assert unfilled == want[4], tag
        return unfilled, got_all
    finally:
        d_mask.free()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("w,h", MASK_SIZES + [(5, 3)], ids=["48x40", "37x29", "5x3"])
def test_phased_fill_equals_the_reference(ctx, w, h):
    """device masks (every corner rendered: nothing unfilled but the pixels of a frame narrower than the stride) and caller masks with
    unrendered corners, at phases (0, 0), (3, 5), (7, 7), (1, 0); phase (0, 0) writes adanerf_fill_density's bytes"""
    ctx.set_frame_size(*MASK_SIZES[0])      # the fill takes its size as arguments: the context's own is another
    lost = 0
    kinds = set()
    for phase in FILL_PHASES:
        for k in (1, 2, 3):      # strides up to 8 with three rings; the gaze outside; every pixel of stride 8
            gaze, radius, stride, rings = setting(w, h, k)
            mask = R.density_mask_phased(w, h, gaze, rings, phase)
            tag = "%dx%d %s phase %s" % (w, h, SETTINGS[k][1], phase)
            unfilled, got = check_fill(ctx, w, h, mask, phase, seed=100 + k, tag=tag)
            none = sum(1 for p in np.flatnonzero(mask).tolist() if not SR.used_corners(p % w, p // w, int(mask[p]), w, h, phase))
            assert unfilled == none and (none == 0 or (w, h) == (5, 3))
            lost += none
            kinds |= {len(SR.used_corners(p % w, p // w, int(mask[p]), w, h, phase)) for p in np.flatnonzero(mask).tolist()}
            if phase == (0, 0):
                plain = check_fill(ctx, w, h, mask, phase, seed=100 + k, tag=tag + " unphased", unphased=True)[1]
                assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, plain))
        if (w, h) != (5, 3):
            damaged = caller_mask(w, h, 1, seed=7)
            lost += check_fill(ctx, w, h, damaged, phase, seed=200, tag="%dx%d caller phase %s" % (w, h, phase))[0]
    assert lost > 0
    assert kinds >= ({0, 1, 2} if (w, h) == (5, 3) else {1, 2, 4})


@pytest.mark.parametrize("use", [(False, False, False), (True, False, False), (False, True, False), (False, False, True)],
                         ids=["rgb only", "depth", "acc", "rgba8"])
def test_phased_fill_optional_images(ctx, use):
    w, h = MASK_SIZES[1]
    gaze, radius, stride, rings = setting(w, h, 1)
    check_fill(ctx, w, h, R.density_mask_phased(w, h, gaze, rings, (3, 5)), (3, 5), seed=400, use=use, tag="optional %s" % (use,))
    check_fill(ctx, w, h, caller_mask(w, h, 1, 9), (7, 7), seed=401, use=use, count=False, tag="optional, no counter %s" % (use,))


# ---- the sparse resolve -------------------------------------------------------------------------------------------

_HIST, _FRAME, _WANT = {}, {}, {}


def history(sc, w, h, camera_origin=False):
    if (w, h, camera_origin) not in _HIST:
        hr, hd, hc, pose = SR.history_at(sc, w, h, camera_origin)
        for a in (hr, hd, hc):
            a.setflags(write=False)
        _HIST[(w, h, camera_origin)] = (hr, hd, hc, pose)
    return _HIST[(w, h, camera_origin)]


def frame(sc, w, h, phase):
    """(mask, rgb, depth, acc) of the phase: computed once, shared, never changed"""
    if (w, h, phase) not in _FRAME:
        mask = SR.resolve_mask(w, h, phase)
        arrays = (mask,) + tuple(np.ascontiguousarray(a) for a in SR.current_at(sc, w, h, mask, phase))
        for a in arrays:
            a.setflags(write=False)
        _FRAME[(w, h, phase)] = arrays
    return _FRAME[(w, h, phase)]


def reference(sc, w, h, motion, phase, with_depth, clamp, with_hist=True, tol=SR.TEST_TOL, camera_origin=False):
    key = (w, h, motion, phase, with_depth, clamp, with_hist, tol, camera_origin)
    if key not in _WANT:
        hr, hd, hc, (pp, pr) = history(sc, w, h, camera_origin)
        mask, cr, cd, ca = frame(sc, w, h, phase)
        dst = RR.moved(sc, **RR.MOTIONS[motion])
        _WANT[key] = SR.sparse_f32(sc, w, h, camera_origin, mask, phase, cr, cd, ca, dst[0], dst[1], hr if with_hist else None, hd if with_depth else None,
                                   hc if with_hist else None, pp, pr, depth_tol=tol, flags=SR.CLAMP if clamp else 0)
    return _WANT[key]


def _f(v, n):
    if v is None:
        return None, None
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(n)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


class Buffers:
    """the device side of one frame size: the seven sources (mask, current rgb / depth / acc, history rgb / depth / count), five canaried outputs"""
    CANARIES = (CANARY_F32, CANARY_F32, 0xA5, 0xA5, 0xA5)
    NAMES = ("rgb", "depth", "count", "rgba8", "mask")
    SOURCES = ("mask", "cur_rgb", "cur_depth_map", "cur_acc_map", "hist_rgb", "hist_depth", "hist_count")

    def __init__(self, r, sc, w, h, camera_origin=False):
        self.r, self.sc, self.w, self.h, self.n, self.camera_origin = r, sc, w, h, w * h, camera_origin
        n = self.n
        shapes = [((n,), np.uint8), ((n, 3), np.float32), ((n,), np.float32), ((n,), np.float32), ((n, 3), np.float32), ((n,), np.float32), ((n,), np.uint8)]
        self.src = [R.DeviceArray(r, s, t) for s, t in shapes]
        self.host = [None] * 7
        hr, hd, hc, self.prev = history(sc, w, h, camera_origin)
        for k, a in zip((4, 5, 6), (hr, hd, hc)):
            self.host[k] = np.ascontiguousarray(a)
            self.src[k].upload(self.host[k])
        t = PAD + n + PAD
        self.out = [R.DeviceArray(r, (t, 3), np.float32), R.DeviceArray(r, (t,), np.float32), R.DeviceArray(r, (t,), np.uint8),
                    R.DeviceArray(r, (t, 4), np.uint8), R.DeviceArray(r, (t,), np.uint8)]
        self.step = [12, 4, 1, 4, 1]      # bytes per element
        self.reset()

    def load(self, phase):
        for k, a in enumerate(frame(self.sc, self.w, self.h, phase)):
            self.host[k] = a
            self.src[k].upload(a)

    def reset(self):
        for b, c in zip(self.out, self.CANARIES):
            b.upload(np.full(b.shape, c, b.dtype))

    def call(self, phase, cur_pose, prev_pose, alpha=SR.ALPHA, tol=SR.TEST_TOL, acc_min=SR.ACC_MIN, flags=SR.CLAMP, src=(0, 1, 2, 3, 4, 5, 6),
             outs=(0, 1, 2, 3, 4), rejected=True, handle=True, ptrs=None):
        """the C ABI itself; returns (rc, rejected or None).  ptrs: {argument name: pointer} replacing what src / outs give"""
        keep = [_f(cur_pose[0], 3), _f(cur_pose[1], 9), _f(prev_pose[0], 3), _f(prev_pose[1], 9)]
        n_rej = C.c_int32(-7)
        s = [self.src[k].ptr if k is not None else None for k in src]
        o = [self.out[k].ptr + self.step[k] * PAD if k in outs else None for k in range(5)]
        a = dict(mask=s[0], cur_rgb=s[1], cur_depth=s[2], cur_acc=s[3], hist_rgb=s[4], hist_depth=s[5], hist_count=s[6], out_rgb=o[0], out_depth=o[1],
                 out_count=o[2], out_rgba8=o[3], out_mask=o[4])
        a.update(ptrs or {})
        rc = self.r.lib.adanerf_temporal_resolve_sparse(self.r.handle if handle else None, a["mask"], int(phase[0]), int(phase[1]), a["cur_rgb"], a["cur_depth"],
                                                        a["cur_acc"], keep[0][1], keep[1][1], a["hist_rgb"], a["hist_depth"], a["hist_count"], keep[2][1],
                                                        keep[3][1], float(alpha), float(tol), float(acc_min), int(flags), a["out_rgb"], a["out_depth"],
                                                        a["out_count"], a["out_rgba8"], a["out_mask"], C.byref(n_rej) if rejected else None)
        return rc, (n_rej.value if rejected else None)

    def outputs(self):
        """(rgb, depth, count, rgba8, mask) after a sync, canaries and sources checked"""
        self.r.sync()
        n = self.n
        got = [b.numpy() for b in self.out]
        for g, canary, what in zip(got, self.CANARIES, self.NAMES):
            assert np.all(g[:PAD] == canary) and np.all(g[PAD + n:] == canary), "wrote outside the %s output" % what
        for d, hst, what in zip(self.src, self.host, self.SOURCES):
            assert np.array_equal(d.numpy().view(np.uint8).reshape(-1), hst.view(np.uint8).reshape(-1)), "source %s modified" % what
        return [g[PAD:PAD + n] for g in got]

    def untouched(self):
        self.r.sync()
        return all(np.all(b.numpy() == c) for b, c in zip(self.out, self.CANARIES))

    def free(self):
        for b in self.src + self.out:
            b.free()


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


def check(b, motion, phase, with_depth=True, clamp=True, with_hist=True, tol=SR.TEST_TOL, outs=(0, 1, 2, 3, 4), rejected=True):
    want = reference(b.sc, b.w, b.h, motion, phase, with_depth, clamp, with_hist, tol, b.camera_origin)
    dst = RR.moved(b.sc, **RR.MOTIONS[motion])
    b.load(phase)
    b.reset()
    src = (0, 1, 2, 3, 4 if with_hist else None, 5 if with_hist and with_depth else None, 6 if with_hist else None)
    rc, got_rejected = b.call(phase, dst, b.prev if with_hist else (None, None), tol=tol, flags=SR.CLAMP if clamp else 0, src=src, outs=outs, rejected=rejected)
    assert rc == 0, b.r.lib.adanerf_last_error(b.r.handle).decode()
    got = b.outputs()
    compare(got, got_rejected, want, "%dx%d %s phase %s depth %d clamp %d hist %d tol %g" % (b.w, b.h, motion, phase, with_depth, clamp, with_hist, tol), outs, rejected)
    return got, got_rejected, want


@pytest.fixture(scope="module")
def sized(ctx, model):
    """device buffers per frame size, made on first use"""
    made = {}

    def get(w, h):
        ctx.set_frame_size(w, h)
        if (w, h) not in made:
            made[(w, h)] = Buffers(ctx, model[1], w, h)
        return made[(w, h)]
    yield get
    for b in made.values():
        b.free()


@pytest.mark.parametrize("w,h", SR.SIZES, ids=["%dx%d" % s for s in SR.SIZES])
def test_every_motion_equals_the_definition(sized, w, h):
    """every motion x (history depth, clamp) on and off, the phases taken in turn; without a history every pixel is rejected"""
    b = sized(w, h)
    for motion, phase, with_depth, clamp in SR.geometric_cases():
        got, rej, want = check(b, motion, phase, with_depth, clamp)
        if motion == "sees_none":
            assert rej == w * h and np.all(got[4] == 0)
    for clamp in (True, False):
        got, rej, want = check(b, "lateral", (3, 5), with_depth=False, clamp=clamp, with_hist=False)
        assert rej == w * h and np.all(got[4] == 0) and np.array_equal(got[2], (b.host[0] == 0).astype(np.uint8))
        assert np.array_equal(bits(got[0]), bits(b.host[1]))


def test_what_the_inputs_hold(sized):
    """so that the equality above says something: far pixels, NaNs and both zeros in colour and depth; history counts 0, 1, 254 and 255;
    mask bytes 0, 2, 4, 8 and one outside; all three verdicts; reconstructed pixels with one, two and four corners; and a cell whose
    corners straddle a depth step, so that the history's depth lies inside the corners' range and outside the range of the pixel's 3 x 3"""
    w, h = 48, 40
    b = sized(w, h)
    phase = (3, 5)
    got, rej, want = check(b, "identity", phase, tol=SR.DEPTH_TOL)
    mask, cr, cd, ca, hr, hd, hc = b.host
    assert np.isnan(cr).any() and np.isnan(hr).any() and (cr < 0).any() and (cr > 1).any()
    for img in (cr, hr):
        z = bits(img)
        assert (z == 0x80000000).any() and (z == 0).any()
    assert np.isnan(cd).any() and np.isinf(cd).any() and (cd < 0).any() and np.isnan(ca).any() and (ca == 0).any() and ((ca > 0) & (ca < SR.ACC_MIN)).any()
    assert np.isinf(got[1]).any() and np.isinf(hd).any() and np.isfinite(got[1]).any() and (bits(cd) == 0x80000000).any() and (bits(cd) == 0).any()
    for v in (0, 1, 254, 255):
        assert (hc == v).any()
    assert set(np.unique(mask).tolist()) == {0, 2, 4, 8, SR.FOREIGN}
    assert set(np.unique(got[4]).tolist()) == {0, 1, 2} and (got[2] == 255).any() and (got[2] == 0).any()
    rebuilt = np.isin(mask, (2, 4, 8))
    corners = {p: SR.used_corners(p % w, p // w, int(mask[p]), w, h, phase) for p in np.flatnonzero(rebuilt).tolist()}
    assert {len(c) for c in corners.values()} >= {1, 2, 4}
    live, tapped = got[4] == 1, hc[np.maximum(want.tap, 0)]
    assert (live & rebuilt).any() and (live & (mask == 0)).any() and (got[4] == 2).any()
    assert np.array_equal(got[2][live & rebuilt], tapped[live & rebuilt]) and np.all(tapped[got[4] == 2] == 0)
    assert np.array_equal(got[2][live & (mask == 0)], np.minimum(tapped[live & (mask == 0)].astype(int) + 1, 255).astype(np.uint8))
    # the straddling cell: accepted on its corners' range where the neighbourhood's range would have rejected it
    nb = SR.UR._neighbourhood(want.zp, w, h, np.float32(np.nan))
    fin = np.isfinite(nb)
    lo3, hi3 = np.min(np.where(fin, nb, np.inf), axis=0), np.max(np.where(fin, nb, -np.inf), axis=0)
    tol = SR.DEPTH_TOL
    straddle = rebuilt & want.accepted & np.isfinite(want.hd) & ((want.hd > hi3 * (1 + 2 * tol)) | (want.hd < lo3 * (1 - 2 * tol))) & (lo3 <= hi3)
    print("48x40 identity phase %s: %d reconstructed pixels accepted on their corners' range whose 3 x 3 range excludes the history's depth" % (
        phase, int(straddle.sum())))
    assert straddle.any()
    j = int(np.flatnonzero(straddle)[0])
    assert want.zlo[j] < want.zhi[j] and len(corners[j]) >= 2


def test_coarse_fine_depths_count_from_the_camera(tmp_path_factory):
    """a coarse / fine context: the depths count from the camera position, in pass A and in pass B"""
    z, meta, sc = load_case("classroom_coarse_fine_16_24")
    d = str(tmp_path_factory.mktemp("sparse_classroom_coarse_fine_16_24"))
    O.write_model_dir(d, sc, case_weights(meta))
    w, h = 37, 29
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        assert r.info.sampler_mode == R.SAMPLER_COARSE_FINE
        b = Buffers(r, sc, w, h, camera_origin=True)
        try:
            for motion, phase in (("lateral", (3, 5)), ("forward", (6, 1)), ("identity", (0, 7))):
                got, rej, want = check(b, motion, phase)
            other = reference(sc, w, h, "identity", (0, 7), True, True)      # the same call with the depths counted from the sphere exit
            assert not np.array_equal(bits(want.depth), bits(other.depth))
        finally:
            b.free()


def test_optional_outputs_and_the_counter_may_be_null(sized):
    b = sized(37, 29)
    check(b, "lateral", (3, 5), outs=(0, 2))
    check(b, "lateral", (3, 5), outs=(0, 1, 2), rejected=False)
    check(b, "forward", (7, 7), outs=(0, 2, 3))
    check(b, "backward", (1, 0), outs=(0, 2, 4), rejected=False)


def test_same_bits_on_every_call_and_across_frame_sizes(sized):
    first = [a.copy() for a in check(sized(48, 40), "yaw20", (6, 5))[0]]
    again = check(sized(48, 40), "yaw20", (6, 5))[0]
    assert all(np.array_equal(a.view(np.uint8), c.view(np.uint8)) for a, c in zip(first, again))
    check(sized(1, 1), "lateral", (2, 2))      # the zp scratch shrinks in use and grows back
    check(sized(64, 1), "lateral", (2, 2))
    back = check(sized(48, 40), "yaw20", (6, 5))[0]
    assert all(np.array_equal(a.view(np.uint8), c.view(np.uint8)) for a, c in zip(first, back))


def test_refused_arguments_write_nothing(ctx, sized, model, tmp_path_factory):
    w, h = 37, 29
    b = sized(w, h)
    phase = (3, 5)
    b.load(phase)
    dst = RR.moved(model[1], **RR.MOTIONS["lateral"])
    nan = np.float32(np.nan)

    def refused(code=EINVAL, word="adanerf_temporal_resolve_sparse", **kw):
        b.reset()
        args = dict(phase=phase, cur_pose=dst, prev_pose=b.prev)
        args.update(kw)
        rc, rej = b.call(**args)
        assert rc == code and (rej is None or rej == -7) and b.untouched(), kw
        if kw.get("handle", True):
            assert word in ctx.lib.adanerf_last_error(ctx.handle).decode(), kw
    assert b.call(phase, dst, b.prev)[0] == 0      # the arguments below differ from a call that is accepted in one thing each
    refused(handle=False)
    refused(src=(None, 1, 2, 3, 4, 5, 6), word="NULL mask")
    for k in (1, 2, 3):
        refused(src=tuple(None if i == k else i for i in range(7)), word="NULL image")
    refused(outs=(1, 2, 3, 4), word="NULL image")
    refused(outs=(0, 1, 3, 4), word="NULL d_out_count")
    refused(src=(0, 1, 2, 3, 4, 5, None), word="a history needs its count")
    for phase_bad in ((-1, 0), (0, 8), (8, 8), (3, -5)):
        refused(phase=phase_bad, word="phase_x and phase_y must be in 0..7")
    refused(cur_pose=(None, dst[1]), word="NULL pose")
    refused(prev_pose=(b.prev[0], None), word="NULL pose")
    refused(cur_pose=(np.array([nan, 0, 0], np.float32), dst[1]), word="not finite")
    refused(prev_pose=(b.prev[0], np.full(9, np.inf, np.float32)), word="not finite")
    for alpha in (0.0, -0.1, 1.5, nan):
        refused(alpha=alpha, word="alpha")
    refused(tol=-1.0, word="depth_tol")
    refused(tol=nan, word="depth_tol")
    refused(acc_min=-0.5, word="acc_min")
    refused(flags=2, word="flags")
    o = [x.ptr + st * PAD for x, st in zip(b.out, b.step)]
    refused(ptrs=dict(cur_rgb=b.src[1].ptr + 2), word="4-byte aligned")
    refused(ptrs=dict(out_depth=o[1] + 1), word="4-byte aligned")
    refused(ptrs=dict(out_rgb=b.src[4].ptr), word="overlaps")      # the history's colour
    refused(ptrs=dict(out_rgb=b.src[1].ptr), word="overlaps")      # the current colour
    refused(ptrs=dict(out_depth=b.src[5].ptr), word="overlaps")
    refused(ptrs=dict(out_count=b.src[6].ptr), word="overlaps")
    refused(ptrs=dict(out_count=b.src[0].ptr), word="the mask overlaps an output")
    refused(ptrs=dict(out_mask=b.src[0].ptr + 5), word="the mask overlaps an output")
    refused(ptrs=dict(mask=o[0] + 8), word="the mask overlaps an output")
    refused(ptrs=dict(mask=o[3] + 4 * w * h - 1), word="the mask overlaps an output")
    # a history's depth and count alone are no history; the previous pose is then not read
    b.reset()
    rc, rej = b.call(phase, dst, (None, None), src=(0, 1, 2, 3, None, 5, 6))
    assert rc == 0 and rej == w * h
    # a useNDC model; a context that renders one of two shards
    z, meta, sc_ndc = load_case("ndc_synthetic_n8")
    d_ndc = str(tmp_path_factory.mktemp("sparse_ndc_synthetic_n8"))
    O.write_model_dir(d_ndc, sc_ndc, case_weights(meta))
    for d, kw, word in ((d_ndc, dict(), "NDC"), (model[2], dict(shard_world=2, shard_rank=0), "shard_world")):
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), **kw) as r2:
            b2 = Buffers(r2, model[1], w, h)
            try:
                b2.load(phase)
                rc, rej = b2.call(phase, dst, b2.prev)
                assert rc == EUNSUPPORTED and rej == -7 and word in r2.lib.adanerf_last_error(r2.handle).decode()
                assert b2.untouched()
                if kw:
                    assert r2.foveate_density_phased_device((4.0, 4.0), [(2, 1), (2,)], (1, 1), b2.out[4]) == EUNSUPPORTED and b2.untouched()
            finally:
                b2.free()


def test_phased_density_refusals_write_nothing(ctx):
    w, h = MASK_SIZES[1]
    ctx.set_frame_size(w, h)
    gaze, radius, stride, rings = setting(w, h, 1)
    m = Canaried(ctx, w * h, 1, np.uint8, MASK_CANARY)
    img = Canaried(ctx, w * h, 3, np.float32, CANARY_F32)
    try:
        for phase in ((-1, 0), (0, -1), (8, 0), (0, 8), (100, 100)):
            assert ctx.foveate_density_phased_device(gaze, rings, phase, m.ptr) == EINVAL
            assert "adanerf_foveate_density_phased" in ctx.lib.adanerf_last_error(ctx.handle).decode()
            rc, unfilled = ctx.fill_density_phased_device(m.ptr, w, h, phase, img.ptr)
            assert rc == EINVAL and unfilled == -1 and "adanerf_fill_density_phased" in ctx.lib.adanerf_last_error(ctx.handle).decode()
        assert ctx.foveate_density_phased_device(gaze, rings, (1, 1), None) == EINVAL
        assert ctx.foveate_density_phased_device((float("nan"), 1.0), rings, (1, 1), m.ptr) == EINVAL
        assert ctx.foveate_density_phased_device(gaze, [(5, 2), (3, 4), (8,)], (1, 1), m.ptr) == EINVAL
        for bad in (dict(mask=None), dict(rgb=None), dict(width=0), dict(height=16385), dict(rgb=img.ptr + 2), dict(mask=img.ptr + 16)):
            a = dict(mask=m.ptr, width=w, height=h, phase_xy=(3, 5), rgb=img.ptr)
            a.update(bad)
            assert ctx.fill_density_phased_device(**a)[0] == EINVAL, bad
        ctx.sync()
        assert np.all(m.get("mask") == MASK_CANARY) and np.array_equal(img.get("rgb").view(np.uint32), np.full((w * h, 3), CANARY_F32).view(np.uint32))
    finally:
        m.free()
        img.free()


# ---- rendered frames ------------------------------------------------------------------------------------------------

def _psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


FRAME = (48, 32)
E2E_SPEC = "4:1,9:2,15:4,8"


def test_rendered_frames_at_rest_converge_on_the_full_render(model):
    """classroom_n8_thr02 at 48 x 32, gaze centred, the camera still, from a cut: in frame 0 the byte-0 pixels carry adanerf_render's bytes
    and every pixel is rejected; from frame 1 on nothing is rejected; after frame 63 every pixel has been rendered (count >= 1) and the
    resolved frame is closer to the full render than the fill-only frame is"""
    z, sc, d = model
    w, h = FRAME
    n = w * h
    gaze = (0.5 * w, 0.5 * h)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        r.set_camera(z["pose"], z["rot"])
        with pytest.raises(R.AdaNeRFError):
            r.render_foveated_temporal()                         # not enabled
        with pytest.raises(R.AdaNeRFError):
            r.enable_foveated_temporal()                         # no gaze and rings yet
        full, full8 = [a.copy() for a in r.render_numpy()[:2]]
        r.foveate_density(gaze, E2E_SPEC)
        fill_only = r.render_foveated()[0].copy()
        r.enable_foveated_temporal()
        rejected, psnr_at = [], {}
        for k in range(64):
            rgb, rgba8, mask, rej, rendered, st = r.render_foveated_temporal()
            rejected.append(rej)
            lattice = R.density_mask_phased(w, h, gaze, E2E_SPEC, SR.phase_of(k))
            assert rendered == int(np.count_nonzero(lattice == 0)) and rej == int(np.count_nonzero(mask == 0))
            assert np.array_equal(r._ft_dmask.numpy(), lattice), k
            if k == 0:
                on = lattice == 0
                assert np.array_equal(bits(rgb[on]), bits(full[on])) and np.array_equal(rgba8[on], full8[on])
                assert np.array_equal(bits(rgb), bits(fill_only)) and np.array_equal(lattice, R.density_mask(w, h, gaze, E2E_SPEC))
            if k + 1 in (1, 4, 16, 64):
                psnr_at[k + 1] = _psnr(rgb, full)
        count = r._ft_sets[r._ft_hist[0]][2].numpy()
        p_fill = _psnr(fill_only, full)
        print("48x32 %s at rest: PSNR against the full render after 1 / 4 / 16 / 64 frames %s, fill only %.3f dB; rejected per call %s; smallest count %d"
              % (E2E_SPEC, ", ".join("%.3f" % psnr_at[k] for k in (1, 4, 16, 64)), p_fill, rejected[:3], int(count.min())))
        record("foveated_temporal_at_rest", psnr_after={str(k): v for k, v in psnr_at.items()}, psnr_fill_only=p_fill, rejected=rejected[:4])
        assert rejected[0] == n and all(v == 0 for v in rejected[1:])
        assert int(count.min()) >= 1
        assert psnr_at[64] > p_fill
        # a cut, and a frame size change, drop the history; render_foveated is what it was
        r.reset_foveated_temporal()
        assert r.render_foveated_temporal()[3] == n and r.render_foveated_temporal()[3] == 0
        assert np.array_equal(bits(r.render_foveated()[0]), bits(fill_only))      # its own mask stayed at phase (0, 0)
        r.set_frame_size(24, 16)
        with pytest.raises(R.AdaNeRFError):
            r.render_foveated_temporal()                         # the mask went with the frame size
        r.foveate_density((12.0, 8.0), E2E_SPEC)
        out = r.render_foveated_temporal()
        assert out[3] == 24 * 16 and out[0].shape == (24 * 16, 3) and r.render_foveated_temporal()[3] == 0


LATERAL_STEP = 0.01      # of the view cell's size per frame, as tests/test_gpu_temporal.py


def test_rendered_frames_on_a_lateral_path_equal_the_reference_chain(model):
    """eight frames along the temporal tests' lateral path: every resolved frame, its history depth and count equal the definition fed
    with the same device-rendered, device-filled frames; the PSNR against the last pose's full render is recorded beside the fill-only one"""
    z, sc, d = model
    w, h = FRAME
    frames = 8
    gaze = (0.5 * w, 0.5 * h)
    size = np.asarray(sc.view_cell_size, np.float32)
    poses = [(np.asarray(z["pose"], np.float32) + np.float32(LATERAL_STEP * k) * size * np.float32([1, 1, 0])).astype(np.float32) for k in range(frames)]
    rot = np.asarray(z["rot"], np.float32)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
        r.set_camera(poses[-1], rot)
        full = r.render_numpy()[0].copy()
        r.foveate_density(gaze, E2E_SPEC)
        r.enable_foveated_temporal()
        ref = None      # the definition's history: (rgb, depth, count, pos)
        for k, pos in enumerate(poses):
            r.set_camera(pos, rot)
            rgb, rgba8, mask, rej, rendered, st = r.render_foveated_temporal()
            phase = SR.phase_of(k)
            lattice = r._ft_dmask.numpy()
            cur, dm, acc = r._o_rgb.numpy(), r._rp_depth.numpy(), r._rp_acc.numpy()      # the filled frame the resolve was fed with
            hist = (None, None, None, None) if ref is None else ref
            want = SR.sparse_f32(sc, w, h, False, lattice, phase, cur, dm, acc, pos, rot, hist[0], hist[1], hist[2], hist[3], rot)
            ref = (want.rgb, want.depth, want.count, pos)
            assert np.array_equal(bits(rgb), bits(want.rgb)) and np.array_equal(mask, want.mask) and rej == want.rejected, k
            assert np.array_equal(rgba8, want.rgba8), k
            side = r._ft_hist[0]
            assert np.array_equal(bits(r._ft_sets[side][1].numpy()), bits(want.depth)) and np.array_equal(r._ft_sets[side][2].numpy(), want.count), k
        p_res, p_fill = _psnr(rgb, full), _psnr(cur, full)
        print("lateral path, step %g of the view cell, %d frames: PSNR against the last pose's full render: resolved %.3f dB, fill only %.3f dB; "
              "rejected at the last pose %d of %d" % (LATERAL_STEP, frames, p_res, p_fill, rej, w * h))
        record("foveated_temporal_lateral_path", step=LATERAL_STEP, frames=frames, psnr_resolved=p_res, psnr_fill_only=p_fill, rejected=rej, pixels=w * h)


# ---- hosts -----------------------------------------------------------------------------------------------------------

def test_cli_fovea_temporal_equals_the_python_host(model, tmp_path):
    """`adanerf --fovea-density .. --fovea-temporal ALPHA --script` written with -w: out.bmp holds a session's last frame, so the session is
    replayed up to a line; that frame equals NeuralRenderer.render_foveated_temporal over the logged poses, with the `gaze` and `cut` tokens
    applied where the script has them"""
    import os
    import subprocess
    from test_gpu_set_selection import _bmp_pixels, _cli_rotation
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    spec, alpha = "6:1,14:2,4", 0.25
    lines = ["+w", "# hold", "gaze 10.5 30 -w", "cut", "# hold", "+w"]
    w, h = 48, 40
    try:
        for k in (3, 4, 6):
            script = tmp_path / ("session%d.txt" % k)
            script.write_text("\n".join(lines[:k]) + "\n")
            out = subprocess.run([exe, d, "-s", str(w), str(h), "-w", "--script", str(script), "--log-camera", "--fovea-density", spec, "--fovea-temporal",
                                  str(alpha)], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            cam = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
            logged = [l.split() for l in out.stdout.splitlines() if l.startswith("foveated ")]
            assert len(cam) == k and len(logged) == k
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h)) as r:
                r.foveate_density((0.5 * w, 0.5 * h), spec)
                r.enable_foveated_temporal(alpha=alpha)
                for i in range(k):
                    if lines[i].startswith("gaze"):
                        r.foveate_density((10.5, 30.0), spec)
                    if lines[i] == "cut":
                        r.reset_foveated_temporal()
                    r.set_camera(np.array([float(v) for v in cam[i][3:6]], np.float32), _cli_rotation(float(cam[i][7]), float(cam[i][9])))
                    rgb, rgba, mask, rejected, rendered, st = r.render_foveated_temporal()
                    assert [int(logged[i][3]), int(logged[i][4])] == list(SR.phase_of(i)), i
                    assert [int(logged[i][6]), int(logged[i][8]), int(logged[i][10])] == [rendered, w * h, rejected], (k, i, logged[i])
            assert np.array_equal(_bmp_pixels(os.path.join(d, "out.bmp"), w, h), rgba[:, :3]), "after line %d (%s)" % (k, lines[k - 1])
        out = subprocess.run([exe, d, "-s", str(w), str(h), "--fovea-temporal", "0.1", "--frames", "1"], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "only with --fovea-density" in out.stdout
    finally:
        if os.path.exists(os.path.join(d, "out.bmp")):
            os.remove(os.path.join(d, "out.bmp"))


def test_evaluator_fovea_temporal_reports_both_scores(tmp_path):
    """evaluate(..., fovea_density=.., fovea_temporal=0.2) and fovea_temporal_still=3 on a synthetic 12 x 10 dataset of three poses: the plain
    and the fill-only keys and values are those of a run without the option; the resolved ones are what
    NeuralRenderer.render_foveated_temporal gives over the same sequence"""
    import json
    from adanerf_amd.evaluate import evaluate, psnr_from_mse
    from adanerf_amd.png import write_png
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    w, h = 12, 10
    spec = "2:1,4:2,4"
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
    fill_only, frecs = evaluate(md, str(ds), "test", None, precision="bf16", quiet=True, fovea_density=spec)
    extra = ["mean_psnr_foveated_temporal", "mean_foveated_temporal_rejected_fraction"]
    for kw, keys in ((dict(fovea_temporal=0.2), extra), (dict(fovea_temporal_still=3), extra + ["fovea_temporal_still"])):
        summary, recs = evaluate(md, str(ds), "test", str(tmp_path / ("pred_" + "_".join(sorted(kw)))), precision="bf16", quiet=True, fovea_density=spec, **kw)
        assert sorted(summary) == sorted(list(fill_only) + keys)
        assert all(summary[key] == fill_only[key] for key in fill_only if key not in ("mean_ms", "mean_ms_foveated"))
        still = kw.get("fovea_temporal_still", 0)
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, w, h)) as r:
            r.foveate_density((0.5 * w, 0.5 * h), spec)
            r.enable_foveated_temporal(alpha=kw.get("fovea_temporal", 0.1))
            for i, (pose, rot) in enumerate(poses):
                r.set_camera(pose, rot)
                if still:
                    r.reset_foveated_temporal()
                for _ in range(still or 1):
                    rgb, rgba8, mask, rejected, rendered, st = r.render_foveated_temporal()
                ref = gts[i].astype(np.float32).reshape(-1, 3) / 255.0
                mse = float(np.mean((rgb.astype(np.float64) - ref) ** 2))
                assert recs[i]["mse_foveated_temporal"] == mse and recs[i]["psnr_foveated_temporal"] == psnr_from_mse(mse), (kw, i)
                assert recs[i]["foveated_temporal_rejected_fraction"] == rejected / float(w * h)
                assert recs[i]["psnr_foveated"] == frecs[i]["psnr_foveated"] and recs[i]["psnr"] == frecs[i]["psnr"]
                assert (tmp_path / ("pred_" + "_".join(sorted(kw))) / ("%05d_foveated_temporal.png" % i)).exists()
        assert summary["mean_psnr_foveated_temporal"] == float(np.mean([x["psnr_foveated_temporal"] for x in recs]))
        if still:
            assert summary["fovea_temporal_still"] == 3 and all(x["foveated_temporal_rejected_fraction"] == 0.0 for x in recs)
        print("evaluator %s: mean PSNR full %.3f, fill only %.3f, resolved %.3f dB" % (kw, summary["mean_psnr"], summary["mean_psnr_foveated"],
                                                                                    summary["mean_psnr_foveated_temporal"]))
