"""Foveated ray density on the GPU: adanerf_foveate_density against the host mirror (itself checked against the brute-force definition in
tests/test_density_cpu.py), adanerf_fill_density against the numpy restatement of tests/density_reference.py byte for byte in all four
images, the whole path through NeuralRenderer.render_foveated against adanerf_render of the same frame, and every refusal.  Every buffer
has canary elements either side.  Fixture classroom_n8_thr02, bf16 shading, at 48 x 40 and 37 x 29 (ragged against every stride and
against the 128-ray tile).  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C

import numpy as np
import pytest

import adanerf_oracle as O
import density_reference as DR
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
PAD = 64
SIZES = [(48, 40), (37, 29)]
IDS = ["%dx%d" % s for s in SIZES]
# (gaze as a fraction of the frame, spec): the gaze inside, on a pixel corner, outside; 0..3 rings; every stride
SETTINGS = [((0.5, 0.5), "6:1,14:2,4"), ((0.31, 0.72), "4:1,9:2,15:4,8"), ((-0.4, 1.3), "30:2,8"), ((0.5, 0.5), "8"), ((0.1, 0.1), "5:1,1"),
            ((0.77, 0.2), "0:1,3:4,4")]
# per image of the fill: elements per pixel, dtype, the canary element
IMAGES = [("rgb", 3, np.float32, np.float32(-1234.5)), ("depth", 1, np.float32, np.float32(-77.25)), ("acc", 1, np.float32, np.float32(-3.5)),
          ("rgba8", 4, np.uint8, 0x5A)]
MASK_CANARY = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    z, meta, sc = load_case("classroom_n8_thr02")
    d = str(tmp_path_factory.mktemp("density_classroom_n8_thr02"))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, sc, d


@pytest.fixture(scope="module")
def ctx(model):
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 48, 40)) as r:
        r.set_camera(z["pose"], z["rot"])
        yield r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def differing(got, want):
    """the pixels [n] whose bytes differ.  One allowance, for fp32 images only: where the reference computed a NaN (inf - inf, 0 x inf, an
    operand that is one) any NaN agrees -- IEEE 754 leaves the sign and payload of a NaN an operation produces to the implementation, and
    numpy on the host and the GPU's VALU choose differently.  A value that is copied, not computed, is compared by its bits (single_tap)."""
    ne = bits(got).reshape(len(got), -1) != bits(want).reshape(len(want), -1)
    if got.dtype == np.float32:
        both = np.repeat(np.isnan(got) & np.isnan(want), 4, axis=1)
        ne &= ~both
    return np.any(ne, axis=1)


def single_tap(mask, w, h):
    """the unrendered pixels [n] bool whose used corners are one pixel: their value is that pixel's, bit for bit"""
    out = np.zeros(w * h, bool)
    for p in np.flatnonzero(np.isin(mask, (2, 4, 8))).tolist():
        y, x = divmod(p, w)
        c = DR.used_corners(x, y, int(mask[p]), w, h)
        out[p] = len(c) == 1 and mask[c[0]] == 0
    return out


def setting(w, h, k):
    (fx, fy), spec = SETTINGS[k]
    radius, stride = DR.parse_spec(spec)
    return (float(np.float32(fx * w)), float(np.float32(fy * h))), radius, stride, R.parse_fovea_density(spec)


class Canaried:
    """a device buffer of n elements of k values with PAD canary elements either side, starting `skew` bytes into its allocation"""

    def __init__(self, r, n, k, dt, canary, skew=0):
        self.r, self.n, self.k, self.dt, self.canary, self.skew = r, n, k, np.dtype(dt), canary, skew
        self.total = (PAD + n + PAD) * k
        self.dev = R.DeviceArray(r, (self.total * self.dt.itemsize + skew,), np.uint8)
        self.set(np.full((n, k), canary, dt))

    @property
    def ptr(self):
        return self.dev.ptr + self.skew + PAD * self.k * self.dt.itemsize

    def set(self, inner):
        a = np.full(self.total, self.canary, self.dt)
        a[PAD * self.k:(PAD + self.n) * self.k] = np.asarray(inner, self.dt).reshape(-1)
        self.dev.upload(np.concatenate([np.full(self.skew, 0x3C, np.uint8), a.view(np.uint8)]))

    def get(self, what=""):
        raw = self.dev.numpy()
        assert np.all(raw[:self.skew] == 0x3C)
        a = raw[self.skew:].view(self.dt)
        lo, hi = a[:PAD * self.k], a[(PAD + self.n) * self.k:]
        assert np.array_equal(bits(lo), bits(np.full_like(lo, self.canary))) and np.array_equal(bits(hi), bits(np.full_like(hi, self.canary))), \
            "wrote outside the %s buffer" % what
        return a[PAD * self.k:(PAD + self.n) * self.k].reshape(self.n, self.k).copy()

    def free(self):
        self.dev.free()


def device_mask(r, w, h, k, skew=0):
    """(rc, mask bytes) of adanerf_foveate_density for setting k into a canaried buffer"""
    gaze, radius, stride, rings = setting(w, h, k)
    m = Canaried(r, w * h, 1, np.uint8, MASK_CANARY, skew)
    try:
        rc = r.foveate_density_device(gaze, rings, m.ptr)
        r.sync()
        return rc, m.get("mask").reshape(-1)
    finally:
        m.free()


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
@pytest.mark.parametrize("skew", [0, 3], ids=["aligned", "misaligned"])
def test_device_mask_equals_the_host_mask(ctx, w, h, skew):
    ctx.set_frame_size(w, h)
    for k in range(len(SETTINGS)):
        gaze, radius, stride, rings = setting(w, h, k)
        rc, got = device_mask(ctx, w, h, k, skew)
        assert rc == 0, ctx.lib.adanerf_last_error(ctx.handle).decode()
        want = R.density_mask(w, h, gaze, rings)
        assert np.array_equal(got, want), (SETTINGS[k], np.flatnonzero(got != want)[:8])
        assert np.array_equal(want, DR.density_mask(w, h, gaze, radius, stride)), SETTINGS[k]


def synthetic(w, h, mask, seed):
    """random fp32 images with a NaN, both infinities and huge values among the rendered pixels, and distinct values everywhere else"""
    rng = np.random.default_rng(seed)
    n = w * h
    rgb = rng.uniform(-0.5, 1.5, (n, 3)).astype(np.float32)
    depth = (rng.uniform(0.0, 30.0, (n, 1)) * np.float32(2.0) ** rng.integers(-20, 20, (n, 1))).astype(np.float32)
    acc = rng.uniform(0.0, 1.0, (n, 1)).astype(np.float32)
    rgba8 = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    zeros = np.flatnonzero(mask == 0)
    if len(zeros) >= 8:
        pick = rng.choice(zeros, 8, replace=False)
        rgb[pick[0], 1] = np.nan
        rgb[pick[1], 0] = np.inf
        rgb[pick[2], 2] = -np.inf
        rgb[pick[3]] = np.float32(3e38)
        rgb[pick[4]] = np.float32(-3e38)
        depth[pick[5]] = np.inf
        depth[pick[6]] = np.nan
        acc[pick[7]] = np.float32(1e-42)      # a subnormal
    return [rgb, depth, acc, rgba8]


def check_fill(r, w, h, mask, seed, use=(True, True, True), count=True, tag=""):
    """one adanerf_fill_density over canaried synthetic images against the reference; use: depth, acc, rgba8 given (else NULL)"""
    n = w * h
    src = synthetic(w, h, mask, seed)
    d_mask = Canaried(r, n, 1, np.uint8, MASK_CANARY)
    d_mask.set(mask)
    bufs = [Canaried(r, n, k, dt, canary) for _, k, dt, canary in IMAGES]
    try:
        for b, a in zip(bufs, src):
            b.set(a)
        on = [True] + list(use)
        rc, unfilled = r.fill_density_device(d_mask.ptr, w, h, *[b.ptr if o else None for b, o in zip(bufs, on)], count=count)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        r.sync()
        want = DR.fill(mask, w, h, src[0], src[1] if use[0] else None, src[2] if use[1] else None, src[3] if use[2] else None)
        for b, a, wnt, o, (name, _, _, _) in zip(bufs, src, want[:4], on, IMAGES):
            got = b.get(name)
            exp = wnt.reshape(got.shape) if o else a      # an image that was not passed keeps every byte
            diff = differing(got, exp.reshape(got.shape))
            print("%s %s: %d of %d pixels differ (unfilled %s, reference %d)" % (tag, name, int(diff.sum()), n, unfilled, want[4]))
            assert not diff.any(), (tag, name, np.flatnonzero(diff)[:8])
            one = single_tap(mask, w, h)
            assert np.array_equal(bits(got[one]), bits(exp.reshape(got.shape)[one])), (tag, name, "a copied value changed its bits")
            keep = ~np.isin(mask, (2, 4, 8))
            assert np.array_equal(bits(got[keep]), bits(a[keep])), (tag, name, "a pixel with byte 0 or a foreign byte changed")
        assert np.array_equal(d_mask.get("mask").reshape(-1), mask), "mask modified"
        if count:
            assert unfilled == want[4], tag
        return unfilled, want[4]
    finally:
        d_mask.free()
        for b in bufs:
            b.free()


def caller_mask(w, h, k, seed):
    """a device-rule mask damaged by a caller: some rendered pixels marked unrendered (corners go missing), some pixels given foreign bytes
    (1, 3, 16, 255) and some unrendered pixels another stride"""
    gaze, radius, stride, rings = setting(w, h, k)
    mask = R.density_mask(w, h, gaze, rings).copy()
    rng = np.random.default_rng(seed)
    n = w * h
    zeros = np.flatnonzero(mask == 0)
    mask[rng.choice(zeros, max(len(zeros) // 6, 1), replace=False)] = rng.choice([2, 4, 8], max(len(zeros) // 6, 1))
    mask[rng.choice(n, n // 12, replace=False)] = rng.choice([1, 3, 16, 255], n // 12)
    mask[rng.choice(n, n // 12, replace=False)] = rng.choice([2, 4, 8], n // 12)
    return mask


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_fill_with_device_masks_equals_the_reference(ctx, w, h):
    ctx.set_frame_size(SIZES[0][0], SIZES[0][1])      # the fill takes its size as arguments: the context's own is another
    for k in range(len(SETTINGS)):
        gaze, radius, stride, rings = setting(w, h, k)
        mask = R.density_mask(w, h, gaze, rings)
        unfilled, _ = check_fill(ctx, w, h, mask, seed=100 + k, tag="%dx%d %s" % (w, h, SETTINGS[k][1]))
        assert unfilled == 0


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_fill_with_caller_masks_equals_the_reference(ctx, w, h):
    total = 0
    for k in (0, 1, 2):
        mask = caller_mask(w, h, k, seed=7 + k)
        assert set(np.unique(mask).tolist()) >= {0, 1, 2, 3, 4, 8, 16, 255}
        unfilled, ref = check_fill(ctx, w, h, mask, seed=200 + k, tag="%dx%d caller %d" % (w, h, k))
        total += unfilled
    assert total > 0      # the damaged masks do leave pixels without their corners
    every = np.full(w * h, 8, np.uint8)      # no rendered pixel at all: every pixel is counted, nothing is written
    unfilled, _ = check_fill(ctx, w, h, every, seed=300, tag="all 8")
    assert unfilled == w * h
    foreign = np.full(w * h, 5, np.uint8)
    assert check_fill(ctx, w, h, foreign, seed=301, tag="all foreign")[0] == 0


@pytest.mark.parametrize("use", [(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, False)],
                         ids=["rgb only", "depth", "acc", "rgba8", "depth+acc"])
def test_fill_optional_images(ctx, use):
    w, h = SIZES[1]
    gaze, radius, stride, rings = setting(w, h, 1)
    check_fill(ctx, w, h, R.density_mask(w, h, gaze, rings), seed=400, use=use, tag="optional %s" % (use,))
    check_fill(ctx, w, h, caller_mask(w, h, 1, 9), seed=401, use=use, count=False, tag="optional, no counter %s" % (use,))


def full_and_foveated(r, w, h, k):
    """(the full frame's four images, render_foveated's four images, rendered, the mask) at the camera and pixel offset in force"""
    n = w * h
    gaze, radius, stride, rings = setting(w, h, k)
    depth, acc = R.DeviceArray(r, (n,), np.float32), R.DeviceArray(r, (n,), np.float32)
    try:
        r.set_aux_outputs(depth, acc)
        rgb, rgba8, _ = r.render_numpy()
        full = [rgb.copy(), depth.numpy().copy(), acc.numpy().copy(), rgba8.copy()]
        r.foveate_density(gaze, rings)
        # the renderer's images start from other bytes than the full frame's: what is not rendered must come from the fill alone
        r._o_rgb.upload(np.full((n, 3), -5.0, np.float32))
        r._o_rgba.upload(np.full((n, 4), 7, np.uint8))
        depth.upload(np.full(n, -6.0, np.float32))
        acc.upload(np.full(n, -7.0, np.float32))
        f_rgb, f_rgba8, rendered, st = r.render_foveated()
        r.sync()
        got = [f_rgb, depth.numpy().copy(), acc.numpy().copy(), f_rgba8]
        assert st.rays == rendered
        return full, got, rendered, R.density_mask(w, h, gaze, rings)
    finally:
        r.set_aux_outputs(None, None)
        depth.free()
        acc.free()


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
@pytest.mark.parametrize("offset", [(0.0, 0.0), (0.25, -0.375)], ids=["centre", "offset"])
def test_render_foveated_is_the_full_frame_on_the_lattice_and_its_fill_elsewhere(ctx, w, h, offset):
    ctx.set_frame_size(w, h)
    ctx.set_pixel_offset(*offset)
    try:
        for k in (0, 1):
            full, got, rendered, mask = full_and_foveated(ctx, w, h, k)
            assert rendered == int(np.count_nonzero(mask == 0)) and 0 < rendered < w * h
            assert np.array_equal(ctx._fd_mask.numpy(), mask)
            want = DR.fill(mask, w, h, *full)
            assert want[4] == 0
            for g, f, wnt, (name, kk, _, _) in zip(got, full, want[:4], IMAGES):
                g, f, wnt = g.reshape(w * h, kk), f.reshape(w * h, kk), wnt.reshape(w * h, kk)
                lattice = mask == 0
                assert np.array_equal(bits(g[lattice]), bits(f[lattice])), (name, "a rendered pixel differs from adanerf_render's")
                diff = differing(g, wnt)
                print("%dx%d %s %s: %d of %d pixels differ from the reference fill, rendered %d" % (w, h, SETTINGS[k][1], name, int(diff.sum()), w * h, rendered))
                assert not diff.any(), (name, np.flatnonzero(diff)[:8])
            assert len(np.unique(got[3][:, :3])) > 16
    finally:
        ctx.set_pixel_offset(0.0, 0.0)


def test_a_frame_size_change_drops_the_mask(ctx):
    ctx.set_frame_size(*SIZES[0])
    ctx.foveate_density((10.0, 10.0), "4:1,2")
    ctx.render_foveated()
    ctx.set_frame_size(*SIZES[1])
    with pytest.raises(R.AdaNeRFError, match="foveate_density"):
        ctx.render_foveated()
    ctx.foveate_density((10.0, 10.0), "4:1,2")
    assert ctx.render_foveated()[2] == int(np.count_nonzero(R.density_mask(SIZES[1][0], SIZES[1][1], (10.0, 10.0), "4:1,2") == 0))


def test_foveate_density_refusals_write_nothing(ctx, model):
    w, h = SIZES[1]
    ctx.set_frame_size(w, h)
    nan, inf = float("nan"), float("inf")
    m = Canaried(ctx, w * h, 1, np.uint8, MASK_CANARY)
    i32 = C.c_int32

    def call(r, gaze, radius, stride, nr=None, ptr=m.ptr):
        rad = None if radius is None else (i32 * max(len(radius), 1))(*radius)
        st = None if stride is None else (i32 * max(len(stride), 1))(*stride)
        return r.lib.adanerf_foveate_density(r.handle, gaze[0], gaze[1], len(radius) if nr is None else nr, rad, st, ptr)
    try:
        g = (10.0, 9.0)
        bad = [((nan, 9.0), [2, 5], [1, 2, 4], None), ((10.0, inf), [2, 5], [1, 2, 4], None), (g, [], [1], -1), (g, list(range(9)), [1] * 10, None),
               (g, [-1, 5], [1, 2, 4], None), (g, [5, 5], [1, 2, 4], None), (g, [5, 2], [1, 2, 4], None), (g, [2, 5], [1, 3, 4], None),
               (g, [2, 5], [0, 2, 4], None), (g, [2, 5], [1, 2, 16], None), (g, [2, 5], [2, 1, 4], None), (g, [2, 5], [1, 4, 2], None),
               (g, None, [1, 2, 4], 2), (g, [2, 5], None, 2)]
        for gaze, radius, stride, nr in bad:
            assert call(ctx, gaze, radius, stride, nr) == EINVAL, (gaze, radius, stride, nr)
            assert "adanerf_foveate_density" in ctx.lib.adanerf_last_error(ctx.handle).decode()
        assert call(ctx, g, [2, 5], [1, 2, 4], ptr=None) == EINVAL
        z, sc, d = model
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 16), shard_rank=0, shard_world=2) as shard:
            assert call(shard, g, [2, 5], [1, 2, 4]) == EUNSUPPORTED
            assert "shard_world" in shard.lib.adanerf_last_error(shard.handle).decode()
            assert call(shard, (nan, 9.0), [2, 5], [1, 2, 4]) == EINVAL
            shard.sync()
        ctx.sync()
        assert np.all(m.get("mask") == MASK_CANARY)
        assert call(ctx, g, [2, 5], [1, 2, 4]) == 0      # and the same call with a good setting does write
        ctx.sync()
        assert np.array_equal(m.get("mask").reshape(-1), R.density_mask(w, h, g, [(2, 1), (5, 2), (4,)]))
    finally:
        m.free()


def test_fill_density_refusals_write_nothing(ctx):
    w, h = SIZES[1]
    n = w * h
    mask = R.density_mask(w, h, (12.0, 9.0), "4:1,9:2,4")
    src = synthetic(w, h, mask, 500)
    d_mask = Canaried(ctx, n, 1, np.uint8, MASK_CANARY)
    d_mask.set(mask)
    bufs = [Canaried(ctx, n, k, dt, canary) for _, k, dt, canary in IMAGES]
    try:
        for b, a in zip(bufs, src):
            b.set(a)
        rgb, depth, acc, rgba8 = [b.ptr for b in bufs]
        u = C.c_int32(-7)

        def call(m=d_mask.ptr, ww=w, hh=h, a=rgb, b=depth, c=acc, d=rgba8):
            return ctx.lib.adanerf_fill_density(ctx.handle, m, ww, hh, a, b, c, d, C.byref(u))
        bad = [dict(m=None), dict(a=None), dict(ww=0), dict(hh=0), dict(ww=-3), dict(ww=16385), dict(hh=16385),
               dict(a=rgb + 2), dict(b=depth + 1), dict(c=acc + 2), dict(d=rgba8 + 3),
               dict(b=rgb), dict(b=rgb + 4 * (3 * n - 1)), dict(c=depth), dict(c=depth + 4 * (n - 1)), dict(d=acc), dict(d=rgb + 8 * n),
               dict(m=rgb), dict(m=rgb + 12 * n - 1), dict(m=depth + 4), dict(m=rgba8 + 4 * n - 1), dict(a=d_mask.ptr - 12 * n + 4)]
        for kw in bad:
            assert call(**kw) == EINVAL, kw
            assert "adanerf_fill_density" in ctx.lib.adanerf_last_error(ctx.handle).decode()
        assert u.value == -7
        ctx.sync()
        for b, a, (name, _, _, _) in zip(bufs, src, IMAGES):
            assert np.array_equal(bits(b.get(name)), bits(a.reshape(b.n, b.k))), name
        assert np.array_equal(d_mask.get("mask").reshape(-1), mask)
        assert call() == 0 and u.value == 0      # and the same call with its own arguments fills
    finally:
        d_mask.free()
        for b in bufs:
            b.free()


def test_cli_fovea_density_equals_the_python_host(ctx, model, tmp_path):
    """`adanerf --fovea-density ... --script` written with -w: out.bmp holds a session's last frame, so the session is replayed up to a line;
    each of those frames equals NeuralRenderer.render_foveated at the logged pose -- with the gaze at the frame centre, after a `gaze` token
    and after a `size` token (the mask is filled again for the new size, the gaze stays)."""
    import os
    import subprocess
    from test_gpu_set_selection import _bmp_pixels, _cli_rotation
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    spec = "6:1,14:2,4"
    lines = ["+w", "gaze 10.5 30 -w", "size 37 29"]
    w, h = SIZES[0]
    gaze = (0.5 * w, 0.5 * h)
    shown = []
    try:
        for k in (1, 2, 3):
            script = tmp_path / ("session%d.txt" % k)
            script.write_text("\n".join(lines[:k]) + "\n")
            out = subprocess.run([exe, d, "-s", str(SIZES[0][0]), str(SIZES[0][1]), "-w", "--script", str(script), "--log-camera", "--fovea-density", spec],
                                 capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            cam = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
            assert len(cam) == k
            pos, rot = np.array([float(v) for v in cam[-1][3:6]], np.float32), _cli_rotation(float(cam[-1][7]), float(cam[-1][9]))
            if k >= 2:
                gaze = (10.5, 30.0)
            if k == 3:
                w, h = SIZES[1]
            ctx.set_frame_size(w, h)
            ctx.set_camera(pos, rot)
            ctx.foveate_density(gaze, spec)
            _, rgba, rendered, _ = ctx.render_foveated()
            shown.append(rgba)
            assert np.array_equal(_bmp_pixels(os.path.join(d, "out.bmp"), w, h), rgba[:, :3]), "after line %d (%s)" % (k, lines[k - 1])
            logged = [l.split() for l in out.stdout.splitlines() if l.startswith("foveated ")]
            assert len(logged) == k and [int(logged[-1][3]), int(logged[-1][5])] == [rendered, w * h]
        assert not np.array_equal(shown[0], shown[1])      # the gaze does change the frame
    finally:
        ctx.set_camera(z["pose"], z["rot"])
        if os.path.exists(os.path.join(d, "out.bmp")):
            os.remove(os.path.join(d, "out.bmp"))
