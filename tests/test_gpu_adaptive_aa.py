"""Adaptive supersampling on the GPU: adanerf_contrast_mask against the brute-force numpy definition (tests/contrast_reference.py) at the
sizes where its stencil, its tile seams and its packed stores can go wrong; adanerf_accumulate_masked / adanerf_resolve_mean_masked against
their numpy restatements; and the frame the hosts build from them (NeuralRenderer.render_supersampled_adaptive, the CLI, the evaluator)
against render_supersampled on the flagged pixels and adanerf_render on the others.  Every comparison is exact equality; every buffer has
canary elements either side.  Fixture classroom_n8_thr02, bf16 shading, 16 x 12.  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import contrast_reference as CR
from conftest import ROOT, case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

EINVAL = -1
PAD = 64
f32 = np.float32
W, H = 16, 12                  # the end-to-end frame
THRESHOLD = 0.3

# the kernel's tile, read from its source: the sizes below are built from it, so a changed tile changes the test
_src = open(os.path.join(ROOT, "adanerf_amd", "csrc", "k_contrast.hip.hpp")).read()
TILE_W, TILE_H = (int(v) for v in re.search(r"kContrastTileW = (\d+), kContrastTileH = (\d+)", _src).groups())
SIZES = [(1, 1), (1, 9), (9, 1), (3, 3),
         (TILE_W - 1, TILE_H - 1),                  # one pixel less than a tile in each axis
         (TILE_W + 1, TILE_H + 1),                  # crosses a tile seam by one pixel in both axes
         (2 * TILE_W + 3, 2 * TILE_H + 1)]          # three tiles by three, a width not divisible by 4 (every row at another alignment)
IDS = ["%dx%d" % s for s in SIZES]
assert (2 * TILE_W + 3) % 4 != 0
RGB_CANARY, MASK_CANARY = f32(-1234.5), 0xA5


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    z, meta, sc = load_case("classroom_n8_thr02")
    d = str(tmp_path_factory.mktemp("adaptive_classroom_n8_thr02"))
    O.write_model_dir(d, sc, case_weights(meta))
    return z, sc, d


@pytest.fixture(scope="module")
def ctx(model):
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as r:
        r.set_camera(z["pose"], z["rot"])
        yield r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


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


# ---- adanerf_contrast_mask ------------------------------------------------------------------------------------------------------------

def seam_pixels(w, h):
    """the pixels either side of a tile seam and on the image border: where a halo value is read"""
    xs = sorted({x for x in (0, w - 1, TILE_W - 1, TILE_W, 2 * TILE_W - 1, 2 * TILE_W) if 0 <= x < w})
    ys = sorted({y for y in (0, h - 1, TILE_H - 1, TILE_H, 2 * TILE_H - 1, 2 * TILE_H) if 0 <= y < h})
    return [(x, y) for y in ys for x in range(w)] + [(x, y) for x in xs for y in range(h)]


def image(seed, w, h, specials):
    """flat patches of random colours in [-0.5, 1.5], about 5 pixels a side, under noise of +-0.04 -- so that a threshold between the noise
    and the patch contrast flags some pixels and leaves others; with `specials`, NaN / +-inf / -0 / far out-of-range values on the
    seams, the borders and elsewhere"""
    rng = np.random.default_rng(seed)
    patch = rng.uniform(-0.5, 1.5, ((h + 4) // 5, (w + 4) // 5, 3))
    a = np.repeat(np.repeat(patch, 5, axis=0), 5, axis=1)[:h, :w].reshape(h * w, 3)
    a = (a + rng.uniform(-0.04, 0.04, a.shape)).astype(f32)
    if specials:
        vals = [f32("nan"), f32("inf"), f32("-inf"), f32(-0.0), f32(1e30), f32(-1e30), f32(1.0), f32(0.0)]
        where = seam_pixels(w, h)
        pick = [where[i] for i in rng.permutation(len(where))[:max(len(where) // 3, 1)]]
        pick += [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(max(w * h // 8, 1))]
        for k, (x, y) in enumerate(pick):
            a[y * w + x, int(rng.integers(0, 3))] = vals[k % len(vals)]
    return a


def run_contrast(r, rgb, w, h, thr, skew=0, count=True, twice=False):
    """(mask bytes, n_flagged) of adanerf_contrast_mask over canaried buffers; the image must keep its bits"""
    d_rgb = Canaried(r, w * h, 3, f32, RGB_CANARY)
    d_mask = Canaried(r, w * h, 1, np.uint8, MASK_CANARY, skew)
    try:
        d_rgb.set(rgb)
        rc, n = r.contrast_mask(d_rgb.ptr, w, h, thr, d_mask.ptr, count=count)
        assert rc == 0, r.lib.adanerf_last_error(r.handle).decode()
        r.sync()
        got = d_mask.get("mask").reshape(-1)
        if twice:      # the same bytes and the same count on a second call: the counter starts from 0 each time
            d_mask.set(np.full(w * h, 0x77, np.uint8))
            rc2, n2 = r.contrast_mask(d_rgb.ptr, w, h, thr, d_mask.ptr, count=count)
            r.sync()
            assert rc2 == 0 and n2 == n and np.array_equal(d_mask.get("mask").reshape(-1), got)
        assert np.array_equal(bits(d_rgb.get("rgb")), bits(np.asarray(rgb, f32).reshape(-1, 3))), "the image was modified"
        return got, n
    finally:
        d_rgb.free()
        d_mask.free()


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "odd address"])
def test_contrast_mask_equals_the_reference(ctx, w, h, skew):
    seen = set()
    for k, (thr, specials) in enumerate(((0.0, False), (0.05, True), (0.3, False), (0.3, True), (0.7, True), (1.0, True))):
        rgb = image(1000 * w + 10 * h + k, w, h, specials)
        want, n_want = CR.contrast_mask(rgb, w, h, thr)
        got, n = run_contrast(ctx, rgb, w, h, thr, skew, twice=k == 3)
        print("%dx%d skew %d thr %.2f specials %d: %d of %d flagged (reference %d), %d bytes differ" %
              (w, h, skew, thr, specials, n, w * h, n_want, int(np.count_nonzero(got != want))))
        assert np.array_equal(got, want), (thr, specials, np.flatnonzero(got != want)[:8])
        assert n == n_want == int(np.count_nonzero(got == 0))
        seen |= set(got.tolist())
        got_async, none = run_contrast(ctx, rgb, w, h, thr, skew, count=False)      # a NULL n_flagged: the same bytes, no count
        assert none is None and np.array_equal(got_async, want)
    assert seen == ({1} if w * h == 1 else {0, 1})


def test_contrast_mask_on_the_tile_seams(ctx):
    """NaN / inf / out-of-range values on a seam and in the halo, and the exact-threshold pair straddling a seam in every direction"""
    w, h = TILE_W + 1, TILE_H + 1
    thr = f32(0.3)
    lo = f32(0.125)
    hi = f32(lo + thr)
    assert f32(hi - lo) == thr
    above = np.nextafter(hi, f32(2))
    sx, sy = TILE_W - 1, TILE_H - 1      # the last pixel of the first tile; its neighbours at + 1 belong to the next tile
    for name, (qx, qy) in (("vertical seam", (sx + 1, 3)), ("horizontal seam", (5, sy + 1)), ("corner", (sx + 1, sy + 1))):
        px, py = qx - (1 if qx == sx + 1 else 0), qy - (1 if qy == sy + 1 else 0)
        for ch in range(3):
            rgb = np.full((h * w, 3), lo, f32)
            rgb[qy * w + qx, ch] = hi
            got, n = run_contrast(ctx, rgb, w, h, float(thr))
            assert n == 0 and np.all(got == 1), (name, ch, "a pair exactly on the threshold was flagged")
            rgb[qy * w + qx, ch] = above
            got, n = run_contrast(ctx, rgb, w, h, float(thr))
            want, n_want = CR.contrast_mask(rgb, w, h, float(thr))
            assert np.array_equal(got, want) and n == n_want, (name, ch)
            assert got[py * w + px] == 0 and got[qy * w + qx] == 0, (name, ch, "the pair one ulp above the threshold was not flagged on both sides")
    # special values placed on the seam pixels only: what one tile computes of them, its neighbour reads from its halo
    rgb = np.full((h * w, 3), 0.5, f32)
    vals = [f32("nan"), f32("inf"), f32("-inf"), f32(7.0), f32(-7.0), f32(-0.0), f32(0.81), f32(0.19)]
    for k, (x, y) in enumerate([(sx, 2), (sx + 1, 4), (sx, sy), (sx + 1, sy + 1), (3, sy), (8, sy + 1), (sx + 1, sy), (sx, sy + 1), (0, 0), (w - 1, h - 1)]):
        rgb[y * w + x, k % 3] = vals[k % len(vals)]
    for t in (0.3, 0.49, 0.5):
        got, n = run_contrast(ctx, rgb, w, h, t)
        want, n_want = CR.contrast_mask(rgb, w, h, t)
        assert np.array_equal(got, want) and n == n_want, t
        assert n < w * h and (n > 0 or t >= 0.5)      # no clamped value lies more than 0.5 from the background's 0.5


def test_contrast_mask_is_independent_of_the_frame_size_and_equals_the_host_mirror(ctx):
    w, h = 2 * TILE_W + 3, 2 * TILE_H + 1
    assert (ctx.info.width, ctx.info.height) == (W, H)
    rgb = image(77, w, h, True)
    got, n = run_contrast(ctx, rgb, w, h, 0.2)
    host, n_host = R.host_contrast_mask(rgb, w, h, 0.2)
    assert np.array_equal(got, host) and n == n_host


def test_contrast_mask_refusals_write_nothing(ctx):
    w, h = 21, 9
    n = w * h
    rgb = image(5, w, h, False)
    d_rgb = Canaried(ctx, n, 3, f32, RGB_CANARY)
    d_mask = Canaried(ctx, n, 1, np.uint8, MASK_CANARY)
    cnt = C.c_int32(-7)
    nan, inf = float("nan"), float("inf")
    try:
        d_rgb.set(rgb)

        def call(a=d_rgb.ptr, ww=w, hh=h, t=0.3, m=d_mask.ptr):
            return ctx.lib.adanerf_contrast_mask(ctx.handle, a, ww, hh, t, m, C.byref(cnt))
        bad = [dict(a=None), dict(m=None), dict(ww=0), dict(hh=0), dict(ww=-2), dict(ww=16385), dict(hh=16385), dict(t=nan), dict(t=inf), dict(t=-inf),
               dict(t=-0.01), dict(t=1.01), dict(a=d_rgb.ptr + 1), dict(a=d_rgb.ptr + 2), dict(m=d_rgb.ptr), dict(m=d_rgb.ptr + 12 * n - 1),
               dict(m=d_rgb.ptr - n + 1), dict(a=d_mask.ptr - 12 * n + 4)]
        for kw in bad:
            assert call(**kw) == EINVAL, kw
            assert "adanerf_contrast_mask" in ctx.lib.adanerf_last_error(ctx.handle).decode()
        assert cnt.value == -7
        ctx.sync()
        assert np.all(d_mask.get("mask") == MASK_CANARY) and np.array_equal(bits(d_rgb.get("rgb")), bits(rgb))
        assert call() == 0      # and the same call with its own arguments writes
        assert np.array_equal(d_mask.get("mask").reshape(-1), CR.contrast_mask(rgb, w, h, 0.3)[0]) and cnt.value == CR.contrast_mask(rgb, w, h, 0.3)[1]
    finally:
        d_rgb.free()
        d_mask.free()


# ---- adanerf_accumulate_masked / adanerf_resolve_mean_masked ---------------------------------------------------------------------------

NAN_PAYLOAD = 0x7FC12345      # what an unselected pixel holds: a value no arithmetic would leave alone


def mask_of(seed, n):
    rng = np.random.default_rng(seed)
    m = rng.choice(np.array([0, 1, 2, 31, 32, 255], np.uint8), n)
    m[:min(n, 6)] = np.array([0, 1, 2, 31, 32, 255], np.uint8)[:min(n, 6)]
    return m


def frames_of(seed, n, count):
    rng = np.random.default_rng(seed)
    out = [rng.uniform(-0.5, 1.5, (n, 3)).astype(f32) for _ in range(count)]
    if n >= 8:
        out[0][3, 1], out[0][4, 0], out[0][5, 2] = np.nan, np.inf, -np.inf
        out[-1][4, 0], out[-1][6] = -np.inf, f32(3e38)      # inf - inf in the sum; an overflow
    return out


@pytest.mark.parametrize("n", [0, 1, 7, 300, 70001], ids=lambda n: "n%d" % n)      # below a wave, ragged against 256, several blocks
@pytest.mark.parametrize("values", [1, 2, 5, 0x80000001, 0xFFFFFFFF], ids=lambda v: "values%x" % v)
def test_masked_pair_equals_the_reference(ctx, n, values):
    frames = {0: 1, 1: 1, 7: 4, 300: 9, 70001: 4}[n]
    mask = mask_of(n + values % 97, n)
    sel = CR.selected(mask, values)
    src = frames_of(n, max(n, 1), frames)
    src = [a[:n] for a in src]
    canary3 = np.full((n, 3), NAN_PAYLOAD, np.uint32).view(f32)
    d_mask = Canaried(ctx, n, 1, np.uint8, MASK_CANARY)
    d_rgb = Canaried(ctx, n, 3, f32, RGB_CANARY)
    d_sum = Canaried(ctx, n, 3, f32, f32(-77.25))
    d_out = Canaried(ctx, n, 3, f32, f32(-3.5))
    d_rgba = Canaried(ctx, n, 4, np.uint8, 0x5A)
    try:
        d_mask.set(mask)
        d_sum.set(canary3)
        want = canary3.copy()
        for k, a in enumerate(src):
            d_rgb.set(a)
            ctx.accumulate_masked_device(d_rgb.ptr, d_mask.ptr, values, n, d_sum.ptr, first=k == 0)
            want = CR.accumulate_masked(a, mask, values, want, k == 0)
            ctx.sync()
            got = d_sum.get("sum")
            # One allowance: where an ADDITION gave the reference a NaN (inf - inf, a NaN operand) any NaN agrees -- IEEE 754 leaves the sign
            # and payload of a NaN an operation produces to the implementation.  The first frame is copied, not computed: compared by its bits.
            same_nan = np.isnan(got) & np.isnan(want) & sel[:, None] & (k > 0)
            assert np.array_equal(got.view(np.uint32)[~same_nan], want.view(np.uint32)[~same_nan]), (k, "sum")
            assert np.all(got.view(np.uint32)[~sel] == NAN_PAYLOAD), "an unselected pixel of the sum changed"
            assert np.array_equal(bits(d_rgb.get("rgb")), bits(a)), "the frame was modified"
            want = got      # later steps start from the device's own bits
        before_rgb, before_rgba = canary3.copy(), np.full((n, 4), 0x5A, np.uint8)
        d_out.set(before_rgb)
        ctx.resolve_mean_masked_device(d_sum.ptr, d_mask.ptr, values, n, frames, d_rgba.ptr, d_out.ptr)
        ctx.sync()
        total = d_sum.get("sum")
        want_rgb, want_rgba = CR.resolve_mean_masked(total, mask, values, frames, before_rgb, before_rgba)
        got_rgb, got_rgba = d_out.get("rgb out"), d_rgba.get("rgba8")
        nan = np.isnan(want_rgb) & np.isnan(got_rgb) & sel[:, None] & np.isnan(total)      # NaN / frames: the same allowance, for the division
        assert np.array_equal(got_rgb.view(np.uint32)[~nan], want_rgb.view(np.uint32)[~nan])
        assert np.array_equal(got_rgba, want_rgba)
        assert np.all(got_rgb.view(np.uint32)[~sel] == NAN_PAYLOAD) and np.all(got_rgba[~sel] == 0x5A)
        assert np.array_equal(bits(total), bits(got))      # the resolve does not write the sum
        # in place (d_rgb_f32_out == d_sum), the 8-bit image alone, the fp32 image alone
        ctx.resolve_mean_masked_device(d_sum.ptr, d_mask.ptr, values, n, frames, None, d_sum.ptr)
        ctx.sync()
        in_place = d_sum.get("sum")
        assert np.array_equal(in_place.view(np.uint32)[sel], got_rgb.view(np.uint32)[sel]) and np.all(in_place.view(np.uint32)[~sel] == NAN_PAYLOAD)
        assert np.array_equal(d_rgba.get("rgba8"), got_rgba) and np.array_equal(bits(d_mask.get("mask").reshape(-1)), bits(mask))
        print("n %d values %x frames %d: %d selected" % (n, values, frames, int(sel.sum())))
    finally:
        for b in (d_mask, d_rgb, d_sum, d_out, d_rgba):
            b.free()


def test_masked_pair_on_selected_pixels_is_the_unmasked_pair(ctx):
    """a mask that selects everything: the masked kernels write what adanerf_accumulate / adanerf_resolve_mean write"""
    n = 1000
    src = frames_of(9, n, 4)
    mask = np.zeros(n, np.uint8)
    d_mask = R.DeviceArray(ctx, (n,), np.uint8).upload(mask)
    bufs = [R.DeviceArray(ctx, (n, 3), f32) for _ in range(3)] + [R.DeviceArray(ctx, (n, 4), np.uint8) for _ in range(2)]
    d_rgb, d_a, d_b, d_ra, d_rb = bufs
    try:
        for k, a in enumerate(src):
            d_rgb.upload(a)
            ctx.accumulate_device(d_rgb, n, d_a, first=k == 0)
            ctx.accumulate_masked_device(d_rgb, d_mask, 1, n, d_b, first=k == 0)
        assert np.array_equal(bits(d_a.numpy()), bits(d_b.numpy()))
        ctx.resolve_mean_device(d_a, n, 4, d_ra, d_a)
        ctx.resolve_mean_masked_device(d_b, d_mask, 1, n, 4, d_rb, d_b)
        assert np.array_equal(bits(d_a.numpy()), bits(d_b.numpy())) and np.array_equal(d_ra.numpy(), d_rb.numpy())
    finally:
        d_mask.free()
        for b in bufs:
            b.free()


def test_masked_pair_refusals_write_nothing(ctx):
    n = 50
    d_mask = Canaried(ctx, n, 1, np.uint8, MASK_CANARY)
    d_rgb = Canaried(ctx, n, 3, f32, RGB_CANARY)
    d_sum = Canaried(ctx, n, 3, f32, f32(-77.25))
    d_rgba = Canaried(ctx, n, 4, np.uint8, 0x5A)
    try:
        d_mask.set(np.zeros(n, np.uint8))
        lib, hnd = ctx.lib, ctx.handle

        def acc(a=d_rgb.ptr, m=d_mask.ptr, v=1, nn=n, s=d_sum.ptr):
            return lib.adanerf_accumulate_masked(hnd, a, m, v, nn, s, 1)

        def res(s=d_sum.ptr, m=d_mask.ptr, v=1, nn=n, f=4, b=d_rgba.ptr, o=d_rgb.ptr):
            return lib.adanerf_resolve_mean_masked(hnd, s, m, v, nn, f, b, o)
        for kw in (dict(a=None), dict(s=None), dict(m=None), dict(v=0), dict(nn=-1), dict(nn=0x7fffffff // 3 + 1), dict(a=d_rgb.ptr + 2), dict(s=d_sum.ptr + 1),
                   dict(s=d_rgb.ptr + 12), dict(m=d_sum.ptr + 5)):
            assert acc(**kw) == EINVAL, kw
            assert "adanerf_accumulate_masked" in lib.adanerf_last_error(hnd).decode()
        for kw in (dict(s=None), dict(b=None, o=None), dict(m=None), dict(v=0), dict(nn=-1), dict(f=0), dict(f=65537), dict(s=d_sum.ptr + 2), dict(b=d_rgba.ptr + 1),
                   dict(o=d_sum.ptr + 12), dict(b=d_sum.ptr), dict(b=d_rgb.ptr + 4), dict(m=d_rgb.ptr + 3), dict(m=d_rgba.ptr + 4 * n - 1)):
            assert res(**kw) == EINVAL, kw
            assert "adanerf_resolve_mean_masked" in lib.adanerf_last_error(hnd).decode()
        ctx.sync()
        for b, name in ((d_rgb, "rgb"), (d_sum, "sum"), (d_rgba, "rgba8")):
            assert np.array_equal(bits(b.get(name)), bits(np.full((b.n, b.k), b.canary, b.dt))), name
        assert acc() == 0 and res() == 0 and res(o=d_sum.ptr) == 0      # the same calls with their own arguments run
        ctx.sync()
    finally:
        for b in (d_mask, d_rgb, d_sum, d_rgba):
            b.free()


# ---- the frame the hosts build -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frames(ctx):
    """computed once: the plain frame and the fully supersampled frames of the fixture's pose at offset (0, 0)"""
    ctx.set_frame_size(W, H)
    ctx.set_pixel_offset(0.0, 0.0)
    rgb, rgba, _ = ctx.render_numpy()
    out = {1: (rgb.copy(), rgba.copy())}
    for s in (2, 3):
        m, b, _ = ctx.render_supersampled(s)
        out[s] = (m.copy(), b.copy())
    for a, b in out.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return out


def check_adaptive(ctx, frames, s, thr):
    plain_rgb, plain_rgba = frames[1]
    ss_rgb, ss_rgba = frames[s]
    want_mask, n_want = CR.contrast_mask(plain_rgb, W, H, thr)      # the reference applied to the device's own centre frame
    # the renderer's images start from other bytes: every pixel must come from this call
    ctx.render_numpy()
    ctx._o_rgb.upload(np.full((W * H, 3), -5.0, f32))
    ctx._o_rgba.upload(np.full((W * H, 4), 7, np.uint8))
    rgb, rgba, mask, n_refined, st = ctx.render_supersampled_adaptive(s, thr)
    flagged = want_mask == 0
    print("s %d threshold %.2f: %d of %d pixels flagged (%.1f %%), %d unflagged" % (s, thr, n_want, W * H, 100.0 * n_want / (W * H), W * H - n_want))
    assert np.array_equal(mask, want_mask) and n_refined == n_want == int(flagged.sum())
    assert np.array_equal(bits(rgb[flagged]), bits(ss_rgb[flagged])) and np.array_equal(rgba[flagged], ss_rgba[flagged]), "a flagged pixel is not render_supersampled's"
    assert np.array_equal(bits(rgb[~flagged]), bits(plain_rgb[~flagged])) and np.array_equal(rgba[~flagged], plain_rgba[~flagged]), "an unflagged pixel is not adanerf_render's"
    assert np.array_equal(bits(ctx._o_rgb.numpy()), bits(rgb)) and np.array_equal(ctx._o_rgba.numpy(), rgba)
    assert st.rays == W * H
    return flagged, st


@pytest.mark.parametrize("s", [2, 3])
def test_adaptive_frame_is_supersampled_on_the_edges_and_plain_elsewhere(ctx, frames, s):
    flagged, st = check_adaptive(ctx, frames, s, THRESHOLD)
    # a condition on the inputs: each class holds at least a quarter of the pixels, so that neither assertion above runs over nothing
    assert flagged.sum() >= W * H // 4 and (~flagged).sum() >= W * H // 4, (int(flagged.sum()), int((~flagged).sum()))
    differ = np.any(frames[s][0] != frames[1][0], axis=1)
    assert differ[flagged].any()      # and the two sources do differ on the flagged pixels: the test can tell them apart


def test_adaptive_thresholds_0_and_1(ctx, frames, monkeypatch):
    calls = []
    real = ctx.render_masked
    monkeypatch.setattr(ctx, "render_masked", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    flagged, _ = check_adaptive(ctx, frames, 2, 0.0)
    assert flagged.all() and len(calls) == 4      # all refined: the whole frame is render_supersampled's
    del calls[:]
    flagged, st = check_adaptive(ctx, frames, 2, 1.0)
    assert not flagged.any() and calls == []      # none refined: no masked pass is launched, the frame is adanerf_render's
    for bad_s in (1, 0, 9, True, 2.0):
        with pytest.raises(ValueError):
            ctx.render_supersampled_adaptive(bad_s, 0.3)
    for bad_t in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ctx.render_supersampled_adaptive(2, bad_t)


def test_adaptive_restores_the_offset_and_the_aux_maps_which_hold_the_centre_frame(ctx, frames):
    n = W * H
    maps = [R.DeviceArray(ctx, (n,), f32) for _ in range(3)]
    depth, acc, disp = maps
    try:
        ctx.set_pixel_offset(0.0, 0.0)
        ctx.set_aux_outputs(depth, acc)
        ctx.set_disp_output(disp)
        ctx.render_numpy()
        centre = [m.numpy().copy() for m in maps]
        for m in maps:
            m.upload(np.full(n, -9.0, f32))
        ctx.set_pixel_offset(0.25, -0.125)
        flagged, _ = check_adaptive(ctx, frames, 2, THRESHOLD)      # the centre frame is at (0, 0) whatever offset is in force
        assert flagged.any()
        assert ctx.pixel_offset == (0.25, -0.125)
        assert ctx._aux_in_force == (depth, acc) and ctx._disp_in_force is disp
        for m, c, name in zip(maps, centre, ("depth", "acc", "disp")):      # the maps describe the centre frame whole
            assert np.array_equal(bits(m.numpy()), bits(c)), name
        for m in maps:      # and they are installed again: the next render fills them, at the offset in force
            m.upload(np.full(n, -9.0, f32))
        ctx.render_numpy()
        assert all(not np.any(m.numpy() == f32(-9.0)) for m in maps)
        assert not np.array_equal(bits(depth.numpy()), bits(centre[0]))
    finally:
        ctx.set_pixel_offset(0.0, 0.0)
        ctx.set_aux_outputs(None, None)
        ctx.set_disp_output(None)
        for m in maps:
            m.free()


def test_a_context_the_masked_render_refuses_raises_its_message(model):
    z, sc, d = model
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), sampling="fp16") as r:
        r.set_camera(z["pose"], z["rot"])
        r.set_pixel_offset(0.125, 0.25)
        with pytest.raises(R.AdaNeRFError, match="adanerf_render_masked: sampling modes fp16 and fp32 have no ray list"):
            r.render_supersampled_adaptive(2, 0.0)
        assert r.pixel_offset == (0.125, 0.25)
        _, _, _, n, _ = r.render_supersampled_adaptive(2, 1.0)      # nothing flagged: no masked pass, nothing to refuse
        assert n == 0


def test_cli_supersample_contrast_writes_the_library_frame(model):
    from test_gpu_antialias import _bmp, _cli_rotation
    z, sc, d = model
    exe = adanerf_amd.build.build_cli()
    try:
        out = subprocess.run([exe, d, "-s", str(W), str(H), "--supersample", "2", "--supersample-contrast", str(THRESHOLD), "-w", "--frames", "1", "--log-camera"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H)) as r:
            r.set_camera(np.asarray(r.info.view_cell_center, np.float32), _cli_rotation(-80.0, 0.0))
            _, rgba, _, n_refined, _ = r.render_supersampled_adaptive(2, THRESHOLD)
            _, plain, _ = r.render_numpy()
            plain = plain.copy()
            _, full, _ = r.render_supersampled(2)
        shown = _bmp(os.path.join(d, "out.bmp"), W, H)
        assert np.array_equal(shown, rgba[:, :3].reshape(H, W, 3)) and len(np.unique(rgba[:, :3])) > 16
        assert 0 < n_refined < W * H
        assert not np.array_equal(rgba, plain) and not np.array_equal(rgba, full)      # neither of the two frames it is made of
        logged = [l.split() for l in out.stdout.splitlines() if l.startswith("adaptive supersample ")]
        assert len(logged) == 1 and [int(logged[0][4]), int(logged[0][6])] == [n_refined, W * H]
        out = subprocess.run([exe, d, "-s", str(W), str(H), "--supersample", "2", "--supersample-contrast", "0.3", "--sampling", "fp16", "--frames", "1"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and "adanerf_render_masked: sampling modes fp16 and fp32 have no ray list" in out.stdout + out.stderr
    finally:
        if os.path.exists(os.path.join(d, "out.bmp")):
            os.remove(os.path.join(d, "out.bmp"))


def test_evaluator_supersample_contrast(model, tmp_path):
    """evaluate(..., supersample=2, supersample_contrast=0.3) on a two-image dataset directory: every image is
    render_supersampled_adaptive(2, 0.3) of its pose, and mean_refined_fraction is the mean of the masks' flagged fractions"""
    from adanerf_amd.evaluate import evaluate, psnr_from_mse
    from adanerf_amd.png import read_png, write_png
    z, sc, md = model
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[W, H], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    pose0, rot0 = np.asarray(z["pose"], f32).reshape(3), np.asarray(z["rot"], f32).reshape(3, 3)
    poses = [(pose0, rot0), (pose0 + f32([0.05, 0.02, 0.0]), rot0)]
    frames, gts = [], []
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        gts.append(np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
        write_png(str(ds / "test" / ("%05d.png" % i)), gts[-1])
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    summary, recs = evaluate(md, str(ds), "test", str(tmp_path / "pred"), precision="bf16", quiet=True, supersample=2, supersample_contrast=THRESHOLD)
    full, frecs = evaluate(md, str(ds), "test", None, precision="bf16", quiet=True, supersample=2)
    assert sorted(summary) == sorted(list(full) + ["mean_refined_fraction"]) and "refined_fraction" not in frecs[0]
    fractions = []
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(md, W, H)) as r:
        for i, fr in enumerate(frames):
            m = np.asarray(fr["transform_matrix"], np.float32)
            r.set_camera(m[:3, 3], m[:3, :3])
            rgb, rgba, mask, n_refined, st = r.render_supersampled_adaptive(2, THRESHOLD)
            fractions.append(float(np.count_nonzero(mask == 0)) / float(W * H))
            assert recs[i]["refined_fraction"] == fractions[-1] == n_refined / float(W * H)
            assert np.array_equal(read_png(str(tmp_path / "pred" / ("%05d.png" % i))), rgba[:, :3].reshape(H, W, 3))
            ref = gts[i].astype(np.float32).reshape(-1, 3) / 255.0
            mse = float(np.mean((rgb.astype(np.float64) - ref) ** 2))
            assert recs[i]["mse"] == mse and recs[i]["psnr"] == psnr_from_mse(mse) and recs[i]["supersample"] == 2
    assert summary["mean_refined_fraction"] == float(np.mean(fractions)) and 0.0 < summary["mean_refined_fraction"] < 1.0
