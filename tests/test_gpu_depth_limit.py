"""Hybrid rendering on the GPU (adanerf_set_depth_limit / adanerf_compact_depth_limit / adanerf_blend_behind).  A ray under a limit must
carry exactly the selection its context made, without the entries at or behind the limit, so every comparison in this file is exact
(bytes / bits): against the numpy rule of tests/depth_limit_reference.py for the stage entry, the trim of whole frames and the blend,
against the library's own stage entry points for what the trimmed arrays composite to.  Frame: 97 x 61 = 5 917 rays, no multiple of 32,
64 or 256; fixture classroom_n8_thr02.  Run with `pytest -m gpu` on an MI355X box."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import budget_reference as B
import depth_limit_reference as D
import mask_reference as MR
import stage_reference as S
from conftest import case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R
from adanerf_amd import sharding

pytestmark = pytest.mark.gpu

W, H = 97, 61
NR = W * H
F32 = np.float32
EINVAL, EUNSUPPORTED = -1, -4
CANARY = 64      # elements behind every output
INF, NAN = F32(np.inf), F32(np.nan)


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    out = {}
    for name in ("classroom_n8_thr02", "classroom_pdf_n8", "classroom_coarse_fine_16_24", "ndc_synthetic_n8"):
        z, meta, sc = load_case(name)
        d = str(tmp_path_factory.mktemp("limit_" + name))
        O.write_model_dir(d, sc, case_weights(meta))
        out[name] = (z, d)
    return out


@pytest.fixture(scope="module")
def ztab(models):
    """the context's depth table: the bin centres do not depend on N"""
    return S.host_depth_table(R.load_library(), R._Options, models["classroom_n8_thr02"][1], 8, 0.2)


def up(a):
    with np.errstate(invalid="ignore"):
        return np.nextafter(a, INF).astype(F32)


def down(a):
    with np.errstate(invalid="ignore"):
        return np.nextafter(a, -INF).astype(F32)


# ---- 1. the stage entry against the rule ---------------------------------------------------------------------------------------------

N_RAYS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000)
POS1 = np.array([0.5, -2.0, 1.25], F32)
ROT1 = O.camera_rotation(35.0, 10.0)
_REF = {}


def stage_case(n_max, ztab):
    """(oracle rows [1000, 128], rays [1000, 8], limits [1000], the expected trimmed selection), made once per n_max and shared by both
    selection kernels; ray r's expectation does not depend on the other rays, so a batch of n rays is the first n rows of everything.
    Ray kinds by r % 7, limit kinds by r % 11 (coprime: every pair occurs); rays 128..255 are plain rays behind a -inf limit, so whole
    segments of 32 and of 64 rows come out empty."""
    if n_max in _REF:
        return _REF[n_max]
    Rm = N_RAYS[-1]
    rng = np.random.default_rng(500 + n_max)
    thr = 0.25
    orc = rng.uniform(-0.5, 1.5, (Rm, 128)).astype(F32)
    cnt, bins, wts = O.select_adaptive(orc, n_max, thr)
    fwd = -ROT1[:, 2].astype(np.float64)
    rays = np.zeros((Rm, 8), F32)
    rays[:, 0:3] = POS1 + rng.uniform(-0.3, 0.3, (Rm, 3)).astype(F32)
    side = rng.normal(size=(Rm, 3))
    side -= (side @ fwd)[:, None] * fwd[None, :]      # across the viewing axis: the sign of d . fwd is the ray kind's
    kind = np.arange(Rm) % 7
    kind[128:256] = 0
    sign = np.where(kind == 1, -1.0, 1.0)      # kind 1: a direction pointing away from the camera, zc falls along the row
    rays[:, 4:7] = (sign[:, None] * fwd[None, :] * rng.uniform(0.5, 1.5, (Rm, 1)) + 0.4 * side).astype(F32)
    rays[kind == 2, 1] = NAN                   # a NaN ray record: every zc is NaN, every entry stays
    rays[kind == 3, 5] = NAN
    rays[kind == 4, 4:7] = 0.0                 # no direction: every entry of the row has the same zc
    rays[kind == 5, 0] = INF                   # an infinite origin: zc is an infinity or a NaN
    zc = D.sample_zc(rays, ztab, bins, POS1, ROT1)
    j = np.arange(Rm) % np.maximum(cnt, 1)
    own = zc[np.arange(Rm), j]                 # the zc of one entry of the ray's own row
    lk = np.arange(Rm) % 11
    lk[128:256] = 5
    with np.errstate(invalid="ignore"):      # a row without a finite zc: inf - inf, a NaN limit
        mid = (0.5 * (zc.min(axis=1, initial=np.inf, where=np.isfinite(zc)) + zc.max(axis=1, initial=-np.inf, where=np.isfinite(zc)))).astype(F32)
    limit = np.select([lk == 0, lk == 1, lk == 2, lk == 3, lk == 4, lk == 5, lk == 6, lk == 7, lk == 8, lk == 9],
                      [own, up(own), down(own), NAN, INF, -INF, F32(-1.5), F32(0.0), mid, F32(1e30)], default=own).astype(F32)
    exp = D.trim(cnt, bins, wts, zc, limit)
    # every branch does occur
    e_cnt = exp[0]
    plain = (kind == 0) | (kind == 6)
    assert (np.diff(ztab) > 0).all() and (limit[128:256] == -INF).all()
    assert (e_cnt[128:256] == 0).all() and (e_cnt[plain & (lk == 3)] == cnt[plain & (lk == 3)]).all()
    assert (e_cnt[np.isin(kind, (2, 3))] == cnt[np.isin(kind, (2, 3))]).all()                       # NaN zc: kept, even behind -inf
    if n_max > 1:
        assert ((e_cnt > 0) & (e_cnt < cnt)).any() and (e_cnt == cnt).any()
        away = (kind == 1) & (e_cnt > 0) & (e_cnt < cnt)
        assert away.any() and (exp[1][away, 0] != bins[away, 0]).any()                              # survivors that are not a prefix of the row
        eq = plain & (lk == 0) & (cnt > 1)
        assert (e_cnt[eq] == j[eq]).all() and (D.trim(cnt, bins, wts, zc, up(own))[0][eq] == j[eq] + 1).all()      # equality drops, one ulp above keeps
    _REF[n_max] = (orc, thr, rays, limit, exp)
    return _REF[n_max]


@pytest.fixture(scope="module")
def stage_ctx(models):
    z, d = models["classroom_n8_thr02"]
    ctxs = {}
    for wave in (False, True):
        ctxs[wave] = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 8), wave_select=wave)
        ctxs[wave].init()
    yield ctxs
    for r in ctxs.values():
        r.close()


@pytest.mark.parametrize("wave_select", [False, True], ids=["pair", "wave"])
@pytest.mark.parametrize("n_max", [1, 4, 8, 16, 32])
def test_compact_depth_limit_against_the_rule(stage_ctx, ztab, n_max, wave_select):
    r = stage_ctx[wave_select]
    Rm = N_RAYS[-1]
    orc, thr, rays, limit, (e_cnt, e_bins, e_w) = stage_case(n_max, ztab)
    d_orc, d_rays, d_lim = r.empty((Rm, 128), F32).upload(orc), r.empty((Rm, 8), F32).upload(rays), r.empty((Rm,), F32).upload(limit)
    cap = Rm * n_max
    outs = [r.empty((Rm + CANARY,), np.int32), r.empty((Rm + CANARY,), np.int32), r.empty((cap + CANARY,), np.uint32),
            r.empty((cap + CANARY,), F32), r.empty((1 + CANARY,), np.int32)]
    fills = [np.full(o.shape, 0x5A5A5A5A, np.uint32).view(o.dtype) for o in outs]
    empty_segments = set()
    for n in N_RAYS:
        for o, f in zip(outs, fills):
            o.upload(f)
        assert r.compact_depth_limit(d_orc, n, n_max, thr, d_rays, d_lim, POS1, ROT1, *outs) == 0, r.lib.adanerf_last_error(r.handle).decode()
        off, cnt, key, sw, tot = [o.numpy() for o in outs]
        x_off, x_key, x_w, x_tot = B.compacted(e_cnt[:n], e_bins[:n], e_w[:n])
        assert cnt[:n].tobytes() == e_cnt[:n].tobytes(), n
        assert off[:n].tobytes() == x_off.tobytes(), n
        assert int(tot[0]) == x_tot, n
        assert key[:x_tot].tobytes() == x_key.tobytes(), n
        assert sw[:x_tot].tobytes() == x_w.tobytes(), n
        for got, fill, used in ((off, fills[0], n), (cnt, fills[1], n), (key, fills[2], x_tot), (sw, fills[3], x_tot), (tot, fills[4], 1)):
            assert got[used:].tobytes() == fill[used:].tobytes(), (n, "canary")
        for seg in (32, 64):
            full = [e_cnt[s:s + seg] for s in range(0, n - seg + 1, seg)]
            if any((c == 0).all() for c in full):
                empty_segments.add(seg)
    assert empty_segments == {32, 64}
    # the entry's own refusals: nothing written
    for o, f in zip(outs, fills):
        o.upload(f)
    assert r.compact_depth_limit(d_orc, 64, n_max, 0.0, d_rays, d_lim, POS1, ROT1, *outs) == EINVAL
    assert r.compact_depth_limit(d_orc, 64, n_max, thr, None, d_lim, POS1, ROT1, *outs) == EINVAL
    assert r.compact_depth_limit(d_orc, 64, n_max, thr, d_rays, None, POS1, ROT1, *outs) == EINVAL
    assert r.compact_depth_limit(d_orc, 64, n_max, thr, d_rays.ptr + 4, d_lim, POS1, ROT1, *outs) == EINVAL
    r.sync()
    assert all(o.numpy().tobytes() == f.tobytes() for o, f in zip(outs, fills))
    for o in outs + [d_orc, d_rays, d_lim]:
        o.free()
        r._own.remove(o)


# ---- whole frames --------------------------------------------------------------------------------------------------------------------

IMAGES = ("rgba", "rgb", "depth", "acc", "disp")


class Ctx:
    """A renderer with every output attached, and a snapshot of all a frame leaves behind."""

    def __init__(self, d, z, n=8, thr=0.2, w=W, h=H, **kw):
        self.r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=kw.pop("batch_size", -1)), num_samples=n, threshold=thr, **kw)
        self.r.init()
        self.pose, self.rot = z["pose"], z["rot"]
        self.r.set_camera(self.pose, self.rot)
        self.attach()

    def attach(self):
        nl = self.r.info.rays_local
        self.aux = [self.r.empty((nl,), F32) for _ in range(3)]
        self.r.set_aux_outputs(self.aux[0], self.aux[1])
        self.r.set_disp_output(self.aux[2])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.r.close()

    def frame(self, buffers=True):
        r = self.r
        for a in self.aux:
            a.upload(np.full(a.shape, -7.0, F32))
        rgb, rgba, st = r.render_numpy()
        self.stats = st
        out = dict(rgba=rgba, rgb=rgb, depth=self.aux[0].numpy(), acc=self.aux[1].numpy(), disp=self.aux[2].numpy(),
                   total_samples=np.int64(st.total_samples))
        if buffers:      # an unbatched frame: the buffers hold all of it
            nl = r.info.rays_local
            assert r.info.batch_rays >= nl
            out.update(counts=r.buffer(R.BUF_RAY_COUNTS, np.int32, (nl,)), offsets=r.buffer(R.BUF_RAY_OFFSETS, np.int32, (nl,)),
                       total=r.buffer(R.BUF_TOTAL, np.int32, (1,)), rays=r.buffer(R.BUF_RAYS, F32, (nl, 8)))
            s = int(out["total"][0])
            out["key"] = r.buffer(R.BUF_SAMPLE_KEY, np.uint32, (s,))
            out["w"] = r.buffer(R.BUF_SAMPLE_W, F32, (s,))
            out["raw"] = r.buffer(R.BUF_RAW, F32, (s, 4))
        return out


def same(a, b, what, keys=None):
    if keys is None:
        assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
        keys = sorted(a)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def rows_of(f, n_max=8):
    """select_adaptive's layout ([R, N] bins -1 padded, values 0 padded, and the sample index of every entry) of a frame's compacted arrays"""
    cnt, off = f["counts"], f["offsets"]
    k = np.arange(n_max)[None, :]
    m = k < cnt[:, None]
    idx = np.where(m, off[:, None] + k, 0)
    bins = np.where(m, (f["key"][idx] & 127).astype(np.int16), -1).astype(np.int16)
    wts = np.where(m, f["w"][idx], F32(0)).astype(F32)
    return bins, wts, idx, m


def frame_limit(f, ztab, pose, rot, n_max=8):
    """The limit of the issue, from the frame itself: ray r with c_r samples gets the zc of its sample number r mod (c_r + 1), the value
    c_r meaning +inf; every fourth ray NaN instead.  Returns (limit, zc, bins, wts, idx)."""
    bins, wts, idx, m = rows_of(f, n_max)
    zc = D.sample_zc(f["rays"], ztab, bins, pose, rot)
    cnt = f["counts"]
    r = np.arange(len(cnt))
    j = r % (cnt + 1)
    limit = np.where(j < cnt, zc[r, np.minimum(j, n_max - 1)], INF).astype(F32)
    limit[r % 4 == 3] = NAN
    return limit, zc, bins, wts, idx


def expected_frame(f, limit, zc, bins, wts, idx):
    """what the limited frame's buffers must hold, and the raw values of the kept samples taken from the unlimited frame"""
    e_cnt, e_bins, e_w = D.trim(f["counts"], bins, wts, zc, limit)
    x_off, x_key, x_w, x_tot = B.compacted(e_cnt, e_bins, e_w)
    valid = np.arange(bins.shape[1])[None, :] < f["counts"][:, None]
    with np.errstate(invalid="ignore"):
        keep = valid & ~(zc >= limit[:, None])
    return dict(counts=e_cnt, offsets=x_off, key=x_key, w=x_w, total=np.array([x_tot], np.int32), raw=f["raw"][idx[keep]])


@pytest.fixture(scope="module")
def plain(models):
    """the unlimited frame, rendered once and left unchanged"""
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z) as c:
        return c.frame()


@pytest.fixture(scope="module")
def limited(models, plain, ztab):
    """(limit, expectation, the limited frame) of the plain frame under frame_limit, rendered once and left unchanged"""
    z, d = models["classroom_n8_thr02"]
    parts = frame_limit(plain, ztab, z["pose"], z["rot"])
    exp = expected_frame(plain, *parts)
    with Ctx(d, z) as c:
        c.r.set_depth_limit(parts[0])
        return parts[0], exp, c.frame()


def test_whole_frame_under_a_limit_made_from_the_frame_itself(models, plain, ztab):
    z, d = models["classroom_n8_thr02"]
    limit, zc, bins, wts, idx = frame_limit(plain, ztab, z["pose"], z["rot"])
    exp = expected_frame(plain, limit, zc, bins, wts, idx)
    # before looking at the device: the three classes of rays all occur
    c0, c1 = plain["counts"], exp["counts"]
    frac = [float(((c1 == 0) & (c0 > 0)).mean()), float((c1 == c0).mean()), float(((c1 > 0) & (c1 < c0)).mean())]
    print("rays that lose everything / nothing / something: %.3f %.3f %.3f" % tuple(frac))
    assert min(frac) >= 0.05, frac
    with Ctx(d, z) as c:
        r = c.r
        r.set_depth_limit(limit)
        got = c.frame()
        for k in ("counts", "offsets", "key", "total", "w"):
            assert got[k].tobytes() == exp[k].tobytes(), k
        # the raw [rgb, alpha] of every kept sample is the unlimited frame's at the same (ray, bin)
        assert got["raw"].tobytes() == exp["raw"].tobytes()
        assert int(got["total_samples"]) == int(exp["total"][0]) == int(c.stats.total_samples)
        # the images are what the library's own compositing gives on the trimmed arrays
        s = int(exp["total"][0])
        dev = [r.to_device(exp["raw"]), r.to_device(exp["w"]), r.to_device(exp["offsets"]), r.to_device(exp["counts"]), r.to_device(exp["key"])]
        o_rgb, o_rgba, o_d, o_a, o_disp = r.empty((NR, 3), F32), r.empty((NR, 4), np.uint8), r.empty((NR,), F32), r.empty((NR,), F32), r.empty((NR,), F32)
        assert s > 0
        r.composite_aux(dev[0], dev[1], dev[2], dev[3], dev[4], NR, o_rgb, o_rgba, o_d, o_a)
        r.disp_map(o_d, o_a, NR, o_disp)
        r.sync()
        for k, o in zip(("rgb", "rgba", "depth", "acc", "disp"), (o_rgb, o_rgba, o_d, o_a, o_disp)):
            assert got[k].tobytes() == o.numpy().tobytes(), k
        # an empty ray: rgb 0, RGBA8 (0, 0, 0, 255), depth 0, acc 0, disp NaN
        e = c1 == 0
        assert e.any() and (got["rgb"][e] == 0).all() and (got["rgba"][e] == np.array([0, 0, 0, 255], np.uint8)).all()
        assert (got["depth"][e] == 0).all() and (got["acc"][e] == 0).all() and np.isnan(got["disp"][e]).all()


def test_identities(models, plain):
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z) as c:
        same(c.frame(), plain, "a fresh context")
        for name, v in (("+inf", INF), ("NaN", NAN)):
            c.r.set_depth_limit(np.full(NR, v, F32))
            same(c.frame(), plain, "all " + name)
        c.r.set_depth_limit(np.full(NR, -INF, F32))
        got = c.frame()
        assert (got["counts"] == 0).all() and int(got["total"][0]) == 0 and int(got["total_samples"]) == 0 and (got["offsets"] == 0).all()
        assert (got["rgb"] == 0).all() and (got["rgba"] == np.array([0, 0, 0, 255], np.uint8)).all()
        assert (got["depth"] == 0).all() and (got["acc"] == 0).all() and np.isnan(got["disp"]).all()
        c.r.set_depth_limit(None)
        same(c.frame(), plain, "installed, then removed")


# ---- 4. composition ------------------------------------------------------------------------------------------------------------------

def test_batches_of_1000_equal_the_unbatched_frame(models, limited):
    z, d = models["classroom_n8_thr02"]
    limit, exp, full = limited
    with Ctx(d, z, batch_size=1000) as c:
        assert c.r.info.batch_rays == 1000
        c.r.set_depth_limit(limit)
        same(c.frame(buffers=False), full, "batch_size 1000", keys=list(IMAGES) + ["total_samples"])


@pytest.mark.parametrize("which", ["checkerboard", "one_pixel"])
def test_render_masked_under_a_limit(models, limited, which):
    z, d = models["classroom_n8_thr02"]
    limit, exp, full = limited
    if which == "checkerboard":
        mask, values = MR.checkerboard(NR, W)
    else:      # one pixel whose row the limit cut in the middle
        p = int(np.flatnonzero((exp["counts"] > 0) & np.isfinite(limit) & (np.arange(NR) > 2000))[0])
        mask, values = np.ones(NR, np.uint8), 1
        mask[p] = 0
    sel = MR.selected(mask, values)
    with Ctx(d, z) as c:
        r = c.r
        r.set_depth_limit(limit)
        fills = dict(rgba=np.full((NR, 4), 0xA5, np.uint8), rgb=np.full((NR, 3), -1234.5, F32), depth=np.full(NR, -77.25, F32),
                     acc=np.full(NR, -3.5, F32), disp=np.full(NR, -9.75, F32))
        d_rgba, d_rgb, d_mask = r.to_device(fills["rgba"]), r.to_device(fills["rgb"]), r.to_device(mask)
        for a, k in zip(c.aux, ("depth", "acc", "disp")):
            a.upload(fills[k])
        m, st = r.render_masked(d_mask, values, d_rgba, d_rgb)
        got = dict(rgba=d_rgba.numpy(), rgb=d_rgb.numpy(), depth=c.aux[0].numpy(), acc=c.aux[1].numpy(), disp=c.aux[2].numpy())
        assert m == int(sel.sum()) and st.total_samples == int(exp["counts"][sel].sum())
        for k in IMAGES:
            assert got[k].tobytes() == MR.expected(fills[k], full[k], mask, values).tobytes(), k


def test_two_strip_shards_equal_the_full_frame(models, limited):
    z, d = models["classroom_n8_thr02"]
    limit, exp, full = limited
    for rank in range(2):
        px = sharding.local_to_pixel(W, H, 4, 2, rank)
        with Ctx(d, z, shard_rank=rank, shard_world=2, strip_rows=4) as c:
            assert c.r.info.rays_local == len(px)
            c.r.set_depth_limit(np.ascontiguousarray(limit[px]))
            got = c.frame()
            for k in IMAGES + ("counts",):
                assert got[k].tobytes() == np.ascontiguousarray(full[k][px]).tobytes(), (rank, k)
            assert int(got["total_samples"]) == int(exp["counts"][px].sum())


def test_budget_map_plus_limit(models, ztab):
    """ray r carries the budget selection at (n_r, thr_r) with the entries at or behind the limit removed: the restatement's trim of
    budget_reference's selection of the frame's own oracle values; the fused path leaves the same frame"""
    z, d = models["classroom_n8_thr02"]
    rng = np.random.default_rng(11)
    n_map = rng.integers(0, 10, NR).astype(np.uint8)
    thr_map = rng.choice(np.array([0.1, 0.2, 0.3, 0.5, np.nan], F32), NR)
    with Ctx(d, z, keep_oracle=True) as c:
        base = c.frame()
        orc = c.r.buffer(R.BUF_ORACLE, F32, (NR, 128))
        b_cnt, b_bins, b_w = B.expected_selection(orc, 8, 0.2, n_map, thr_map)
        zc = D.sample_zc(base["rays"], ztab, b_bins, z["pose"], z["rot"])
        j = np.arange(NR) % (b_cnt + 1)
        limit = np.where(j < b_cnt, zc[np.arange(NR), np.minimum(j, 7)], INF).astype(F32)
        e_cnt, e_bins, e_w = D.trim(b_cnt, b_bins, b_w, zc, limit)
        assert ((e_cnt > 0) & (e_cnt < b_cnt)).any() and (b_cnt < base["counts"]).any()      # both trims do cut
        x_off, x_key, x_w, x_tot = B.compacted(e_cnt, e_bins, e_w)
        c.r.set_budget_map(n_map, thr_map)
        c.r.set_depth_limit(limit)
        got = c.frame()
        assert got["counts"].tobytes() == e_cnt.tobytes() and got["offsets"].tobytes() == x_off.tobytes()
        assert got["key"].tobytes() == x_key.tobytes() and got["w"].tobytes() == x_w.tobytes()
        assert int(got["total_samples"]) == x_tot == int(got["total"][0])
    with Ctx(d, z) as c:
        c.r.set_budget_map(n_map, thr_map)
        c.r.set_depth_limit(limit)
        same(c.frame(), got, "fused against keep_oracle")


GUARD = dict(sampling="guarded", precision="bf16", guard_eps=1e-2, guard_eps_pair=1.5e-2, guard_cache=False)


def test_guarded_context_under_a_limit(models, limited):
    z, d = models["classroom_n8_thr02"]
    limit, exp, full = limited
    with Ctx(d, z, **GUARD) as c:
        c.r.set_depth_limit(limit)
        got = c.frame()
        assert 0 < c.stats.rays_refined < NR and c.stats.guard_audit_mismatch == 0 and c.stats.guard_violations == 0
    with Ctx(d, z, sampling="split", precision="bf16") as s:
        s.r.set_depth_limit(limit)
        want = s.frame()
    for k in ("counts", "offsets", "key", "total"):
        assert got[k].tobytes() == want[k].tobytes() == exp[k].tobytes(), k


def test_pixel_offset_in_force_is_honoured(models, plain, ztab):
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z) as c:
        c.r.set_pixel_offset(0.25, -0.5)
        moved = c.frame()
        assert moved["rays"].tobytes() != plain["rays"].tobytes()
        parts = frame_limit(moved, ztab, z["pose"], z["rot"])
        exp = expected_frame(moved, *parts)      # the limits sit on the zc of the moved rays to the bit
        c.r.set_depth_limit(parts[0])
        got = c.frame()
        for k in ("counts", "offsets", "key", "total", "w", "raw"):
            assert got[k].tobytes() == exp[k].tobytes(), k


# ---- 5. refusals and life cycle -------------------------------------------------------------------------------------------------------

REFUSED = [("dense", "classroom_n8_thr02", dict(num_samples=128, threshold=0.0)), ("pdf", "classroom_pdf_n8", {}),
           ("coarse_fine", "classroom_coarse_fine_16_24", {}), ("ndc", "ndc_synthetic_n8", {})]


@pytest.mark.parametrize("name,case,kw", REFUSED, ids=[u[0] for u in REFUSED])
def test_contexts_without_a_selection_in_camera_space_refuse(models, name, case, kw):
    z, d = models[case]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 32, 24), **kw) as r:
        r.set_camera(z["pose"], z["rot"])
        buf = r.to_device(np.full(r.info.rays_local, -INF, F32))
        rgb0, rgba0, _ = r.render_numpy()
        assert r.lib.adanerf_set_depth_limit(r.handle, buf.ptr) == EUNSUPPORTED, name
        msg = r.lib.adanerf_last_error(r.handle).decode()
        assert "adanerf_set_depth_limit" in msg and len(msg) > 40, msg
        assert r.lib.adanerf_set_depth_limit(r.handle, None) == 0      # nothing to turn off is fine
        rgb1, rgba1, _ = r.render_numpy()
        assert rgba0.tobytes() == rgba1.tobytes() and rgb0.tobytes() == rgb1.tobytes(), name


def test_selection_and_frame_size_under_a_limit(models, limited, plain):
    z, d = models["classroom_n8_thr02"]
    limit, exp, full = limited
    with Ctx(d, z) as c:
        lib, h = c.r.lib, c.r.handle
        c.r.set_depth_limit(limit)
        same(c.frame(), full, "the limited frame")
        assert lib.adanerf_set_selection(h, 128, 0.0) == EUNSUPPORTED and "depth limit" in lib.adanerf_last_error(h).decode()
        same(c.frame(), full, "after the refused threshold 0")
        assert lib.adanerf_set_depth_limit(h, c.r._dl_buf.ptr + 2) == EINVAL      # misaligned: the limit in force stays
        same(c.frame(), full, "after the refused pointer")
        c.r.set_frame_size(W, H)
        same(c.frame(), full, "set_frame_size to the size in force keeps the limit")
        c.r.set_frame_size(64, 40)
        c.attach()
        with Ctx(d, z, w=64, h=40) as e:
            same(c.frame(), e.frame(), "set_frame_size to another ray count removes the limit")
        c.r.set_frame_size(W, H)
        c.attach()
        same(c.frame(), plain, "and back: still no limit")
        c.r.set_depth_limit(limit)
        same(c.frame(), full, "installed again")


# ---- 6. the blend ----------------------------------------------------------------------------------------------------------------------

ACC = np.array([0.0, 1.0, np.nextafter(F32(1), F32(2)), 2.0, -1.0, np.nan, 0.25, np.nextafter(F32(1), F32(0)), -0.0, np.inf, -np.inf, 1e-30], F32)


def blend_case(n):
    rng = np.random.default_rng(n)
    rgb = rng.uniform(-0.2, 1.2, (n, 3)).astype(F32)
    behind = rng.uniform(-0.2, 1.2, (n, 3)).astype(F32)
    acc = ACC[(np.arange(n) + n) % len(ACC)].copy()
    with np.errstate(invalid="ignore"):
        t0 = ~(F32(1) - acc > 0)      # the pixels that copy rgb: a NaN / inf behind them cannot leak
    behind[t0 & (np.arange(n) % 2 == 0)] = NAN
    behind[t0 & (np.arange(n) % 2 == 1)] = INF
    if n > 20:
        rgb[7] = NAN                  # a NaN in the frame itself propagates either way
        behind[19, 1] = NAN           # and one in the behind image where it is let through
        acc[19] = 0.5
    return rgb, acc, behind


@pytest.fixture(scope="module")
def blend_ctx(models):
    z, d = models["classroom_n8_thr02"]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 8)) as r:
        yield r


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_blend_behind_against_the_restatement(blend_ctx, n):
    r = blend_ctx
    rgb, acc, behind = blend_case(n)
    want, want8 = D.blend(rgb, acc, behind)
    with np.errstate(invalid="ignore"):
        copied = ~(F32(1) - acc > 0)
    assert np.array_equal(want[copied].view(np.uint32), rgb[copied].view(np.uint32))
    d_rgb, d_acc, d_beh = r.to_device(rgb), r.to_device(acc), r.to_device(behind)
    fill, fill8 = np.full((n + CANARY, 3), -55.5, F32), np.full((n + CANARY, 4), 0xA5, np.uint8)
    o_rgb, o_8 = r.to_device(fill), r.to_device(fill8)
    r.blend_behind(d_rgb, d_acc, d_beh, n, o_rgb, o_8)
    g, g8 = o_rgb.numpy(), o_8.numpy()
    assert g[:n].tobytes() == want.tobytes() and g8[:n].tobytes() == want8.tobytes()
    assert g[n:].tobytes() == fill[n:].tobytes() and g8[n:].tobytes() == fill8[n:].tobytes()
    # either output alone, and in place
    o_rgb.upload(fill)
    o_8.upload(fill8)
    r.blend_behind(d_rgb, d_acc, d_beh, n, None, o_8)
    assert o_8.numpy()[:n].tobytes() == want8.tobytes() and o_rgb.numpy().tobytes() == fill.tobytes()
    o_8.upload(fill8)
    r.blend_behind(d_rgb, d_acc, d_beh, n, d_rgb, None)
    assert d_rgb.numpy().tobytes() == want.tobytes() and o_8.numpy().tobytes() == fill8.tobytes()
    assert d_acc.numpy().tobytes() == acc.tobytes() and d_beh.numpy().tobytes() == behind.tobytes()
    for a in (d_rgb, d_acc, d_beh, o_rgb, o_8):
        a.free()
        r._own.remove(a)


def test_blend_behind_refusals(blend_ctx):
    r = blend_ctx
    n = 256
    lib, h = r.lib, r.handle
    bufs = {k: r.to_device(np.full((n + CANARY) * m, v, dt)) for k, m, dt, v in
            (("rgb", 3, F32, 1.5), ("acc", 1, F32, 0.5), ("behind", 3, F32, 2.5), ("out", 3, F32, -55.5), ("out8", 1, np.uint32, 0xA5A5A5A5))}
    before = {k: b.numpy() for k, b in bufs.items()}
    p = {k: b.ptr for k, b in bufs.items()}
    call = lambda rgb=p["rgb"], acc=p["acc"], behind=p["behind"], n=n, out=p["out"], out8=p["out8"]: lib.adanerf_blend_behind(h, rgb, acc, behind, n, out, out8)
    bad = [dict(rgb=None), dict(acc=None), dict(behind=None), dict(out=None, out8=None), dict(n=-1), dict(n=0x7fffffff // 3 + 1),
           dict(rgb=p["rgb"] + 2), dict(acc=p["acc"] + 1), dict(behind=p["behind"] + 3), dict(out=p["out"] + 2), dict(out8=p["out8"] + 1),
           dict(out=p["rgb"] + 12),                  # shifted by one pixel: a partial overlap with rgb
           dict(out=p["behind"]), dict(out=p["behind"] + 4 * 3 * (n - 1)), dict(out=p["acc"]),      # an input other than rgb
           dict(out8=p["rgb"]), dict(out8=p["acc"] + 4 * (n - 1)), dict(out8=p["behind"]),
           dict(out=p["out"], out8=p["out"] + 8)]    # the two outputs
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert "adanerf_blend_behind" in lib.adanerf_last_error(h).decode()
    assert lib.adanerf_blend_behind(None, p["rgb"], p["acc"], p["behind"], n, p["out"], p["out8"]) == EINVAL
    r.sync()
    assert all(b.numpy().tobytes() == before[k].tobytes() for k, b in bufs.items())
    assert call(n=0) == 0 and call(n=0, out=None) == 0
    r.sync()
    assert all(b.numpy().tobytes() == before[k].tobytes() for k, b in bufs.items())
    assert call() == 0 and call(out=p["rgb"], out8=None) == 0
    for b in bufs.values():
        b.free()
        r._own.remove(b)


def _occluder(z, plain, ztab):
    """a sphere in the middle of the view, its centre at the median camera-space depth of the plain frame's samples"""
    bins, _, _, m = rows_of(plain)
    dist = float(np.median(D.sample_zc(plain["rays"], ztab, bins, z["pose"], z["rot"])[m]))
    fwd = -np.asarray(z["rot"], np.float64).reshape(3, 3)[:, 2]
    return (np.asarray(z["pose"], np.float64) + dist * fwd).astype(F32), F32(0.35 * dist)


def test_cli_occluder_equals_the_python_host(models, tmp_path):
    """`adanerf --occluder ... --occluder ... --script` written with -w: out.bmp holds a session's last frame, so the session is replayed up
    to a line; each of those frames equals NeuralRenderer.render_hybrid at the logged pose with the per-pixel minimum of sphere_zc over the
    spheres and the nearest sphere's colour behind -- after a turn of the camera and after a `size` token too (the map is filled again)."""
    from test_gpu_set_selection import _bmp_pixels, _cli_rotation
    z, d = models["classroom_n8_thr02"]
    exe = adanerf_amd.build.build_cli()
    lines = ["+w", "b+ 10 10", "m 40 10 -w", "size 64 40"]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="bf16") as r:
        rot0 = _cli_rotation(-80.0, 0.0).astype(np.float64)      # the host starts at the view-cell centre, yaw -80
        centre = np.array(list(r.info.view_cell_center), np.float64)
        spheres = [((centre - 2.0 * rot0[:, 2]).astype(F32), F32(0.6), np.array([0.9, 0.3, 0.1], F32)),
                   ((centre - 1.5 * rot0[:, 2] + 0.5 * rot0[:, 0]).astype(F32), F32(0.4), np.array([0.5, 0.5, 0.5], F32))]      # the default grey
        args = []
        for k, (c, rad, col) in enumerate(spheres):
            args += ["--occluder", ",".join("%.9g" % v for v in list(c) + [rad] + (list(col) if k == 0 else []))]
        w, h = W, H
        shown = []
        for k in (1, 3, 4):
            script = tmp_path / ("session%d.txt" % k)
            script.write_text("\n".join(lines[:k]) + "\n")
            out = subprocess.run([exe, d, "-s", str(W), str(H), "-w", "--script", str(script), "--log-camera"] + args, capture_output=True, text=True,
                                 timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            cam = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
            assert len(cam) == k
            pos, rot = np.array([float(v) for v in cam[-1][3:6]], F32), _cli_rotation(float(cam[-1][7]), float(cam[-1][9]))
            if k == 4:
                w, h = 64, 40
                r.set_frame_size(w, h)
            r.set_camera(pos, rot)
            zcs = np.stack([R.sphere_zc(w, h, r.info.focal, pos, rot, c, rad) for c, rad, _ in spheres])
            near = np.argmin(zcs, axis=0)      # the first given on a tie
            limit = zcs[near, np.arange(w * h)]
            behind = np.where(np.isfinite(limit)[:, None], np.stack([s[2] for s in spheres])[near], F32(0)).astype(F32)
            assert len(np.unique(near[np.isfinite(limit)])) == 2      # both spheres are seen
            _, rgba, _ = r.render_hybrid(limit, behind)
            shown.append(rgba)
            assert np.array_equal(_bmp_pixels(os.path.join(d, "out.bmp"), w, h), rgba[:, :3]), "after line %d (%s)" % (k, lines[k - 1])
        assert not np.array_equal(shown[0], shown[1])                    # the turn does change the frame
        assert not np.array_equal(r.render_numpy()[1], shown[-1])      # and so do the spheres
    os.remove(os.path.join(d, "out.bmp"))
    bad = subprocess.run([exe, d, "--occluder", "1,2,3", "--dry-run"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "cx,cy,cz,r[,R,G,B]" in bad.stdout + bad.stderr


def test_render_hybrid_equals_the_sequence_by_hand(models, plain, ztab):
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z) as c:
        r = c.r
        center, radius = _occluder(z, plain, ztab)
        limit = R.sphere_zc(W, H, r.info.focal, z["pose"], z["rot"], center, radius)
        hit = np.isfinite(limit)
        assert 0.05 < hit.mean() < 0.95
        behind = np.where(hit[:, None], np.array([0.9, 0.3, 0.1], F32), F32(0)).astype(F32)
        # by hand
        r.set_depth_limit(limit)
        by_hand = c.frame()
        d_behind, o_rgb, o_8 = r.to_device(behind), r.empty((NR, 3), F32), r.empty((NR, 4), np.uint8)
        r.blend_behind(r._o_rgb, c.aux[1], d_behind, NR, o_rgb, o_8)
        want, want8 = o_rgb.numpy(), o_8.numpy()
        ref, ref8 = D.blend(by_hand["rgb"], by_hand["acc"], behind)
        assert want.tobytes() == ref.tobytes() and want8.tobytes() == ref8.tobytes()
        assert by_hand["total_samples"] < plain["total_samples"] and (by_hand["counts"][~hit] == plain["counts"][~hit]).all()
        r.set_depth_limit(None)
        # the host's one call; the limit (none) and the aux outputs in force come back
        rgb, rgba, st = r.render_hybrid(limit, behind)
        assert rgb.tobytes() == want.tobytes() and rgba.tobytes() == want8.tobytes() and st.total_samples == by_hand["total_samples"]
        same(c.frame(), plain, "after render_hybrid")
        # with a limit of the caller's in force: that one comes back
        r.set_depth_limit(np.full(NR, -INF, F32))
        rgb2, rgba2, _ = r.render_hybrid(limit, behind)
        assert rgb2.tobytes() == want.tobytes() and rgba2.tobytes() == want8.tobytes()
        assert int(c.frame()["total_samples"]) == 0
