"""Per-ray sample budgets on the GPU (adanerf_set_budget_map / adanerf_foveate / adanerf_compact_budget).  Ray r under a map must carry
exactly the selection a context with (n_r, thr_r) makes for it, so every comparison in this file is exact (bytes / bits): against the
numpy rule of tests/budget_reference.py for the stage entry and the ring fill, against contexts set to a uniform pair for whole frames.
Frame: 97 x 61 = 5 917 rays, no multiple of 32, 64 or 256.  Run with `pytest -m gpu` on an MI355X box."""
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import budget_reference as B
from conftest import GOLD, case_weights, load_case

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

W, H = 97, 61
F32 = np.float32
EINVAL, EUNSUPPORTED = -1, -4
CANARY = 64      # elements behind every output


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    out = {}
    for name in ("classroom_n8_thr02", "classroom_pdf_n8", "classroom_coarse_fine_16_24"):
        z, meta, sc = load_case(name)
        d = str(tmp_path_factory.mktemp("budget_" + name))
        O.write_model_dir(d, sc, case_weights(meta))
        out[name] = (z, d)
    return out


# ---- 1. the stage entry against the reference rule ----------------------------------------------------------------------------------

N_RAYS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000)
KINDS = ("uniform", "quantised", "edge", "nan", "single")
VARIANTS = ("both", "n_only", "thr_only", "none")
_REF = {}


def stage_case(kind, n_max, variant):
    """(oracle rows [1000, 128], thr, n_map, thr_map, expected selection), made once per case and shared by both selection kernels; ray r's
    expectation does not depend on the other rays, so a batch of n rays is the first n rows of everything"""
    key = (kind, n_max, variant)
    if key in _REF:
        return _REF[key]
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n_max)
    R_ = N_RAYS[-1]
    thr = 0.25
    if kind == "uniform":
        orc = rng.uniform(-0.5, 1.5, (R_, 128)).astype(F32)
    elif kind == "quantised":      # multiples of 0.25: ties at every cut, the context's threshold and the per-ray ones included
        orc = (np.round(rng.uniform(-0.5, 1.5, (R_, 128)) * 4) / 4).astype(F32)
    elif kind == "edge":
        z = np.load(os.path.join(GOLD, "selection_edge_cases.npz"))
        k = "n%d" % n_max
        orc = np.tile(z[k + "_orc"], (2, 1))[:R_].astype(F32)
        thr = float(z[k + "_thr"])
    elif kind == "nan":
        orc = np.full((R_, 128), np.nan, F32)
    else:      # one number in a row of NaN: the arg-max whatever the thresholds
        orc = np.full((R_, 128), np.nan, F32)
        orc[np.arange(R_), rng.integers(0, 128, R_)] = rng.uniform(-0.5, 1.5, R_).astype(F32)
    vr = np.random.default_rng(77 + n_max)
    n_map = vr.integers(0, n_max + 4, R_).astype(np.uint8) if variant in ("both", "n_only") else None
    choices = np.array([0.5 * thr, thr, thr + 0.25, 1e3, np.inf, np.nan], F32)      # below, equal, above, above every value, +inf, NaN
    thr_map = vr.choice(choices, R_) if variant in ("both", "thr_only") else None
    _REF[key] = (orc, thr, n_map, thr_map, B.expected_selection(orc, n_max, thr, n_map, thr_map))
    return _REF[key]


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
def test_compact_budget_against_the_reference_rule(stage_ctx, n_max, wave_select):
    r = stage_ctx[wave_select]
    Rm = N_RAYS[-1]
    d_orc = r.empty((Rm, 128), F32)
    d_n, d_t = r.empty((Rm,), np.uint8), r.empty((Rm,), F32)
    cap = Rm * n_max
    # canaries: every output is filled with a pattern before every call, and everything behind what the call may write must still hold it
    outs = [r.empty((Rm + CANARY,), np.int32), r.empty((Rm + CANARY,), np.int32), r.empty((cap + CANARY,), np.uint32),
            r.empty((cap + CANARY,), F32), r.empty((1 + CANARY,), np.int32)]
    fills = [np.full(o.shape, 0x5A5A5A5A, np.uint32).view(o.dtype) for o in outs]
    for kind in KINDS:
        for variant in VARIANTS:
            orc, thr, n_map, thr_map, (e_cnt, e_bins, e_w) = stage_case(kind, n_max, variant)
            d_orc.upload(orc)
            if n_map is not None:
                d_n.upload(n_map)
            if thr_map is not None:
                d_t.upload(thr_map)
            for n in N_RAYS:
                for o, f in zip(outs, fills):
                    o.upload(f)
                r.compact_budget(d_orc, n, n_max, thr, d_n if n_map is not None else None, d_t if thr_map is not None else None, *outs)
                off, cnt, key, sw, tot = [o.numpy() for o in outs]
                x_off, x_key, x_w, x_tot = B.compacted(e_cnt[:n], e_bins[:n], e_w[:n])
                tag = (kind, variant, n)
                assert cnt[:n].tobytes() == e_cnt[:n].tobytes(), tag
                assert off[:n].tobytes() == x_off.tobytes(), tag
                assert int(tot[0]) == x_tot, tag
                assert key[:x_tot].tobytes() == x_key.tobytes(), tag
                assert sw[:x_tot].tobytes() == x_w.tobytes(), tag
                for got, fill, used in ((off, fills[0], n), (cnt, fills[1], n), (key, fills[2], x_tot), (sw, fills[3], x_tot), (tot, fills[4], 1)):
                    assert got[used:].tobytes() == fill[used:].tobytes(), (tag, "canary")
    for o in outs + [d_orc, d_n, d_t]:
        o.free()
        r._own.remove(o)


# ---- whole frames -------------------------------------------------------------------------------------------------------------------

class Ctx:
    """A renderer with every output attached, and a snapshot of all a frame leaves behind."""

    def __init__(self, d, z, n, thr, w=W, h=H, **kw):
        self.r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=kw.pop("batch_size", -1)), num_samples=n, threshold=thr, **kw)
        self.r.init()
        self.r.set_camera(z["pose"], z["rot"])
        self.attach()

    def attach(self):
        nl = self.r.info.rays_local
        self.aux = [self.r.empty((nl,), F32) for _ in range(2)]
        self.r.set_aux_outputs(self.aux[0], self.aux[1])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.r.close()

    def frame(self):
        r = self.r
        for a in self.aux:
            a.upload(np.full(a.shape, -7.0, F32))
        rgb, rgba, st = r.render_numpy()
        info = r.refresh_info()
        nl, nb = info.rays_local, info.batch_rays
        last = nl - ((nl - 1) // nb) * nb if nl else 0      # the buffers hold the frame's last batch
        out = dict(rgba=rgba, rgb=rgb, depth=self.aux[0].numpy(), acc=self.aux[1].numpy(),
                   counts=r.buffer(R.BUF_RAY_COUNTS, np.int32, (last,)), offsets=r.buffer(R.BUF_RAY_OFFSETS, np.int32, (last,)),
                   total=r.buffer(R.BUF_TOTAL, np.int32, (1,)), total_samples=np.int64(st.total_samples))
        s = int(out["total"][0])
        out["key"] = r.buffer(R.BUF_SAMPLE_KEY, np.uint32, (s,))
        out["w"] = r.buffer(R.BUF_SAMPLE_W, F32, (s,))
        self.refined = int(st.rays_refined)
        self.info_bytes = bytes(info)
        return out

    def uniform_map(self, n, thr):
        nl = self.r.info.rays_local
        self.r.set_budget_map(np.full(nl, n, np.uint8), np.full(nl, thr, F32))


def same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def fresh(d, z, n, thr, **kw):
    with Ctx(d, z, n, thr, **kw) as c:
        return c.frame()


PATHS = {"fused": {}, "wave_select": dict(wave_select=True), "keep_oracle": dict(keep_oracle=True), "batch_1000": dict(batch_size=1000),
         "shard_1_of_3": dict(shard_rank=1, shard_world=3, strip_rows=4), "fp32_shading": dict(precision="fp32")}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_a_uniform_map_is_set_selection(models, path):
    """(8, 0.2) under a map of all (4, 0.3) leaves what a context set to (4, 0.3) leaves -- frames, aux maps, counts, offsets, keys, weights,
    totals; a map of all (0, 0) and NULL after a map both give the no-map frame."""
    z, d = models["classroom_n8_thr02"]
    kw = PATHS[path]
    with Ctx(d, z, 8, 0.2, **kw) as c:
        plain = c.frame()
        c.uniform_map(4, 0.3)
        got = c.frame()
        same(got, fresh(d, z, 4, 0.3, **kw), path + ": all (4, 0.3)")
        assert got["counts"].max() <= 4 and got["total_samples"] < plain["total_samples"]
        c.uniform_map(0, 0.0)
        same(c.frame(), plain, path + ": all (0, 0)")
        c.uniform_map(4, 0.3)
        c.frame()
        c.r.set_budget_map(None, None)
        same(c.frame(), plain, path + ": NULL after a map")
        # one half of the pair at a time: the other follows the context
        c.r.set_budget_map(np.full(c.r.info.rays_local, 4, np.uint8), None)
        same(c.frame(), fresh(d, z, 4, 0.2, **kw), path + ": N only")
        c.r.set_budget_map(None, np.full(c.r.info.rays_local, 0.3, F32))
        same(c.frame(), fresh(d, z, 8, 0.3, **kw), path + ": threshold only")


def test_two_zones(models):
    """left half (2, thr), right half (N, thr): every pixel is the same pixel of the matching uniform frame"""
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z, 8, 0.2) as c:
        full = c.frame()
        left = (np.arange(W * H) % W) < W // 2
        c.r.set_budget_map(np.where(left, 2, 8).astype(np.uint8), np.full(W * H, 0.2, F32))
        got = c.frame()
    low = fresh(d, z, 2, 0.2)
    for k in ("rgba", "rgb", "depth", "acc", "counts"):
        assert got[k][left].tobytes() == low[k][left].tobytes(), k + ": left half"
        assert got[k][~left].tobytes() == full[k][~left].tobytes(), k + ": right half"
    assert (low["counts"][left] < full["counts"][left]).any()      # the zones do differ
    assert got["total_samples"] == low["counts"][left].sum() + full["counts"][~left].sum()


# ---- 4. the ring fill ----------------------------------------------------------------------------------------------------------------

RINGS3 = [(6, 8, 0.2), (20, 4, 0.3), (45, 2, 0.35), (1, 0.5)]
FOVEA_CASES = {
    "centre": ((W / 2, H / 2), RINGS3),
    "off_image_left": ((-20.25, 10.0), RINGS3),
    "far_outside": ((500.0, -300.5), RINGS3),
    "zero_rings": ((10.0, 10.0), [(3, 0.4)]),
    "ring_wider_than_the_image": ((48.5, 30.5), [(5, 8, 0.2), (400, 5, 0.25), (2, 0.5)]),
    "eight_rings": ((30.75, 40.25), [(2 + 5 * k, 8 - k, 0.2 + 0.05 * k) for k in range(8)] + [(0, 0.9)]),
    "radius_zero_and_ties_to_even": ((0.25, 0.75), [(0, 7, 0.2), (1, 6, 0.3), (3, 0.4)]),
}


@pytest.mark.parametrize("shard", [None, 0, 1, 2])
def test_foveate_against_the_numpy_fill(models, shard):
    z, d = models["classroom_n8_thr02"]
    kw = {} if shard is None else dict(shard_rank=shard, shard_world=3, strip_rows=4)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), **kw) as r:
        nl = r.info.rays_local
        d_n, d_t = r.empty((nl + CANARY,), np.uint8), r.empty((nl + CANARY,), F32)
        for name, (gaze, rings) in FOVEA_CASES.items():
            d_n.upload(np.full(nl + CANARY, 0xA5, np.uint8))
            d_t.upload(np.full(nl + CANARY, -7.0, F32))
            assert r.foveate_device(gaze, rings, d_n, d_t) == 0, name
            want_n, want_t = B.ring_fill(W, H, gaze, rings, **({} if shard is None else dict(strip_rows=4, world=3, rank=shard)))
            got_n, got_t = d_n.numpy(), d_t.numpy()
            assert got_n[:nl].tobytes() == want_n.tobytes() and got_t[:nl].tobytes() == want_t.tobytes(), name
            assert (got_n[nl:] == 0xA5).all() and (got_t[nl:] == F32(-7.0)).all(), name + ": canary"
        assert len(np.unique(B.ring_fill(W, H, *FOVEA_CASES["centre"])[0])) == 4      # the cases do exercise the rings
        # either output alone
        d_n.upload(np.full(nl + CANARY, 0xA5, np.uint8))
        d_t.upload(np.full(nl + CANARY, -7.0, F32))
        assert r.foveate_device((W / 2, H / 2), RINGS3, d_n, None) == 0 and r.foveate_device((1.0, 2.0), RINGS3, None, None) == 0
        assert (d_t.numpy() == F32(-7.0)).all() and d_n.numpy()[:nl].tobytes() == B.ring_fill(W, H, (W / 2, H / 2), RINGS3, **(
            {} if shard is None else dict(strip_rows=4, world=3, rank=shard)))[0].tobytes()
        # every refusal leaves the buffers as they were
        d_n.upload(np.full(nl + CANARY, 0xA5, np.uint8))
        bad = [((float("nan"), 1.0), RINGS3), ((1.0, float("inf")), RINGS3), ((1.0, 1.0), [(k + 1, 8, 0.2) for k in range(9)] + [(1, 0.5)]),
               ((1.0, 1.0), [(5, 8, 0.2), (5, 4, 0.3), (1, 0.5)]), ((1.0, 1.0), [(9, 8, 0.2), (5, 4, 0.3), (1, 0.5)]),
               ((1.0, 1.0), [(-1, 8, 0.2), (1, 0.5)]), ((1.0, 1.0), [(5, 256, 0.2), (1, 0.5)]), ((1.0, 1.0), [(5, 8, 0.2), (-1, 0.5)]),
               ((1.0, 1.0), [(5, 8, float("nan")), (1, 0.5)]), ((1.0, 1.0), [(5, 8, 0.2), (1, float("nan"))])]
        for gaze, rings in bad:
            assert r.foveate_device(gaze, rings, d_n, d_t) == EINVAL, (gaze, rings)
            assert len(r.lib.adanerf_last_error(r.handle).decode()) > 10
        r.sync()
        assert (d_n.numpy() == 0xA5).all() and (d_t.numpy() == F32(-7.0)).all()
        nr = r.lib.adanerf_foveate(r.handle, 1.0, 1.0, -1, None, None, None, d_n.ptr, d_t.ptr)
        assert nr == EINVAL


def test_foveated_frame_is_the_reference_rule_ray_by_ray(models):
    """NeuralRenderer.foveate on a context that keeps its oracle values: the counts and keys of the frame are expected_selection of those
    values under the maps of the numpy fill, and total_samples is their sum."""
    z, d = models["classroom_n8_thr02"]
    gaze, rings = (40.5, 25.0), RINGS3
    with Ctx(d, z, 8, 0.2, keep_oracle=True) as c:
        c.r.foveate(gaze, rings)
        got = c.frame()
        orc = c.r.buffer(R.BUF_ORACLE, F32, (W * H, 128))
        n_map, thr_map = B.ring_fill(W, H, gaze, rings)
        assert c.r.budget_buffers()[0].numpy().tobytes() == n_map.tobytes()
    e_cnt, e_bins, e_w = B.expected_selection(orc, 8, 0.2, n_map, thr_map)
    x_off, x_key, x_w, x_tot = B.compacted(e_cnt, e_bins, e_w)
    assert got["counts"].tobytes() == e_cnt.tobytes() and got["offsets"].tobytes() == x_off.tobytes()
    assert got["key"].tobytes() == x_key.tobytes() and got["w"].tobytes() == x_w.tobytes()
    assert int(got["total_samples"]) == x_tot == int(got["total"][0])
    with Ctx(d, z, 8, 0.2) as c:      # and the fused path leaves the same frame
        c.r.foveate(gaze, RINGS3)
        f = c.frame()
    same({k: v for k, v in f.items()}, got, "fused against keep_oracle")


# ---- 5. lifecycle --------------------------------------------------------------------------------------------------------------------

def test_contexts_without_a_selection_to_trim_refuse(models):
    z, d = models["classroom_n8_thr02"]
    for name, n, thr in (("classroom_n8_thr02", 128, 0.0), ("classroom_pdf_n8", 8, -1.0), ("classroom_coarse_fine_16_24", 0, -1.0)):
        z, d = models[name]
        with Ctx(d, z, n, thr) if name != "classroom_coarse_fine_16_24" else _plain(d, z) as c:
            r = c.r
            buf_n, buf_t = r.empty((r.info.rays_local,), np.uint8), r.empty((r.info.rays_local,), F32)
            rgb0, rgba0, _ = r.render_numpy()
            for a, b in ((buf_n, buf_t), (buf_n, None), (None, buf_t)):
                assert r.lib.adanerf_set_budget_map(r.handle, R._ptr(a), R._ptr(b)) == EUNSUPPORTED, name
                assert len(r.lib.adanerf_last_error(r.handle).decode()) > 10
            assert r.lib.adanerf_set_budget_map(r.handle, None, None) == 0      # nothing to turn off is fine
            rgb1, rgba1, _ = r.render_numpy()
            assert rgba0.tobytes() == rgba1.tobytes() and rgb0.tobytes() == rgb1.tobytes(), name


class _plain:
    def __init__(self, d, z):
        self.r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 32, 24))
        self.r.init()
        self.r.set_camera(z["pose"], z["rot"])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.r.close()


def test_selection_and_frame_size_under_a_map(models):
    z, d = models["classroom_n8_thr02"]
    rng = np.random.default_rng(3)
    with Ctx(d, z, 8, 0.2) as c:
        lib, h = c.r.lib, c.r.handle
        n_map = rng.integers(0, 9, W * H).astype(np.uint8)
        c.r.set_budget_map(n_map, None)
        mapped = c.frame()
        # threshold 0 is refused while the map is installed, and nothing has changed
        assert lib.adanerf_set_selection(h, 128, 0.0) == EUNSUPPORTED and "budget map" in lib.adanerf_last_error(h).decode()
        assert lib.adanerf_set_selection(h, 0, 0.0) == EUNSUPPORTED
        same(c.frame(), mapped, "after the refused threshold 0")
        # the N in force is the cap, evaluated per render
        c.r.set_selection(4, None)
        capped = c.frame()
        assert capped["counts"].max() <= 4
        with Ctx(d, z, 8, 0.2) as e:
            e.r.set_budget_map(np.where((n_map == 0) | (n_map > 4), 4, n_map).astype(np.uint8), None)
            same(capped, e.frame(), "set_selection(4, -1) under a map with entries up to 8")
        c.r.set_selection(8, None)
        same(c.frame(), mapped, "back at N = 8")
        # the same size keeps the map; another rays_local clears it
        c.r.set_frame_size(W, H)
        same(c.frame(), mapped, "set_frame_size to the size in force")
        c.r.set_frame_size(64, 40)
        c.attach()
        same(c.frame(), fresh(d, z, 8, 0.2, w=64, h=40), "set_frame_size to another ray count clears the map")
        c.r.set_frame_size(W, H)
        c.attach()
        same(c.frame(), fresh(d, z, 8, 0.2), "and back: still no map")
        c.r.set_budget_map(n_map, None)
        same(c.frame(), mapped, "installed again")


GUARD = dict(sampling="guarded", precision="bf16", guard_eps=1e-2, guard_eps_pair=1.5e-2, guard_cache=False)


def test_guarded_context_renders_as_split_under_a_map(models):
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z, 8, 0.2, **GUARD) as c:
        a0 = c.frame()
        info0, refined0 = c.info_bytes, c.refined
        assert 0 < refined0 < W * H
        c.uniform_map(4, 0.3)
        got = c.frame()
        assert c.refined == 0 and c.info_bytes == info0
        with Ctx(d, z, 8, 0.2, sampling="split", precision="bf16") as s:
            s.uniform_map(4, 0.3)
            same(got, s.frame(), "guarded under a map against split under the map")
        c.frame()
        assert c.refined == 0
        c.r.set_budget_map(None, None)
        back = c.frame()
        assert c.refined > 0 and c.info_bytes == info0
        # the frames under the map did not move the audit on: this is the second guarded frame of a context that never had a map
        with Ctx(d, z, 8, 0.2, **GUARD) as e:
            same(e.frame(), a0, "first guarded frame")
            same(e.frame(), back, "guarded again after NULL")
            assert e.refined == c.refined


def test_cli_fovea_and_gaze_token_equal_the_python_host(models, tmp_path):
    """`adanerf --fovea SPEC --script` written with -w: out.bmp holds a session's last frame, so the session is replayed up to each of its
    lines in turn; every one of those frames equals what NeuralRenderer.foveate renders at the logged pose -- the gaze at the frame centre
    until a `gaze` token moves it."""
    from test_gpu_set_selection import _bmp_pixels, _cli_rotation
    z, d = models["classroom_n8_thr02"]
    exe = adanerf_amd.build.build_cli()
    spec = "10:8:0.2,30:4:0.3,2:0.4"
    lines = ["+w", "gaze 20.5 15", "-w gaze 90 70.25"]
    gazes = [(W / 2, H / 2), (20.5, 15.0), (90.0, 70.25)]
    frames = []
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="bf16") as r:
        for k in range(1, len(lines) + 1):
            script = tmp_path / ("session%d.txt" % k)
            script.write_text("\n".join(lines[:k]) + "\n")
            out = subprocess.run([exe, d, "-s", str(W), str(H), "-w", "--fovea", spec, "--script", str(script), "--log-camera"], capture_output=True,
                                 text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            cam = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
            assert len(cam) == k
            r.foveate(gazes[k - 1], spec)
            r.set_camera(np.array([float(v) for v in cam[-1][3:6]], F32), _cli_rotation(float(cam[-1][7]), float(cam[-1][9])))
            _, rgba, st = r.render_numpy()
            frames.append(rgba)
            assert np.array_equal(_bmp_pixels(os.path.join(d, "out.bmp"), W, H), rgba[:, :3]), "frame %d (%s)" % (k, lines[k - 1])
        r.set_budget_map(None, None)
        assert not np.array_equal(r.render_numpy()[1], frames[-1])      # the map does change the frame
    os.remove(os.path.join(d, "out.bmp"))
