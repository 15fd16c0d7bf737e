"""The sample cap on the GPU (adanerf_set_sample_cap / adanerf_sample_cap_report / adanerf_compact_cap).  A capped batch must be, byte for
byte, the batch the same context renders with no cap and a threshold map filled with t*, and t* must be the one the brute-force rule of
tests/cap_reference.py finds -- so every comparison in this file is exact (bytes / bits).  Stage-level cases go through
adanerf_compact_cap with caller-made rows, so every value is chosen; frames are 97 x 61 = 5 917 rays of a golden scene, no multiple of
32, 64 or 256.  Run with `pytest -m gpu` on an MI355X box."""
import json
import os
import subprocess

import numpy as np
import pytest

import adanerf_oracle as O
import budget_reference as B
import cap_reference as K
import depth_limit_reference as D
import stage_reference as S
from conftest import case_weights, load_case
from test_gpu_budget_map import GUARD, Ctx, same

import adanerf_amd
from adanerf_amd import renderer as R

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
    for name in ("classroom_n8_thr02", "classroom_pdf_n8", "classroom_coarse_fine_16_24", "classroom_dense128"):
        z, meta, sc = load_case(name)
        d = str(tmp_path_factory.mktemp("cap_" + name))
        O.write_model_dir(d, sc, case_weights(meta))
        out[name] = (z, d)
    return out


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


# ---- 1. the stage entry against the reference rule ------------------------------------------------------------------------------------

class Stage:
    """Device buffers for batches of up to `rays` rays of `n_max` entries; every output lies in front of CANARY elements of 0xA5 bytes."""

    def __init__(self, r, rays, n_max):
        self.r, self.rays, self.n_max = r, rays, n_max
        cap = rays * n_max
        self.d_orc = r.empty((rays, 128), F32)
        self.outs = [r.empty((rays + CANARY,), np.int32), r.empty((rays + CANARY,), np.int32), r.empty((cap + CANARY,), np.uint32),
                     r.empty((cap + CANARY,), F32), r.empty((1 + CANARY,), np.int32), r.empty((1 + CANARY,), F32)]
        self.fills = [np.full(o.shape, 0xA5A5A5A5, np.uint32).view(o.dtype) for o in self.outs]
        self.extra = []

    def device(self, arr):
        a = self.r.empty(arr.shape, arr.dtype).upload(arr)
        self.extra.append(a)
        return a

    def run(self, orc, thr, cap_total, **kw):
        """adanerf_compact_cap on the rows `orc` -> dict of the outputs cut to what the call wrote; the canaries are checked"""
        n = orc.shape[0]
        self.d_orc.upload(np.concatenate([orc, np.zeros((self.rays - n, 128), F32)]))
        for o, f in zip(self.outs, self.fills):
            o.upload(f)
        rc = self.r.compact_cap(self.d_orc, n, self.n_max, thr, cap_total, *self.outs, **kw)
        assert rc == 0, self.r.lib.adanerf_last_error(self.r.handle).decode()
        off, cnt, key, sw, tot, ts = [o.numpy() for o in self.outs]
        t = int(tot[0]) if n else 0
        for got, fill, used in ((off, self.fills[0], n), (cnt, self.fills[1], n), (key, self.fills[2], t), (sw, self.fills[3], t),
                                (tot, self.fills[4], 1 if n else 0), (ts, self.fills[5], 1)):
            assert got[used:].tobytes() == fill[used:].tobytes(), "canary"
        return dict(off=off[:n], cnt=cnt[:n], key=key[:t], w=sw[:t], total=t, tstar=ts[0])

    def plain(self, orc, thr):
        """adanerf_compact on the same rows, into the same buffers"""
        n = orc.shape[0]
        self.d_orc.upload(np.concatenate([orc, np.zeros((self.rays - n, 128), F32)]))
        for o, f in zip(self.outs, self.fills):
            o.upload(f)
        self.r.compact(self.d_orc, n, self.n_max, thr, *self.outs[:5])
        off, cnt, key, sw, tot = [o.numpy() for o in self.outs[:5]]
        t = int(tot[0])
        return dict(off=off[:n], cnt=cnt[:n], key=key[:t], w=sw[:t], total=t)

    def close(self):
        for o in self.outs + [self.d_orc] + self.extra:
            o.free()
            self.r._own.remove(o)


def expect(sel, cap_total):
    """the reference's capped selection as adanerf_compact_cap's outputs"""
    t, c, b, w = K.apply(sel[0], sel[1], sel[2], cap_total)
    off, key, sw, tot = B.compacted(c, b, w)
    return dict(off=off, cnt=c.astype(np.int32), key=key, w=sw, total=tot, tstar=F32(t))


def check(got, exp, tag):
    print("%s: t* %r (expected %r), total %d (expected %d)" % (tag, float(got["tstar"]), float(exp["tstar"]), got["total"], exp["total"]))
    assert F32(got["tstar"]).tobytes() == F32(exp["tstar"]).tobytes(), (tag, "t*", got["tstar"], exp["tstar"])
    assert got["total"] == exp["total"], (tag, "total")
    for k in ("cnt", "off", "key", "w"):
        assert got[k].tobytes() == exp[k].tobytes(), (tag, k)


SIZES = (1, 33, 257, NR)
_REF = {}


def random_ref(n, n_max):
    if (n, n_max) not in _REF:
        orc, n_max, thr, cap = K.random_case(n, n_max)
        _REF[(n, n_max)] = (orc, thr, cap, expect(K.selection(orc, n_max, thr), cap))
    return _REF[(n, n_max)]


@pytest.mark.parametrize("n_max,wave_select", [(8, False), (16, False), (24, False), (8, True)], ids=["n8_thread", "n16_thread", "n24_wave", "n8_wave_select"])
def test_compact_cap_against_the_reference_rule(stage_ctx, n_max, wave_select):
    st = Stage(stage_ctx[wave_select], NR, n_max)
    trimmed = 0
    for n in SIZES:
        orc, thr, cap, exp = random_ref(n, n_max)
        got = st.run(orc, thr, cap)
        check(got, exp, "random n=%d n_max=%d" % (n, n_max))
        assert got["total"] <= cap
        trimmed += exp["tstar"] != -INF
    assert trimmed >= 3
    st.close()


BUILT = K.built_cases()
_BUILT_REF = {}


@pytest.mark.parametrize("name", sorted(BUILT))
def test_rows_built_for_the_places_it_can_go_wrong(stage_ctx, name):
    orc, n_max, thr, cap = BUILT[name]
    if name not in _BUILT_REF:
        _BUILT_REF[name] = expect(K.selection(orc, n_max, thr), cap)
    exp = _BUILT_REF[name]
    for wave in ((False, True) if n_max <= 16 else (False,)):      # the pair and the wave selection: 32- and 64-ray segments
        st = Stage(stage_ctx[wave], orc.shape[0], n_max)
        got = st.run(orc, thr, cap)
        check(got, exp, "%s wave_select=%s" % (name, wave))
        assert got["total"] <= max(cap, 0) or exp["tstar"] == -INF
        again = st.run(orc, thr, cap)      # two calls give the same bytes
        for k in ("cnt", "off", "key", "w"):
            assert again[k].tobytes() == got[k].tobytes(), (name, k, "second call")
        assert F32(again["tstar"]).tobytes() == F32(got["tstar"]).tobytes()
        if exp["tstar"] == -INF:      # C >= T_now: what adanerf_compact writes, and t* = -inf
            base = st.plain(orc, thr)
            for k in ("cnt", "off", "key", "w"):
                assert got[k].tobytes() == base[k].tobytes(), (name, k, "against adanerf_compact")
            assert got["total"] == base["total"]
        st.close()


def test_budget_map_depth_limit_and_cap_together(stage_ctx, models):
    """the three trims in their order, rows emptied by the limit included; against the three references applied in that order"""
    ztab = S.host_depth_table(R.load_library(), R._Options, models["classroom_n8_thr02"][1], 8, 0.2)
    pos, rot = np.array([0.5, -2.0, 1.25], F32), O.camera_rotation(35.0, 10.0)
    for n_max, wave in ((8, False), (8, True), (24, False)):
        n = 1000
        rng = np.random.default_rng(900 + n_max)
        thr = 0.25
        orc = (np.round(rng.uniform(-0.5, 0.35, (n, 128)) * 1024) / 1024).astype(F32)
        n_map = rng.integers(0, n_max + 3, n).astype(np.uint8)
        thr_map = rng.choice(np.array([0.1, 0.25, 0.28, 0.3, np.nan], F32), n)
        cnt, bins, wts = B.expected_selection(orc, n_max, thr, n_map, thr_map)
        fwd = -rot[:, 2].astype(np.float64)
        rays = np.zeros((n, 8), F32)
        rays[:, 0:3] = pos + rng.uniform(-0.3, 0.3, (n, 3)).astype(F32)
        rays[:, 4:7] = (fwd[None, :] * rng.uniform(0.5, 1.5, (n, 1)) + 0.2 * rng.normal(size=(n, 3))).astype(F32)
        zc = D.sample_zc(rays, ztab, bins, pos, rot)
        limit = np.where(np.arange(n) % 5 == 0, -INF, np.where(np.arange(n) % 5 == 1, np.median(zc, axis=1).astype(F32), INF)).astype(F32)
        limit[128:256] = -INF      # whole segments of 32 and of 64 rows come out empty
        cnt2, bins2, wts2 = D.trim(cnt, bins, wts, zc, limit)
        assert (cnt2 == 0).sum() >= 250 and (cnt2 > 1).sum() >= 300
        for frac in (0.6, 1.0):
            cap = max(n, int(frac * cnt2.sum()))
            exp = expect((cnt2, bins2, wts2), cap)
            st = Stage(stage_ctx[wave], n, n_max)
            got = st.run(orc, thr, cap, n_map=st.device(n_map), thr_map=st.device(thr_map), rays=st.device(rays), limit_zc=st.device(limit), pos=pos,
                         rot_c2w=rot)
            check(got, exp, "three trims n_max=%d wave_select=%s C=%d" % (n_max, wave, cap))
            assert (got["cnt"][128:256] == 0).all() and ((exp["tstar"] == -INF) == (frac == 1.0))
            st.close()


def test_compact_cap_refusals(stage_ctx):
    r = stage_ctx[False]
    st = Stage(r, 64, 8)
    orc = K.random_case(64, 8)[0]
    st.d_orc.upload(orc)
    for o, f in zip(st.outs, st.fills):
        o.upload(f)
    assert r.compact_cap(st.d_orc, 64, 8, 0.25, 63, *st.outs) == EINVAL                  # C < n
    assert r.compact_cap(st.d_orc, 64, 8, 0.0, 64, *st.outs) == EINVAL                   # dense
    assert r.compact_cap(st.d_orc, 64, 8, 0.25, 64, *st.outs[:5], None) == EINVAL        # no place for t*
    assert r.compact_cap(st.d_orc, 64, 8, 0.25, 64, *st.outs, limit_zc=st.outs[3]) == EINVAL      # a limit without rays and pose
    r.sync()
    assert all(o.numpy().tobytes() == f.tobytes() for o, f in zip(st.outs, st.fills))
    st.close()


# ---- 2. whole frames ------------------------------------------------------------------------------------------------------------------

CAP = 4.0      # the golden scene selects about 6.6 samples per ray at (8, 0.2)


def report(c):
    rep = c.r.sample_cap_report()
    return dict(threshold_max=F32(rep.threshold_max), batches_trimmed=int(rep.batches_trimmed), selected=int(rep.samples_selected), kept=int(rep.samples_kept))


@pytest.mark.parametrize("path", ["fused", "wave_select", "keep_oracle", "fp32_shading"])
def test_a_capped_frame_is_the_frame_under_a_map_of_its_threshold(models, path):
    """the contract: frame, aux maps, counts, offsets, keys, kept values, totals"""
    z, d = models["classroom_n8_thr02"]
    kw = {"fused": {}, "wave_select": dict(wave_select=True), "keep_oracle": dict(keep_oracle=True), "fp32_shading": dict(precision="fp32")}[path]
    with Ctx(d, z, 8, 0.2, **kw) as c:
        plain = c.frame()
        assert int(plain["total_samples"]) > CAP * NR
        c.r.set_sample_cap(CAP)
        capped = c.frame()
        rep = report(c)
        print("capped frame: %r, total_samples %d of %d, C %d" % (rep, int(capped["total_samples"]), int(plain["total_samples"]), int(CAP * NR)))
        assert rep["batches_trimmed"] == 1 and rep["selected"] == int(plain["total_samples"])
        assert rep["kept"] == int(capped["total_samples"]) == int(capped["total"][0]) <= int(np.floor(CAP * NR))
        assert np.isfinite(rep["threshold_max"]) and rep["threshold_max"] >= F32(0.2)
        same(c.frame(), capped, "a second capped frame")
        # the cap survives a selection and a size that change nothing it depends on
        c.r.set_selection(8, 0.2)
        c.r.set_frame_size(W, H)
        same(c.frame(), capped, "after set_selection / set_frame_size")
        c.r.set_sample_cap(0)
        same(c.frame(), plain, "with the cap removed")
        c.r.set_budget_map(None, np.full(NR, rep["threshold_max"], F32))
        same(c.frame(), capped, "no cap, a threshold map filled with t*")
        c.r.set_budget_map(None, None)
        # a cap that trims nothing, and one at N: the plain frame
        c.r.set_sample_cap(7.99)
        same(c.frame(), plain, "a cap above the frame's mean")
        assert report(c) == dict(threshold_max=-INF, batches_trimmed=0, selected=int(plain["total_samples"]), kept=int(plain["total_samples"]))
        c.r.set_sample_cap(8.0)
        same(c.frame(), plain, "a cap at N")
        assert report(c) == dict(threshold_max=-INF, batches_trimmed=0, selected=0, kept=0)      # nothing launched


def test_without_a_trim_the_selection_is_the_fixture_the_parity_tests_pin(stage_ctx, models):
    """the golden fixture's own oracle values (classroom_n8_thr02; tests/test_gpu_parity.py pins adanerf_compact on them bit for bit): a cap
    that trims nothing leaves sel_count / sel_bins / sel_weight, before and after a call that trims on the same context"""
    z, d = models["classroom_n8_thr02"]
    orc = np.ascontiguousarray(z["oracle_out"], F32)
    n = orc.shape[0]
    fixture = (z["sel_count"].astype(np.int32), z["sel_bins"], z["sel_weight"])
    x_off, x_key, x_w, x_tot = B.compacted(*fixture)
    for wave in (False, True):
        st = Stage(stage_ctx[wave], n, 8)
        for cap in (x_tot, 4 * n, 8 * n):
            got = st.run(orc, 0.2, cap)
            if cap == 4 * n:
                check(got, expect(fixture, cap), "fixture rows under C = 4 n")
                assert got["total"] <= cap < x_tot
                continue
            assert got["tstar"] == -INF and got["total"] == x_tot
            assert got["cnt"].tobytes() == fixture[0].tobytes() and got["off"].tobytes() == x_off.tobytes()
            assert got["key"].tobytes() == x_key.tobytes() and got["w"].tobytes() == x_w.tobytes()
        st.close()


def test_batches_of_ragged_size_are_capped_each_on_its_own_rays(models):
    """-bs 1000: five batches of 1000 rays and one of 917, each with its own t* -- the one adanerf_compact_cap finds on that batch's stage rows"""
    z, d = models["classroom_n8_thr02"]
    bs = 1000
    with Ctx(d, z, 8, 0.2, keep_oracle=True) as whole:      # the stage rows of the frame: the raw outputs are position-invariant per ray
        whole.frame()
        orc = whole.r.buffer(R.BUF_ORACLE, F32, (NR, 128))
        st = Stage(whole.r, bs, 8)
        per_batch = []
        for first in range(0, NR, bs):
            rows = orc[first:first + bs]
            per_batch.append(st.run(rows, 0.2, int(np.floor(np.float64(F32(CAP)) * rows.shape[0]))))
        st.close()
    ts = np.array([b["tstar"] for b in per_batch], F32)
    assert (ts > -INF).sum() >= 2 and len(set(ts.tolist())) >= 2      # the batches do not share one threshold
    with Ctx(d, z, 8, 0.2, batch_size=bs) as c:
        plain = c.frame()
        c.r.set_sample_cap(CAP)
        capped = c.frame()
        rep = report(c)
        last = per_batch[-1]
        assert rep["threshold_max"].tobytes() == ts.max().tobytes() and rep["batches_trimmed"] == int((ts > -INF).sum())
        assert rep["kept"] == sum(b["total"] for b in per_batch) == int(capped["total_samples"]) <= int(np.floor(CAP * NR))
        assert rep["selected"] == int(plain["total_samples"])
        for b, first in zip(per_batch, range(0, NR, bs)):
            assert b["total"] <= int(np.floor(np.float64(F32(CAP)) * len(b["cnt"])))
        assert capped["counts"].tobytes() == last["cnt"].tobytes() and capped["offsets"].tobytes() == last["off"].tobytes()
        assert capped["key"].tobytes() == last["key"].tobytes() and capped["w"].tobytes() == last["w"].tobytes()
        c.r.set_sample_cap(0)
        c.r.set_budget_map(None, np.repeat(ts, bs)[:NR])      # -inf where a batch was not trimmed: the context's threshold
        same(c.frame(), capped, "no cap, every batch under a map of its own t*")


def test_guarded_context_renders_as_split_under_a_cap(models):
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z, 8, 0.2, **GUARD) as c:
        a0 = c.frame()
        info0, refined0 = c.info_bytes, c.refined
        assert 0 < refined0 < NR
        c.r.set_sample_cap(CAP)
        got = c.frame()
        assert c.refined == 0 and c.info_bytes == info0
        with Ctx(d, z, 8, 0.2, sampling="split", precision="bf16") as s:
            s.r.set_sample_cap(CAP)
            same(got, s.frame(), "guarded under a cap against split under the cap")
        c.frame()
        assert c.refined == 0
        c.r.set_sample_cap(0)
        back = c.frame()
        assert c.refined > 0 and c.info_bytes == info0 and c.r.last_stats.guard_violations == 0
        # the frames under the cap did not move the audit on: this is the second guarded frame of a context that never had a cap
        with Ctx(d, z, 8, 0.2, **GUARD) as e:
            same(e.frame(), a0, "first guarded frame")
            same(e.frame(), back, "guarded again after the cap")
            assert e.refined == c.refined


def test_refusals(models):
    z, d = models["classroom_n8_thr02"]
    with Ctx(d, z, 8, 0.2) as c:
        lib, h = c.r.lib, c.r.handle
        plain = c.frame()
        for bad in (0.5, 0.999, -1.0, float("nan"), float("inf"), -float("inf")):
            assert lib.adanerf_set_sample_cap(h, bad) == EINVAL, bad
        same(c.frame(), plain, "after refused caps")
        c.r.set_sample_cap(CAP)
        capped = c.frame()
        assert lib.adanerf_set_sample_cap(h, float("nan")) == EINVAL      # the cap in force stays
        assert lib.adanerf_set_selection(h, 128, 0.0) == EUNSUPPORTED
        mask = c.r.to_device(np.zeros(NR, np.uint8))
        out = c.r.empty((NR, 4), np.uint8)
        stats, m = R.Stats(), R.C.c_int32(0)
        assert lib.adanerf_render_masked(h, mask.ptr, 1, out.ptr, None, R.C.byref(stats), R.C.byref(m)) == EUNSUPPORTED
        assert b"sample cap" in lib.adanerf_last_error(h)
        same(c.frame(), capped, "after the refusals")
        c.r.set_sample_cap(0)
        assert lib.adanerf_render_masked(h, mask.ptr, 1, out.ptr, None, R.C.byref(stats), R.C.byref(m)) == 0 and m.value == NR
    for name in ("classroom_dense128", "classroom_pdf_n8", "classroom_coarse_fine_16_24"):
        z, d = models[name]
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 16, 8)) as r:
            assert r.lib.adanerf_set_sample_cap(r.handle, 4.0) == EUNSUPPORTED, name
            assert r.lib.adanerf_set_sample_cap(r.handle, 0.0) == 0, name


def test_evaluator_sweep_sample_caps(tmp_path):
    """evaluate(..., sweep_sample_caps=[0, 8, half the plain mean, 1]) on a synthetic 12 x 10 dataset: every entry's mean_samples_per_ray is
    at or under its cap, the cap-0 entry is the plain run, and a run without the option keeps its keys"""
    from adanerf_amd.evaluate import evaluate
    from adanerf_amd.png import write_png
    sc = O.Scene((0.783, -3.19, 1.39), (0.7, 0.7, 0.2), (0.1542200982570648, 8.358194804191589), 1.1386263370513916, 8.79825210571289, 8, 0.2)
    md = str(tmp_path / "model")
    O.write_model_dir(md, sc, O.synthetic_weights(0, oracle_bias=0.1, oracle_scale=0.3))
    w, h = 12, 10
    ds = tmp_path / "dataset"
    (ds / "test").mkdir(parents=True)
    json.dump(dict(resolution=[w, h], camera_angle_x=sc.fov, view_cell_center=list(sc.view_cell_center), view_cell_size=list(sc.view_cell_size),
                   flip_depth=False, depth_distance_adjustment=False), open(ds / "dataset_info.json", "w"))
    poses = [(np.array(sc.view_cell_center, F32), O.camera_rotation(100.0, 0.0)),
             (np.array(sc.view_cell_center, F32) + F32([0.1, 0.05, -0.02]), O.camera_rotation(60.0, -8.0))]
    frames = []
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for i, (pose, rot) in enumerate(poses):
        m = np.eye(4, dtype=F32)
        m[:3, :3], m[:3, 3] = rot, pose
        frames.append(dict(file_path="./test/%05d" % i, transform_matrix=m.tolist()))
        write_png(str(ds / "test" / ("%05d.png" % i)), np.stack([(xx * 20 + i * 9) % 256, (yy * 25) % 256, (xx + yy) * 11 % 256], axis=2).astype(np.uint8))
    json.dump(dict(frames=frames), open(ds / "transforms_test.json", "w"))
    plain, precs = evaluate(md, str(ds), "test", None, precision="bf16", quiet=True, metrics=("psnr", "flip"))
    assert sorted(plain) == ["frames", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray"]
    mid = max(1.0, float(np.floor(0.5 * plain["mean_samples_per_ray"] * 4) / 4))
    assert plain["mean_samples_per_ray"] > 2.0      # or the cap in the middle trims nothing
    caps = [0.0, 8.0, mid, 1.0]
    summary, recs = evaluate(md, str(ds), "test", str(tmp_path / "pred"), precision="bf16", quiet=True, metrics=("psnr", "flip"), sweep_sample_caps=caps)
    assert sorted(summary) == ["frames", "sweep"] and [e["sample_cap"] for e in summary["sweep"]] == caps and len(recs) == 2 * len(caps)
    assert sorted(os.listdir(tmp_path / "pred")) == sorted("cap%g" % c for c in caps)
    for e in summary["sweep"]:
        assert sorted(e) == ["mean_cap_threshold", "mean_flip", "mean_ms", "mean_mse", "mean_psnr", "mean_samples_per_ray", "sample_cap"]
        print(e)
        if e["sample_cap"]:
            assert e["mean_samples_per_ray"] <= e["sample_cap"]
    first = summary["sweep"][0]
    assert first["mean_cap_threshold"] is None and first["mean_samples_per_ray"] == plain["mean_samples_per_ray"] and first["mean_mse"] == plain["mean_mse"]
    assert summary["sweep"][1]["mean_cap_threshold"] is None and summary["sweep"][1]["mean_mse"] == plain["mean_mse"]      # a cap at N
    assert summary["sweep"][2]["mean_cap_threshold"] >= 0.2
    assert summary["sweep"][3]["mean_samples_per_ray"] == 1.0      # C = n: one entry per ray
    for x in recs[2 * 2:2 * 3]:
        assert x["sample_cap"] == mid and x["samples_per_ray"] <= mid and (x["cap_threshold"] is None or x["cap_threshold"] >= 0.2)
    with pytest.raises(ValueError):
        evaluate(md, str(ds), "test", None, quiet=True, sweep_sample_caps=[0.5])
    with pytest.raises(ValueError):
        evaluate(md, str(ds), "test", None, quiet=True, sweep_sample_caps=[2.0], sweep_samples=[4])


def test_cli_sample_cap_and_cap_token_equal_the_python_host(models, tmp_path):
    """`adanerf --sample-cap 4 --script` written with -w: out.bmp holds a session's last frame, so the session is replayed up to each of its
    lines in turn; every one of those frames equals what NeuralRenderer.set_sample_cap renders at the logged pose -- cap 4, then `cap 2.5`,
    then `cap 0`"""
    from test_gpu_set_selection import _bmp_pixels, _cli_rotation
    z, d = models["classroom_n8_thr02"]
    exe = adanerf_amd.build.build_cli()
    lines = ["+w", "cap 2.5", "-w cap 0"]
    caps = [4.0, 2.5, 0.0]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="bf16") as r:
        seen = []
        for k in range(1, len(lines) + 1):
            script = tmp_path / ("session%d.txt" % k)
            script.write_text("\n".join(lines[:k]) + "\n")
            out = subprocess.run([exe, d, "-s", str(W), str(H), "-w", "--sample-cap", "4", "--script", str(script), "--log-camera"], capture_output=True,
                                 text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            cam = [l.split() for l in out.stdout.splitlines() if l.startswith("camera ")]
            assert len(cam) == k
            r.set_sample_cap(caps[k - 1])
            r.set_camera(np.array([float(v) for v in cam[-1][3:6]], F32), _cli_rotation(float(cam[-1][7]), float(cam[-1][9])))
            _, rgba, st = r.render_numpy()
            seen.append(st.total_samples)
            assert caps[k - 1] == 0 or st.total_samples <= int(caps[k - 1] * NR)
            assert np.array_equal(_bmp_pixels(os.path.join(d, "out.bmp"), W, H), rgba[:, :3]), "frame %d (%s)" % (k, lines[k - 1])
        assert seen[1] < seen[0] < seen[2]
