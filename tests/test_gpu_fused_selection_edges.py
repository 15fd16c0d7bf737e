"""The fused selection (pair_epilogue / pair_select of k_select_pair.hip.hpp, inlined into sample_mlp16x3_kernel, sample_mlp16_kernel,
sample_mlp16x2_kernel and sample_mlp16x3_gen_kernel) on the rows continuous networks never produce: ties at the cut, the arg-max fallback,
values equal to the threshold, repeated maxima and non-finite rows, mixed with ordinary rays inside one wave.  The networks are exact by
construction (tests/tie_networks.py; their CPU side is tests/test_tie_networks_cpu.py): on a saturated ray the raw row is known in advance,
bit for bit, in every engine.  Nothing here is a tolerance; every comparison is equality, the only numbers are the class floors
(tie_networks.FLOORS, conditions) and the saturation margin 0.25 (derived in tie_networks.py).

 a. engines are exact on exact data: the raw rows of adanerf_sample_mlp (split, fp16, fp32) equal the prediction bit for bit on the rays
    that are saturated by the device's own adanerf_ray_features                                        test_engines_exact_on_exact_data
 b. the fused selection, the pair launch (keep_oracle) and the wave launch (wave_select) give, on saturated rays, O.select_adaptive +
    O.compact of the predicted rows; on all rays the rule applied to the engine's own stage rows; and each other's bytes, the image
    included -- over a walk of (N, thr) on the live contexts, with the class floors asserted on the device's rows
                                                                                test_walk_on_the_live_context, test_frame_above_a_full_round
 c. segment totals: offsets at every 32-ray segment and the total follow from the counts, at batch sizes -1, 1000, 37        test_batch_sizes
 d. guarded mode: the split engine's counts, offsets and keys; its kept values and its pixels on every re-evaluated and every saturated
    ray (an unrefined ray keeps the fp16 engine's values by contract and is composited with them: inside the band there); every tie ray re-evaluated, no violation, no audit
    mismatch                                                                                                              test_guarded_mode
 e. adanerf_render_masked (split and guarded contexts) with a mask whose edge cuts through tie blocks                  test_masked_rendering
 f. the overflow gate: non-finite rows under split / fp16, selected as the rule reads them; the counter; refined when guarded
                                                                                                                     test_overflow_models
 g. every output buffer a test owns sits between 4 KiB canaries (Guarded of test_gpu_mlp_engines.py).

Plain-fp16 sampling runs with $ADANERF_DEBUG_GUARD = 2 (the 8-wave kernel) and = 4 (the two-block kernel); run-time-shaped networks have
no plain-fp16 engine (sampling="fp16" runs the split kernel) and no guarded mode (it is the split engine alone)."""
import math

import numpy as np
import pytest

import adanerf_oracle as O
import tie_networks as T
from conftest import load_case, record
from test_gpu_mlp_engines import Guarded

import adanerf_amd
from adanerf_amd import renderer as R

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
FORMS = {"fused": {}, "keep_oracle": dict(keep_oracle=True), "wave_select": dict(wave_select=True)}
# engine id: (sampling mode, $ADANERF_DEBUG_GUARD or None)
ENGINES = {"split": ("split", None), "fp16_8wave": ("fp16", "2"), "fp16_2block": ("fp16", "4"), "fp16": ("fp16", None)}
SHORT_WALK = [(16, 0.125, "equal"), (3, 0.5, "equal"), (5, 0.5625, "between"), (1, 4.0, "above")]      # a subset of T.WALK, one pair of every kind


def engines_of(name):
    return ["split", "fp16_8wave", "fp16_2block"] if name.startswith("fixed") else ["split", "fp16"]


MODEL_ENGINES = [(m, e) for m in T.PLAIN for e in engines_of(m)]
IDS = ["%s-%s" % me for me in MODEL_ENGINES]


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def base_case():
    return load_case("synthetic_fixed8")


@pytest.fixture(scope="module")
def models(base_case, tmp_path_factory):
    """name -> (scene, weights, gates, model directory), built once"""
    cache = {}

    def get(name):
        if name not in cache:
            sc, wts, gates, feat = T.build(name, base_case)
            d = str(tmp_path_factory.mktemp("tie_" + name))
            O.write_model_dir(d, sc, wts)
            cache[name] = (sc, wts, gates, d)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def compute_units(models):
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(models("fixed_10_4")[3], 8, 8), precision="fp32") as r:
        return int(r.info.compute_units)


def big_frame(cu):
    """(w, h) just above one full round of the 8-wave kernel's grid (8 waves x 32 rays per workgroup, one workgroup per compute unit): the
    smallest w x h >= 8 * 32 * cu + 97 that is no multiple of 32, h between half the square root and the square root (65 636 rays on 256
    compute units, three more than asked for).  A frame of one row of pixels would hold the ray count exactly, but no gate edge crosses its
    rows: the classes come in runs of thousands of rays and hardly a wave mixes them."""
    n = 8 * 32 * cu + 97
    s = math.isqrt(n)
    return min((-(-n // h) * h, -(-n // h), h) for h in range(s // 2, s + 1) if (-(-n // h) * h) % 32)[1:]


@pytest.fixture(scope="module")
def stage(models, base_case):
    """(model, sampling mode, w, h) -> (saturated [n] from the device's own features, predicted rows [n, 128] fp32 (NaN where not saturated),
    the engine's stage-call rows [n, 128] fp32, features); computed once, never modified"""
    z = base_case[0]
    cache = {}

    def get(name, mode, w, h):
        key = (name, mode, w, h)
        if key not in cache:
            sc, wts, gates, d = models(name)
            n = w * h
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h), precision="bf16", sampling=mode) as r:
                r.set_camera(z["pose"], z["rot"])
                assert r.info.n_in0 == sc.n_in0
                out = Guarded(r, n * 512)
                r.sample_mlp(0, n, out.ptr, None)
                r.sync()
                rows = out.body("stage rows %s %s" % (name, mode)).view(np.float32).reshape(n, 128).copy()
                out.free()
                fb = Guarded(r, n * sc.n_in0 * 4)
                r.ray_features(0, n, fb.ptr, None)
                r.sync()
                feat = fb.body("features %s" % name).view(np.float32).reshape(n, sc.n_in0).copy()
                fb.free()
            sat, pred = T.predict(feat, gates, engine16=mode != "fp32")
            for a in (rows, feat, sat):
                a.setflags(write=False)
            pred = pred.astype(np.float32)
            pred.setflags(write=False)
            cache[key] = (sat, pred, rows, feat)
        return cache[key]
    return get


def rule(rows, n, thr, first=0):
    """O.select_adaptive + O.compact of rows[first:] in the layout of the device's buffers (ray ids local to the batch, as the keys hold them)"""
    cnt, bins, w = O.select_adaptive(rows[first:], n, thr)
    off, ray, b, sw = O.compact(cnt, bins, w)
    return dict(counts=cnt.astype(np.int32), offsets=off.astype(np.int32), total=np.array([cnt.sum()], np.int32),
                key=(ray.astype(np.uint32) << 7) | b.astype(np.uint32), w=sw.astype(np.float32))


def per_ray(f, n_max):
    """the compacted buffers of a one-batch frame back as [rays, n_max] bins (-1 padded) and values (0 padded)"""
    cnt, off = f["counts"], f["offsets"].astype(np.int64)
    m = np.arange(n_max)[None, :] < cnt[:, None]
    idx = np.where(m, off[:, None] + np.arange(n_max)[None, :], 0)
    return cnt, np.where(m, (f["key"][idx] & 127).astype(np.int16), -1), np.where(m, f["w"][idx], np.float32(0))


def same(a, b, what, keys=("counts", "offsets", "total", "key", "w")):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def segments_follow_from_counts(f, what):
    """c: the offset of every ray is the sum of the counts in front of it -- at every 32-ray segment start that is the sum of the segment
    totals in front -- and the total is the sum of all"""
    cnt, off = f["counts"].astype(np.int64), f["offsets"].astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(cnt)])
    seg = np.arange(0, cnt.size, 32)
    assert np.array_equal(off[seg], csum[seg]), what + ": a segment's base is not the sum of the segment totals in front of it"
    assert np.array_equal(off, csum[:-1]), what + ": offsets inside a segment"
    assert int(f["total"][0]) == int(csum[-1]) == f["key"].size, what + ": total"


class Live:
    """a context with canaried image outputs, and everything a frame leaves behind"""

    def __init__(self, d, z, w, h, n, thr, bs=-1, **kw):
        self.r = adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, w, h, batch_size=bs), precision="bf16", num_samples=n, threshold=thr, **kw)
        self.r.init()
        self.r.set_camera(z["pose"], z["rot"])
        self.n = w * h
        self.rgba, self.rgb = Guarded(self.r, self.n * 4), Guarded(self.r, self.n * 12)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.r.close()

    def frame(self):
        r = self.r
        self.rgba.reset()
        self.rgb.reset()
        st = r.render(self.rgba.ptr, self.rgb.ptr, stats=True)
        info = r.refresh_info()
        nb = info.batch_rays
        last = self.n - ((self.n - 1) // nb) * nb      # the buffers hold the frame's last batch
        tot = r.buffer(R.BUF_TOTAL, np.int32, (1,))
        f = dict(rgba=self.rgba.body("rgba8").copy(), rgb=self.rgb.body("rgb").copy(), counts=r.buffer(R.BUF_RAY_COUNTS, np.int32, (last,)),
                 offsets=r.buffer(R.BUF_RAY_OFFSETS, np.int32, (last,)), total=tot, key=r.buffer(R.BUF_SAMPLE_KEY, np.uint32, (int(tot[0]),)),
                 w=r.buffer(R.BUF_SAMPLE_W, np.float32, (int(tot[0]),)))
        assert st.total_samples >= int(tot[0]) and st.rays == self.n
        return f, st, last


def open_forms(d, z, w, h, n, thr, mode, **kw):
    return {k: Live(d, z, w, h, n, thr, sampling=mode, **dict(kw, **f)) for k, f in FORMS.items()}


def check_pair(ctxs, sat, pred, rows, n, thr, what, keep_rows=True):
    """b for one (N, thr) on live one-batch contexts of the three forms; returns the fused frame"""
    want = rule(rows, n, thr)
    sel = O.select_adaptive(pred[sat], n, thr)
    got = {}
    for form, c in ctxs.items():
        info = c.r.set_selection(n, thr)
        assert (info.num_samples, info.threshold, info.dense) == (n, np.float32(thr), 0)
        f, st, last = c.frame()
        assert last == c.n
        got[form] = f
        tag = "%s %s" % (what, form)
        same(f, want, tag + " against the rule on the engine's stage rows")
        cnt, bins, w = per_ray(f, n)
        assert np.array_equal(cnt[sat], sel[0]), tag + ": counts on saturated rays against the predicted rows"
        assert np.array_equal(bins[sat], sel[1]), tag + ": kept bins on saturated rays against the predicted rows"
        assert w[sat].tobytes() == sel[2].tobytes(), tag + ": kept values on saturated rays against the predicted rows"
        segments_follow_from_counts(f, tag)
        if form == "keep_oracle" and keep_rows:
            assert c.r.buffer(R.BUF_ORACLE, np.float32, (c.n, 128)).tobytes() == rows.tobytes(), tag + ": the kept oracle buffer"
    for form in ("keep_oracle", "wave_select"):
        same(got["fused"], got[form], "%s fused against %s" % (what, form), keys=("counts", "offsets", "total", "key", "w", "rgba", "rgb"))
    return got["fused"]


# ---- a ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(T.MODELS))
def test_engines_exact_on_exact_data(name, models, stage, compute_units):
    sc, wts, gates, d = models(name)
    overflow = T.MODELS[name]["overflow"]
    for w, h in [(W, H)] + ([] if overflow else [big_frame(compute_units)]):
        for mode in ("split", "fp16", "fp32"):
            sat, pred, rows, feat = stage(name, mode, w, h)
            over = T.overflow_open(feat, gates) & sat if mode != "fp32" else np.zeros_like(sat)
            ok = sat & ~over
            small = (w, h) == (W, H)      # the frame the gates were placed for: the floors of tests/test_tie_networks_cpu.py hold on the device too
            assert not small or ok.mean() >= (0.3 if overflow else T.FLOORS["saturated"]), (name, mode, ok.mean())
            bad = np.flatnonzero((rows[ok].view(np.uint32) != pred[ok].view(np.uint32)).any(axis=1))
            record("fused_selection_edges_engine", model=name, mode=mode, rays=int(w * h), saturated=int(sat.sum()), overflow_open=int(over.sum()),
                   rows_differ=int(bad.size), distinct_rows=int(len(np.unique(pred[ok], axis=0))))
            assert bad.size == 0, "%s %s %dx%d: %d saturated rays differ from the predicted row, first %s" % (name, mode, w, h, bad.size, np.flatnonzero(ok)[bad[:8]])
            assert not small or len(np.unique(pred[ok], axis=0)) >= T.FLOORS["distinct"]
            assert not np.isfinite(rows[over]).all(axis=1).any(), (name, mode, "a ray behind the open overflow gate is finite")
            if mode == "fp32" or not overflow:
                assert np.isfinite(rows).all(), (name, mode)
            assert (rows[:, gates["bins"]:] == T.ABSENT).all()


# ---- b, c ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,engine", MODEL_ENGINES, ids=IDS)
def test_walk_on_the_live_context(name, engine, models, stage, base_case, monkeypatch):
    sc, wts, gates, d = models(name)
    mode, dbg = ENGINES[engine]
    if dbg:
        monkeypatch.setenv("ADANERF_DEBUG_GUARD", dbg)
    sat, pred, rows, feat = stage(name, mode, W, H)
    assert sat.mean() >= T.FLOORS["saturated"]
    reached = {}
    ctxs = open_forms(d, base_case[0], W, H, 8, 0.125, mode)
    try:
        for n, thr, kind in T.WALK:
            reached[n, thr, kind] = c = T.class_counts(rows, sat, n, thr)
            record("fused_selection_edges_classes", model=name, engine=engine, rays=W * H, n=n, thr=thr, kind=kind, saturated=int(sat.sum()), **c)
            f = check_pair(ctxs, sat, pred, rows, n, thr, "%s %s (%d, %g)" % (name, engine, n, thr))
            assert f["counts"].max() <= n and f["counts"].min() >= 1
            if kind == "above":
                assert (f["counts"] == 1).all()
        T.check_floors(reached, "%s %s on the device's rows" % (name, engine))      # classes that drained away fail here
    finally:
        for c in ctxs.values():
            c.r.close()


@pytest.mark.parametrize("name,engine", MODEL_ENGINES, ids=IDS)
def test_frame_above_a_full_round(name, engine, models, stage, base_case, compute_units, monkeypatch):
    sc, wts, gates, d = models(name)
    mode, dbg = ENGINES[engine]
    if dbg:
        monkeypatch.setenv("ADANERF_DEBUG_GUARD", dbg)
    w, h = big_frame(compute_units)
    sat, pred, rows, feat = stage(name, mode, w, h)
    ctxs = open_forms(d, base_case[0], w, h, 8, 0.125, mode)
    try:
        for n, thr, kind in SHORT_WALK:
            c = T.class_counts(rows, sat, n, thr)
            record("fused_selection_edges_classes", model=name, engine=engine, rays=w * h, n=n, thr=thr, kind=kind, saturated=int(sat.sum()), **c)
            # the same field of view as the 97 x 61 frame the gates were placed for: the classes must be there in numbers, in mixed blocks
            cls, blocks = (c["max_tie"], c["max_tie_blocks"]) if kind == "above" else (c["tie"], c["tie_blocks"])
            assert cls >= T.FLOORS["tie"] and blocks >= T.FLOORS["tie_blocks"], (name, engine, n, thr, c)
            check_pair(ctxs, sat, pred, rows, n, thr, "%s %s %d rays (%d, %g)" % (name, engine, w * h, n, thr), keep_rows=(n == 16))
    finally:
        for c in ctxs.values():
            c.r.close()


@pytest.mark.parametrize("name,engine", MODEL_ENGINES, ids=IDS)
def test_batch_sizes(name, engine, models, stage, base_case, monkeypatch):
    sc, wts, gates, d = models(name)
    mode, dbg = ENGINES[engine]
    if dbg:
        monkeypatch.setenv("ADANERF_DEBUG_GUARD", dbg)
    sat, pred, rows, feat = stage(name, mode, W, H)
    n_rays = W * H
    whole = {}
    for bs in (-1, 1000, 37):
        ctxs = open_forms(d, base_case[0], W, H, 8, 0.125, mode, bs=bs)
        try:
            for n, thr, kind in SHORT_WALK[:3]:
                want_total = int(O.select_adaptive(rows, n, thr)[0].sum())
                for form, c in ctxs.items():
                    c.r.set_selection(n, thr)
                    f, st, last = c.frame()
                    tag = "%s %s batch %d %s (%d, %g)" % (name, engine, bs, form, n, thr)
                    assert last == (n_rays if bs < 0 else n_rays - ((n_rays - 1) // bs) * bs) and st.batches == -(-n_rays // (n_rays if bs < 0 else bs))
                    same(f, rule(rows, n, thr, first=n_rays - last), tag + " last batch against the rule on the stage rows")
                    segments_follow_from_counts(f, tag)
                    assert st.total_samples == want_total, tag
                    if (n, thr) not in whole:
                        whole[n, thr] = f
                    same(f, whole[n, thr], tag + " against the one-batch fused frame", keys=("rgba", "rgb"))
        finally:
            for c in ctxs.values():
                c.r.close()


# ---- d ------------------------------------------------------------------------------------------------------------------------------------

def guard_band(name, gates):
    """A bound on |plain-fp16 row - split row| for these networks, from the formats alone: the fp16 engine rounds the gate's input (|x| <= 1:
    half an ulp is at most 2^-12) before the factor K = 64, then the activation a in [0, 1) that matters to relu(1 - a) (2^-11 covers the
    binade below 2) and the gate value s in [0, 1] once per following layer (2^-12 each); the last layer sums |w_g| of them.  The split
    engine's own error (2^-22 relative per operand) and fp32 accumulation are covered by the 1e-4."""
    per_gate = T.K * 2.0 ** -12 + 2.0 ** -11 + T.MODELS[name]["depth"] * 2.0 ** -12
    return float(per_gate * np.abs(gates["w_last"]).sum(axis=1).max() + 1e-4)


@pytest.mark.parametrize("name", ["fixed_10_4", "fixed_2_2", "fixed_10_4_overflow"])
def test_guarded_mode(name, models, stage, base_case):
    sc, wts, gates, d = models(name)
    z = base_case[0]
    eps = guard_band(name, gates)
    assert eps < 1.0 / 16      # half the spacing of the row values: decided rays exist
    sat, pred, rows16, feat = stage(name, "fp16", W, H)
    rows = stage(name, "split", W, H)[2]
    kw = dict(guard_eps=eps, guard_cache=False)
    with Live(d, z, W, H, 8, 0.125, sampling="guarded", **kw) as g, Live(d, z, W, H, 8, 0.125, sampling="split") as s:
        for n, thr, kind in SHORT_WALK + [(11, 0.5, "equal"), (4, 0.125, "equal")]:
            tag = "%s guarded (%d, %g)" % (name, n, thr)
            g.r.set_selection(n, thr)
            s.r.set_selection(n, thr)
            fg, stg, _ = g.frame()
            fs, sts, _ = s.frame()
            same(fg, fs, tag + " against the split engine", keys=("counts", "offsets", "total", "key"))
            same(fs, rule(rows, n, thr), tag + ": the split engine against the rule on its stage rows")
            und = O.guard_undecided(rows16, n, thr, eps)
            # the kept values (include/adanerf_hip.h, ADANERF_SAMPLING_GUARDED: "unrefined rays hold the fp16 engine's values"): the split
            # engine's bits on every re-evaluated ray and on every saturated ray (both engines are exact there), inside the band elsewhere
            wg, ws = per_ray(fg, n)[2], per_ray(fs, n)[2]
            exact = und | sat
            assert wg[exact].tobytes() == ws[exact].tobytes(), tag + ": kept values on the re-evaluated and the saturated rays"
            assert (np.abs(wg[~exact].astype(np.float64) - ws[~exact]) <= eps).all(), tag + ": a kept value of an unrefined ray outside the band"
            # the image is composited with the kept values: the split engine's bytes wherever the values are its bits
            for k, b in (("rgba", 4), ("rgb", 12)):
                assert fg[k].reshape(-1, b)[exact].tobytes() == fs[k].reshape(-1, b)[exact].tobytes(), tag + ": %s on the re-evaluated and the saturated rays" % k
            record("fused_selection_edges_guarded_frame", model=name, n=n, thr=thr, exact_rays=int(exact.sum()),
                   pixels_differ=int((fg["rgba"].reshape(-1, 4) != fs["rgba"].reshape(-1, 4)).any(axis=1).sum()))
            c16 = T.classes(rows16, n, thr)
            ties = c16["tie"] | c16["max_tie"]
            assert ties.mean() >= (0.0 if T.MODELS[name]["overflow"] else T.FLOORS["tie"]) and ties.any(), tag + ": no tie rays"
            assert not (ties & ~und).any(), tag + ": a tie ray the guard's rule calls decided"
            assert not (c16["nonfinite"] & ~und).any(), tag + ": a non-finite ray the guard's rule calls decided"
            record("fused_selection_edges_guarded", model=name, n=n, thr=thr, rays_refined=int(stg.rays_refined), undecided=int(und.sum()), ties=int(ties.sum()),
                   guard_max_seen=float(stg.guard_max_seen), guard_eps=eps, violations=int(stg.guard_violations), audited=int(stg.guard_audited),
                   audit_mismatch=int(stg.guard_audit_mismatch))
            assert stg.rays_refined >= int(und.sum()), (tag, stg.rays_refined, int(und.sum()))
            assert stg.guard_violations == 0 and stg.guard_widened == 0, (tag, stg.guard_violations, stg.guard_max_seen, eps)
            assert stg.guard_audit_mismatch == 0, tag
            assert sts.rays_refined == 0


# ---- e ------------------------------------------------------------------------------------------------------------------------------------

# adanerf_render_masked exists for the 8 x 256 network in the split and the guarded mode only (its engine is the split kernel over the ray list
# in both: run-time-shaped networks and the fp16 / fp32 modes are refused, ADANERF_EUNSUPPORTED); a guarded
# context's masked pixels are therefore the SPLIT engine's full frame, which a second context renders
@pytest.mark.parametrize("name,engine", [(m, e) for m in T.PLAIN if m.startswith("fixed") for e in ("split", "guarded")], ids=lambda v: v)
def test_masked_rendering(name, engine, models, stage, base_case):
    sc, wts, gates, d = models(name)
    sat, pred, rows, feat = stage(name, "split", W, H)
    n_rays = W * H
    y, x = np.divmod(np.arange(n_rays), W)
    mask = np.where((x + 3 * y) % 29 < 13, 0, 255).astype(np.uint8)      # slanted stripes, 13 of 29 pixels wide: edges inside every 32-ray segment
    inside = mask == 0
    kw = dict(sampling="guarded", guard_eps=guard_band(name, gates), guard_cache=False) if engine == "guarded" else dict(sampling="split")
    with Live(d, base_case[0], W, H, 8, 0.125, **kw) as c, Live(d, base_case[0], W, H, 8, 0.125, sampling="split") as ref:
        d_mask = c.r.to_device(mask)
        for n, thr, kind in SHORT_WALK:
            cls = T.classes(rows, n, thr)
            tie = (cls["max_tie"] if kind == "above" else cls["tie"]) & sat
            pad = np.zeros(-(-n_rays // 32) * 32, bool)
            a, b = pad.copy(), pad.copy()
            a[:n_rays], b[:n_rays] = tie & inside, tie & ~inside
            cut = int((a.reshape(-1, 32).any(axis=1) & b.reshape(-1, 32).any(axis=1)).sum())
            assert cut >= T.FLOORS["tie_blocks"], (name, n, thr, cut)      # the mask's edge does cut through tie blocks
            c.r.set_selection(n, thr)
            ref.r.set_selection(n, thr)
            full, st, _ = ref.frame()
            c.frame()      # the masked call comes after a full frame of its own context, as a host issues it
            c.rgba.reset()
            c.rgb.reset()
            m, stm = c.r.render_masked(d_mask, 1, c.rgba.ptr, c.rgb.ptr)
            c.r.sync()
            tag = "%s %s masked (%d, %g)" % (name, engine, n, thr)
            assert m == int(inside.sum()) and stm.rays == m
            assert stm.total_samples == int(full["counts"][inside].sum()), tag
            for nm, g, k in (("rgba", c.rgba, 4), ("rgb", c.rgb, 12)):
                got = g.body(tag + " " + nm).reshape(n_rays, k)
                assert got[inside].tobytes() == full[nm].reshape(n_rays, k)[inside].tobytes(), tag + ": %s on the masked pixels" % nm
                assert (got[~inside] == 0xA5).all(), tag + ": %s outside the mask" % nm
            assert np.array_equal(d_mask.numpy(), mask)


# ---- f ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,engine", [("fixed_10_4_overflow", "split"), ("fixed_10_4_overflow", "fp16_8wave"), ("fixed_10_4_overflow", "fp16_2block"),
                                         ("gen_6x128_overflow", "split")], ids=lambda v: v)
def test_overflow_models(name, engine, models, stage, base_case, monkeypatch):
    sc, wts, gates, d = models(name)
    z = base_case[0]
    mode, dbg = ENGINES[engine]
    if dbg:
        monkeypatch.setenv("ADANERF_DEBUG_GUARD", dbg)
    sat, pred, rows, feat = stage(name, mode, W, H)
    over = T.overflow_open(feat, gates) & sat
    bad = ~np.isfinite(rows).all(axis=1)
    assert over.mean() >= T.FLOORS["tie"] and T.mixed_blocks(over) >= T.FLOORS["tie_blocks"] and not (over & ~bad).any()
    assert np.isfinite(stage(name, "fp32", W, H)[2]).all()
    ok = sat & ~over
    ctxs = open_forms(d, z, W, H, 8, 0.125, mode)
    try:
        for n, thr, kind in SHORT_WALK + [(11, 0.5, "equal")]:
            tag = "%s %s (%d, %g)" % (name, engine, n, thr)
            record("fused_selection_edges_classes", model=name, engine=engine, rays=W * H, n=n, thr=thr, kind=kind, saturated=int(sat.sum()),
                   **T.class_counts(rows, ok, n, thr))
            f = check_pair(ctxs, ok, pred, rows, n, thr, tag)      # the rule on the stage rows, NaN and all; the three forms' bytes
            cnt, bins, w = per_ray(f, n)
            allnan = np.isnan(rows).all(axis=1)
            assert (cnt[allnan] == 1).all() and (bins[allnan, 0] == 0).all() and np.isnan(w[allnan, 0]).all(), tag + ": an all-NaN row keeps bin 0"
            kept_nan = np.isnan(w) & (np.arange(n)[None, :] < cnt[:, None])
            assert not kept_nan[~allnan].any(), tag + ": a NaN ranked"
    finally:
        for c in ctxs.values():
            c.r.close()
    # the counter, on the first frame of fresh contexts (it runs since create); guarded: every such ray is re-evaluated
    for form, kw in FORMS.items():
        with Live(d, z, W, H, 8, 0.125, sampling=mode, **kw) as c:
            f, st, _ = c.frame()
            assert st.sampling_overflow == int(bad.sum()), (name, engine, form, st.sampling_overflow, int(bad.sum()))
    if name.startswith("fixed") and mode == "fp16":
        with Live(d, z, W, H, 8, 0.125, sampling="guarded", guard_eps=guard_band(name, gates), guard_cache=False) as c:
            f, st, _ = c.frame()
            assert st.rays_refined >= int(bad.sum()) and st.guard_audit_mismatch == 0
            same(f, rule(stage(name, "split", W, H)[2], 8, 0.125), "%s %s guarded against the split engine's stage rows" % (name, engine),
                 keys=("counts", "offsets", "total", "key"))
