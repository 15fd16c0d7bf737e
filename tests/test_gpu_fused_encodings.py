"""The positional encoding every fused MLP kernel computes for itself, read slot by slot through networks whose outputs ARE chosen input
slots (tests/probe_networks.py; its CPU side is tests/test_probe_networks_cpu.py) -- the suite saw these encodings only through trained or
random networks under RMS-type bounds, where a wrong slot order, a lost quarter turn or a sine that fails at large arguments is a few percent
of error.  Frame 97 x 61 (5 917 rays: 47 tiles of 128, the last ragged; no multiple of 32, 64, 256); shading on 2 570 samples of those rays.

Kernels, reached through the stage entries adanerf_sample_mlp / adanerf_shade_mlp, and the form of their encoding:
  sample_mlp_kernel <10, 4 | 2, 2>                      fp32, accurate        test_sampling_slots[fixed_10_4-*], [fixed_2_2-near]  mode fp32
  sample_mlp16x3_kernel <10, 4 | 2, 2>                  split, accurate       the same cases, mode split
  sample_mlp16_kernel <10, 4 | 2, 2>                    fp16, fast            the same cases, mode fp16
  sample_mlp16x2_kernel <10, 4 | 2, 2>                  fp16, fast, no rows   test_two_block_kernel_on_the_probe: fused frames under
                                                                              $ADANERF_DEBUG_GUARD = 4 against the 8-wave kernel's under = 2, on
                                                                              the all-slots probe and on 16-slot probes, plain and negated
  sample_mlp_gen_kernel <10, 4 | 2, 2 | 16, 16, 128>    fp32, accurate        [gen_w128-*], [gen_w128_rsi4-*] (raySampleInput = 4),
                                                                              [gen_w128_2_2-near], [gen_w128_16_1-*], [gen_w128_6_3-near]
  sample_mlp_gen_wide_kernel <10, 4 | 2, 2 | 16, 16>    fp32, pe_eval_wide    [wide_w384-*], [wide_w384_2_2-near], [wide_w384_16_1-*],
                                                                              [wide_w384_6_3-near]
  sample_mlp16x3_gen_kernel <10, 4 | 2, 2 | 16, 16, 128>  split, accurate     [gen_split_w96-*], [gen_split_w96_2_2-near], [gen_w128_2_2-near],
                                                                              [gen_w128_16_1-*], [gen_w128_6_3-near]  mode split
  shade_mlp32_kernel <10, 4>                            fp32, accurate        test_shading_slots[fixed_8x256-*] fp32
  shade_mlp16x2_kernel <Bf16 | Fp16, 10, 4>             fast                  the same cases, bf16 and fp16
  shade_mlp16_gen_staged_kernel <., 10, 4 | 16, 16, W>  fast                  [staged_w96_d5-*] (depth 5, skips 1 and 3), [staged_w96_d5_12_2-far],
                                                                              [staged_w96_d5_1_16-far]; W = 512: [wide_w257_d3-*],
                                                                              [wide_w257_d3_12_2-far], [wide_w257_d3_1_16-far]
  shade_mlp32_gen_kernel / shade_mlp32_gen_wide_kernel  fp32, accurate        the same cases in fp32 (wide: width 257)

Scenes (probe_networks.scene_of; the conditions are asserted on the device's own x, probe_networks.conditions): near -- every argument below
256 revolutions and below 1e5; far -- for each component a camera under which a quarter and more of its top-band arguments lie beyond 256 revolutions,
the documented domain of V_SIN_F32; straddle -- 2^9 p_x crosses 1e5, pe_eval's wave-uniform range test, inside 64-ray waves and 128-ray tiles.  A 2-band or
6-band encoding has no far scene (|x| would have to be 800 / 50); a 12- or 16-band encoding of a unit direction has no near one.

Bounds, none of them from the code under test (probe_networks.check_slots: the output lies between the probe on s - E and on s + E):
  identity slots     E = 0: the bits of x on the fp32 engines, the model's rounding of x elsewhere;
  accurate form      E = 1.2e-7 for |a| < 1e5, 2e-7 beyond: the stated and tested accuracy of sin_or_cos (test_device_sin_or_cos_accuracy),
                     around sin / cos in fp64 of the exact product x 2^b;
  fast form          E = 2^-18 around sin(2 pi r32), r32 the fp32 revolution count the fma hands to v_sin_f32 -- beyond 256 revolutions too.
No ray and no slot is excused.  Per band and engine the share of slots that needed the widening and max |out - sin64(a)| are logged
(profiles/fused_encodings_measured.log).

The figures are filed under the kernel that ran (raySampleInput and widths above 256 run the fp32 kernels whatever mode is asked for).
Every case builds one model directory and one small context per probe (23 to 33 for a shading case); on an MI355X the slowest case takes about a
second and the file about twelve (per case: profiles/fused_encodings_measured.md).

Position invariance: the near probe frame from first_ray = 0, 1, 31, 129 with n = 1, 127, 128, 129, 1 000 has the bits of the whole-frame call."""
import time

import numpy as np
import pytest

import adanerf_oracle as O
import probe_networks as P
from conftest import load_case, record
from test_gpu_fused_selection_edges import Live, rule, same
from test_gpu_mlp_engines import Guarded, run_shade

import adanerf_amd

pytestmark = pytest.mark.gpu

W, H, N_RAYS = P.W, P.H, P.W * P.H
WINDOWS = [(f, n) for f in (0, 1, 31, 129) for n in (1, 127, 128, 129, 1000)]
FIXED3 = [("fp32", "exact", "accurate"), ("split", "split", "accurate"), ("fp16", "fp16", "fast")]
# id: depth, width, posEncArgs[0], raySampleInput, [(sampling mode, rounding model, form of the encoding)], scenes.  Run-time-shaped networks have
# no plain-fp16 engine; raySampleInput and widths above 256 run the fp32 kernels in every mode.
SAMPLING = {
    "fixed_10_4": (8, 256, (10, 4), 0, FIXED3, ("near", "far", "straddle")),
    "fixed_2_2": (8, 256, (2, 2), 0, FIXED3, ("near",)),
    "gen_w128": (4, 128, (10, 4), 0, [("fp32", "exact", "accurate")], ("near", "far", "straddle")),
    "gen_w128_rsi4": (4, 128, (10, 4), 4, [("split", "exact", "accurate")], ("near", "far")),
    "wide_w384": (3, 384, (10, 4), 0, [("split", "exact", "accurate")], ("near", "far", "straddle")),
    "gen_split_w96": (4, 96, (10, 4), 0, [("split", "split", "accurate")], ("near", "far", "straddle")),
    "gen_w128_2_2": (4, 128, (2, 2), 0, [("fp32", "exact", "accurate"), ("split", "split", "accurate")], ("near",)),
    "wide_w384_2_2": (3, 384, (2, 2), 0, [("fp32", "exact", "accurate")], ("near",)),
    "gen_split_w96_2_2": (4, 96, (2, 2), 0, [("split", "split", "accurate")], ("near",)),
    "gen_w128_16_1": (4, 128, (16, 1), 0, [("fp32", "exact", "accurate"), ("split", "split", "accurate")], ("near", "far")),
    "wide_w384_16_1": (3, 384, (16, 1), 0, [("fp32", "exact", "accurate")], ("near", "far")),
    "gen_w128_6_3": (4, 128, (6, 3), 0, [("fp32", "exact", "accurate"), ("split", "split", "accurate")], ("near",)),
    "wide_w384_6_3": (3, 384, (6, 3), 0, [("fp32", "exact", "accurate")], ("near",)),
}
# id: depth, width, skips, posEncArgs[1], scenes; every context runs fp32 (accurate), bf16 and fp16 (fast)
SHADING = {
    "fixed_8x256": (8, 256, [4], (10, 4), ("near", "far", "straddle")),
    "staged_w96_d5": (5, 96, [1, 3], (10, 4), ("near", "far", "straddle")),
    "wide_w257_d3": (3, 257, [1], (10, 4), ("near", "far", "straddle")),
    "staged_w96_d5_12_2": (5, 96, [1, 3], (12, 2), ("far",)),
    "staged_w96_d5_1_16": (5, 96, [1, 3], (1, 16), ("far",)),
    "wide_w257_d3_12_2": (3, 257, [1], (12, 2), ("far",)),
    "wide_w257_d3_1_16": (3, 257, [1], (1, 16), ("far",)),
}
KERNEL_CLASS = {"exact": "fp32", "split": "split", "fp16": "fp16"}      # what the figures are filed under: the kernel that ran, not the mode asked for
SHADE_ENGINES = [("fp32", "exact", "accurate"), ("bf16", "bf16", "fast"), ("fp16", "fp16", "fast")]


@pytest.fixture(scope="module", autouse=True)
def _built():
    adanerf_amd.build_library()


@pytest.fixture(scope="module")
def base_case():
    return load_case("synthetic_fixed8")


@pytest.fixture(scope="module")
def filler():
    """the network a probe's model directory does not care about"""
    return O.synthetic_weights(1)


def labels(cols, dir_block):
    """per column: -1 for an identity slot, else band (+ 32 in the direction block): what the figures are grouped by"""
    return np.array([-1 if kind == "id" else band + (32 if blk == dir_block else 0) for (blk, F, kind, band, comp) in cols])


class Figures:
    """per (engine, label): slots, slots outside the bound, slots that needed the widening, max |out - sin64(a)|, summed over probes"""

    def __init__(self):
        self.d = {}

    def add(self, engine, res):
        for b, v in res["per_band"].items():
            f = self.d.setdefault((engine, b), dict(slots=0, bad=0, moved=0.0, max_err=0.0))
            f["slots"] += v["slots"]
            f["bad"] += v["bad"]
            f["moved"] += v["moved"] * v["slots"]
            f["max_err"] = max(f["max_err"], v["max_err"]) if v["max_err"] == v["max_err"] else float("nan")

    def log(self, **ctx):
        for (engine, b), f in sorted(self.d.items()):
            record("fused_encodings_band", engine=engine, block="identity" if b < 0 else ("direction" if b >= 32 else "position"), band=int(b % 32) if b >= 0 else -1,
                   slots=f["slots"], outside=f["bad"], needed_widening=f["moved"] / max(f["slots"], 1), max_abs_err=f["max_err"], **ctx)

    def failures(self):
        return {k: (f["bad"], f["slots"], f["max_err"]) for k, f in sorted(self.d.items()) if f["bad"]}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------

def sampling_dir(tmp_path_factory, filler, tag, sc, depth, width, slots, seed):
    d = str(tmp_path_factory.mktemp("probe_" + tag))
    O.write_model_dir(d, sc, O.Weights(P.sampling_probe(sc.n_in0, depth, width, slots, seed=seed), filler.net1))
    return d


def device_rays(r, sc):
    """(u, p, nds, feature rows, ray records) of the whole frame from adanerf_ray_features; the record's p has the bits of the features' own"""
    fb, rb = Guarded(r, N_RAYS * sc.n_in0 * 4), Guarded(r, N_RAYS * 32)
    r.ray_features(0, N_RAYS, fb.ptr, rb.ptr)
    r.sync()
    feat = fb.body("features").view(np.float32).reshape(N_RAYS, sc.n_in0).copy()
    rec = rb.body("ray records").view(np.float32).reshape(N_RAYS, 8).copy()
    fb.free()
    rb.free()
    qd = 3 + 6 * sc.pos_enc[0][1]
    assert np.array_equal(bits(feat[:, qd:qd + 3]), bits(rec[:, 0:3])), "the features' position columns are not the ray record's p"
    assert np.isfinite(feat).all() and np.isfinite(rec).all()
    return feat[:, 0:3].copy(), rec[:, 0:3].copy(), rec[:, 4:7].copy(), feat, rec


@pytest.mark.parametrize("case,scene", [(c, s) for c, v in SAMPLING.items() for s in v[5]], ids=lambda v: v)
def test_sampling_slots(case, scene, base_case, filler, tmp_path_factory):
    t0 = time.perf_counter()
    depth, width, pe0, rsi, engines, _ = SAMPLING[case]
    sc, rots, pose = P.scene_of(base_case[2], scene, pe0=pe0, ray_sample_input=rsi)
    cols = P.sampling_columns(sc)
    lab = labels(cols, 0)
    ident = lab < 0
    groups = P.slot_groups(sc.n_in0, width)
    dirs = [sampling_dir(tmp_path_factory, filler, "%s_%s_%d" % (case, scene, gi), sc, depth, width, g, gi) for gi, g in enumerate(groups)]
    fig = Figures()
    xs, expect = [], {}
    for mode, model, form in engines:
        for gi, slots in enumerate(groups):
            with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(dirs[gi], W, H), precision="bf16", sampling=mode) as r:
                assert r.info.n_in0 == sc.n_in0
                for ri, rot in enumerate(rots):
                    r.set_camera(pose, rot)
                    if (ri, "x") not in expect:      # the device's own x, once per camera
                        expect[ri, "x"] = device_rays(r, sc)
                        xs.append(expect[ri, "x"][1])
                    u, p, nds, feat, rec = expect[ri, "x"]
                    if (ri, form) not in expect:
                        if rsi and (ri, "z") not in expect:      # the device's depths of the raySampleInput points, off adanerf_ray_features' identity columns
                            n0, npb = sc.n_in0 - rsi * (3 + 6 * pe0[0]), 3 + 6 * pe0[0]
                            expect[ri, "z"] = P.fit_ray_sample_depths(np.stack([feat[:, n0 + a * npb:n0 + a * npb + 3] for a in range(rsi)]), p, nds, sc)
                        expect[ri, form] = P.sampling_expectation(u, p, nds, sc, form, zs=expect.get((ri, "z")))
                    s, E, truth, _ = expect[ri, form]
                    out, rays = Guarded(r, N_RAYS * 512), Guarded(r, N_RAYS * 32)
                    r.sample_mlp(0, N_RAYS, out.ptr, rays.ptr)
                    r.sync()
                    rows = out.body("rows %s %s %s" % (case, scene, mode)).view(np.float32).reshape(N_RAYS, 128).copy()
                    assert rays.body("ray records").tobytes() == rec.tobytes(), "%s %s %s: rays_out differs from adanerf_ray_features' records" % (case, scene, mode)
                    rays.free()
                    k = len(slots)
                    assert not rows[:, k:].any(), "%s %s %s: an output without a slot is not 0" % (case, scene, mode)
                    res = P.check_slots(rows[:, :k], s[:, slots], E[:, slots], model, lab[slots], truth[:, slots])
                    fig.add("%s/%s" % (KERNEL_CLASS[model], form), res)
                    if model == "exact":      # identity slots: the bits of x (the features' identity columns; raySampleInput: restated in numpy)
                        idc = np.flatnonzero(ident[slots])
                        want = s[:, slots][:, idc].astype(np.float32)
                        assert np.array_equal(bits(rows[:, idc]) & 0x7FFFFFFF, bits(want) & 0x7FFFFFFF) and np.array_equal(rows[:, idc], want), \
                            "%s %s %s: identity slots do not carry the bits of x" % (case, scene, mode)
                        own = np.flatnonzero(ident[slots] & (np.array(slots) < feat.shape[1]))
                        assert np.array_equal(rows[:, own], feat[:, np.array(slots)[own]]), "identity slots against adanerf_ray_features' columns"
                    if scene == "near" and ri == 0 and gi == 0:      # position invariance
                        for first, n in WINDOWS:
                            win = Guarded(r, n * 512)
                            r.sample_mlp(first, n, win.ptr, None)
                            r.sync()
                            got = win.body("window (%d, %d)" % (first, n)).view(np.float32).reshape(n, 128)
                            assert got.tobytes() == rows[first:first + n].tobytes(), "%s %s: rays (%d, %d) differ from the whole-frame call" % (case, mode, first, n)
                            win.free()
                    out.free()
    info = P.conditions(scene, xs, pe0[0])
    if scene == "near":
        P.conditions("near", [expect[ri, "x"][0] for ri in range(len(rots))], pe0[1])
    record("fused_encodings_scene", stage="sampling", case=case, contexts=len(engines) * len(groups), seconds=time.perf_counter() - t0, **info)
    fig.log(stage="sampling", case=case, scene=scene)
    assert not fig.failures(), "%s %s: slots outside their bound, (engine, band (+32: direction)): (outside, of, max |out - sin64|) %s" % (case, scene, fig.failures())


@pytest.mark.parametrize("case,scene", [("fixed_10_4", "near"), ("fixed_10_4", "far"), ("fixed_10_4", "straddle"), ("fixed_2_2", "near")], ids=lambda v: v)
def test_two_block_kernel_on_the_probe(case, scene, base_case, filler, tmp_path_factory, monkeypatch):
    """sample_mlp16x2_kernel writes no rows: on probe networks a fused frame's counts, bins and kept values under $ADANERF_DEBUG_GUARD bit 4
    have the bits of the 8-wave kernel's under bit 2 -- and both are the rule on the 8-wave kernel's stage rows, which test_sampling_slots
    holds to the slots.  Through the all-slots probe the selection shows only each ray's few largest slots; the 16-slot probes, plain and
    negated, put every slot beyond +-2^-10 among the kept values, so a wrong small or negative slot shows too.  What stays unseen is a slot
    value inside +-2^-10."""
    t0 = time.perf_counter()
    depth, width, pe0, rsi, engines, _ = SAMPLING[case]
    sc, rots, pose = P.scene_of(base_case[2], scene, pe0=pe0)
    every = P.slot_groups(sc.n_in0, width)[0]
    assert len(every) == sc.n_in0
    # (slots, sign, [(N, thr)]): all slots at once -- the selection then sees each ray's few largest -- and every slot again in groups of 16, plain
    # and negated, with N = 16 and a threshold of 2^-10: whatever the group holds beyond +-2^-10 is kept, value and bin
    probes = [(every, 1.0, [(8, 0.125), (16, 0.5), (3, 0.9375)])]
    probes += [(every[i:i + 16], sg, [(16, 2.0 ** -10)]) for i in range(0, len(every), 16) for sg in (1.0, -1.0)]
    seen = np.zeros(sc.n_in0, np.int64)
    for pi, (slots, sg, walk) in enumerate(probes):
        d = str(tmp_path_factory.mktemp("two_block_%s_%s_%d" % (case, scene, pi)))
        O.write_model_dir(d, sc, O.Weights(P.sampling_probe(sc.n_in0, depth, width, slots, seed=pi, sign=sg), filler.net1))
        rows = []
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="bf16", sampling="fp16") as r:
            out = Guarded(r, N_RAYS * 512)
            for rot in rots:
                out.reset()
                r.set_camera(pose, rot)
                r.sample_mlp(0, N_RAYS, out.ptr, None)
                r.sync()
                rows.append(out.body("stage rows").view(np.float32).reshape(N_RAYS, 128).copy())
        frames = {}
        for dbg in ("2", "4"):
            monkeypatch.setenv("ADANERF_DEBUG_GUARD", dbg)
            with Live(d, dict(pose=pose, rot=rots[0]), W, H, 8, 0.125, sampling="fp16") as c:
                for ri, rot in enumerate(rots):
                    c.r.set_camera(pose, rot)
                    for n, thr in walk:
                        c.r.set_selection(n, thr)
                        frames[dbg, ri, n, thr] = c.frame()[0]
        for (dbg, ri, n, thr), f in frames.items():
            tag = "%s %s probe %d camera %d (%d, %g)" % (case, scene, pi, ri, n, thr)
            same(f, rule(rows[ri], n, thr), tag + " debug guard %s against the rule on the stage rows" % dbg)
            same(f, frames["2", ri, n, thr], tag + ": the two-block kernel against the 8-wave kernel", keys=("counts", "offsets", "total", "key", "w", "rgba", "rgb"))
        if pi:      # rays on which the group's slot is among the kept values (its bin in the key, its bits in the kept values)
            seen[np.array(slots)] += sum((rw[:, :len(slots)] >= walk[0][1]).sum(axis=0) for rw in rows)
    record("fused_encodings_two_block", case=case, scene=scene, probes=len(probes), contexts=3 * len(probes), seconds=time.perf_counter() - t0, slots=int(sc.n_in0), rays=N_RAYS * len(rots),
           kept_share_min=float(seen.min() / (N_RAYS * len(rots))), kept_share_mean=float(seen.mean() / (N_RAYS * len(rots))))
    assert (seen > 0).all(), "%s %s: slots %s never reach the kept values" % (case, scene, np.flatnonzero(seen == 0))


# ---- shading ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,scene", [(c, s) for c, v in SHADING.items() for s in v[4]], ids=lambda v: v)
def test_shading_slots(case, scene, base_case, filler, tmp_path_factory):
    t0 = time.perf_counter()
    depth, width, skips, pe1, _ = SHADING[case]
    sc, rots, pose = P.scene_of(base_case[2], scene, pe1=pe1)
    n_pos, n_dir = 3 + 6 * pe1[0], 3 + 6 * pe1[1]
    cols = P.shading_columns(sc)
    lab = labels(cols, 1)
    plan = P.shading_plan(n_pos, n_dir)
    key = P.shade_keys(N_RAYS)
    S = key.size
    fig = Figures()
    xs, ds, expect = [], [], {}
    for i, slots in enumerate(plan):
        d = str(tmp_path_factory.mktemp("probe_%s_%s_%d" % (case, scene, i)))
        O.write_model_dir(d, sc, O.Weights(filler.net0, P.shading_probe(n_pos, n_dir, depth, width, skips, slots, seed=i)))
        order = [slots[1], slots[2], slots[3], slots[0]]      # (r, g, b, alpha)
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, W, H), precision="fp32") as r:
            d_key = r.to_device(key)
            out = Guarded(r, S * 16)
            for ri, rot in enumerate(rots):
                r.set_camera(pose, rot)
                rays_g = Guarded(r, N_RAYS * 32)
                rays = rays_g.ptr
                r.ray_features(0, N_RAYS, None, rays)
                r.sync()
                assert np.isfinite(rays_g.body("ray records").view(np.float32)).all()
                if (ri, "x") not in expect:      # the device's own x: the identity columns of adanerf_shade_features
                    fb = Guarded(r, S * sc.n_in1 * 4)
                    r.shade_features(rays, d_key, S, fb.ptr)
                    r.sync()
                    feat = fb.body("shade features").view(np.float32).reshape(S, sc.n_in1).copy()
                    fb.free()
                    assert np.isfinite(feat).all()
                    expect[ri, "x"] = (feat[:, :3].copy(), feat[:, n_pos:n_pos + 3].copy())
                    xs.append(expect[ri, "x"][0])
                    ds.append(expect[ri, "x"][1])
                x, dd = expect[ri, "x"]
                for prec, model, form in SHADE_ENGINES:
                    if (ri, form) not in expect:
                        expect[ri, form] = P.shading_expectation(x, dd, sc, form)
                    s, E, truth, _ = expect[ri, form]
                    K = run_shade(r, lambda k, t, m, raw, p, long: r.shade_mlp(rays, k, t, m, raw, p), d_key, S, S, out, prec).copy()
                    res = P.check_slots(K, s[:, order], E[:, order], model, lab[order], truth[:, order])
                    fig.add("%s/%s" % (prec, form), res)
                    if model == "exact":      # cross-check of x itself: the fp32 probe's identity outputs are its bits
                        idc = np.flatnonzero(lab[order] < 0)
                        assert np.array_equal(K[:, idc], s[:, order][:, idc].astype(np.float32)), "%s %s probe %d: identity slots against adanerf_shade_features" % (case, scene, i)
                rays_g.free()
            out.free()
    far_dirs = scene == "far" and pe1[1] >= 12      # the 16-band direction encoding is the far one of that case
    info = P.conditions(scene, ds if far_dirs else xs, pe1[1] if far_dirs else pe1[0])
    if scene == "near":
        P.conditions("near", ds, pe1[1])
    record("fused_encodings_scene", stage="shading", case=case, contexts=len(plan), seconds=time.perf_counter() - t0, **info)
    fig.log(stage="shading", case=case, scene=scene)
    assert not fig.failures(), "%s %s: slots outside their bound, (engine, band (+32: direction)): (outside, of, max |out - sin64|) %s" % (case, scene, fig.failures())
