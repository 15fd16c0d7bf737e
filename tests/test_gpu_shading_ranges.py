"""The 16-bit shading kernels at the edges of their value ranges (the CPU side and the networks / rows: tests/test_shading_ranges_cpu.py):

 A. power-of-two rescaling is exact: the bf16 raw outputs of a rescaled network (mlp_reference.rescale) are the base network's times the two
    output powers of two, bit for bit; fp32 agrees with fp64 of the rescaled network.  (fp16 is left out: subnormals move under rescaling.)
 B. the clamped conversion does not fire when the packer's premise is filled: non-negative networks, positions pushed to |x| <= 4090 through
    adanerf_shade_mlp_z under normalisation "None", against the bf16 rounding model on host features.  (fp16 is left out: the fp64 hidden
    activations exceed 65504 -- asserted in the CPU test.)
 C. all seven normalisations (and a config without the key) through the 16-bit kernels' own front end -- sample_position, the v_sin_f32
    encoding -- against the rounding model on the device's own fp32 feature rows; |x| reaches 8 under "None".
 D. non-finite and out-of-premise positions: every poisoned sample comes out non-finite where fp64 is non-finite -- in bf16 also where
    |x| > kPosIdentityBound, the premise of the scaled packing -- and every other sample keeps the bits of the clean launch.

Bounds of B and C: per quantity the larger of mlp_reference.BOUNDS and 1.5 x what the emulated correct kernel shows on the same rows
(mlp_reference.emulation_bounds: from the reference alone); both are logged with the measured quantities (profiles/shading_ranges_measured.log)."""
import dataclasses

import numpy as np
import pytest

import adanerf_oracle as O
import mlp_reference as M
from conftest import NORM_CASES, case_weights, load_case, record
from test_gpu_mlp_engines import BASE, HOST_FEATURE_FP32, PREC, SHADE_CASES, Guarded, _built, _log, base_case, base_keys, run_shade, same_bits, shading_model      # noqa: F401
from test_gpu_parity import golden_ray_records, golden_samples
from test_shading_ranges_cpu import (K_POS_IDENTITY_BOUND, POSITIVE_CASES, RESCALE_TOPOLOGIES, SCHEDULES, out_exponents, positive_case, rescale_model,
                                     schedule, write_net1)

import adanerf_amd

pytestmark = pytest.mark.gpu


def _shade(r, rays, d_key, n, out, prec, d_z=None):
    fn = (lambda k, t, m, raw, p, long: r.shade_mlp(rays, k, t, m, raw, p)) if d_z is None else \
         (lambda k, t, m, raw, p, long: r.shade_mlp_z(rays, k, d_z, t, m, raw, p))
    return run_shade(r, fn, d_key, n, n, out, prec).copy()


# ---- A ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", RESCALE_TOPOLOGIES)
def test_rescaled_networks_give_the_base_outputs_times_powers_of_two(tag, base_case, tmp_path_factory):
    z = base_case[0]
    sc, wts, d, n_pos = rescale_model(base_case, tmp_path_factory, tag)
    depth = SHADE_CASES[tag][0]
    key = base_keys(np.random.default_rng(91), 256 * 256, 128)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 256, 256), precision="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        rays = r.empty((256 * 256, 8), np.float32)
        r.ray_features(0, 256 * 256, None, rays)
        rec = rays.numpy()
        d_key = r.to_device(key)
        f = r.empty((BASE, sc.n_in1), np.float32)
        r.shade_features(rays, d_key, BASE, f)
        feat = f.numpy()
        out = Guarded(r, BASE * 16)
        K0 = _shade(r, rays, d_key, BASE, out, "bf16")
    ref0 = M.shading_mlp64(feat, wts.net1, n_pos)
    M.check_engine(K0, ref0, M.shading_mlp64(feat, wts.net1, n_pos, "bf16"), "bf16", log=_log("shading_ranges_rescale", case=tag, schedule="base", prec="bf16"))
    for sched in SCHEDULES:
        E = schedule(sched, depth)
        Ea, Ec = out_exponents(E)
        net = M.rescale(wts.net1, n_pos, E)
        dr = write_net1(tmp_path_factory, "gpu_rs_%s_%s" % (tag, sched), sc, wts, net)
        with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(dr, 256, 256), precision="fp32") as r:
            r.set_camera(z["pose"], z["rot"])
            rays, d_key = r.to_device(rec), r.to_device(key)
            out = Guarded(r, BASE * 16)
            K = _shade(r, rays, d_key, BASE, out, "bf16")
            K32 = _shade(r, rays, d_key, BASE, out, "fp32")
        want = np.ldexp(K0, np.array([Ec, Ec, Ec, Ea], np.int32)).astype(np.float32)
        assert np.isfinite(want).all()
        bad = np.flatnonzero((K.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        record("shading_ranges_rescale_bits", case=tag, schedule=sched, prec="bf16", Ea=Ea, Ec=Ec, rows=BASE, rows_differing=int(bad.size))
        assert bad.size == 0, "%s %s: %d of %d bf16 rows are not the base rows x (2^%d, 2^%d), first %s" % (tag, sched, bad.size, BASE, Ec, Ea, bad[:8])
        ref = M.shading_mlp64(feat, net, n_pos)
        M.check_engine(K32, ref, ref, "fp32", log=_log("shading_ranges_rescale", case=tag, schedule=sched, prec="fp32"))


# ---- B ---------------------------------------------------------------------------------------------------------------------------------

def _ray_records(o, d):
    rec = np.zeros((o.shape[0], 8), np.float32)
    rec[:, 0:3], rec[:, 4:7] = o, d
    return rec


@pytest.mark.parametrize("tag", list(POSITIVE_CASES))
def test_the_clamp_does_not_fire_when_the_premise_is_filled(tag, base_case, tmp_path_factory):
    z = base_case[0]
    sc, wts, n_pos, o, dirs, zw, mask, feat = positive_case(base_case, tag)
    d = write_net1(tmp_path_factory, "gpu_" + tag, sc, wts, wts.net1)
    n = o.shape[0]
    key = (np.arange(n, dtype=np.uint32) << 7) | (np.arange(n, dtype=np.uint32) * 37 % 128)      # one ray per sample; the bin is not used with explicit depths
    ref64 = M.shading_mlp64(feat, wts.net1, n_pos)
    refq = M.shading_mlp64(feat, wts.net1, n_pos, "bf16")
    bounds, shown = M.emulation_bounds(feat, wts.net1, n_pos, "bf16", ref64, refq)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 64, 64), precision="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        rays, d_key, d_z = r.to_device(_ray_records(o, dirs)), r.to_device(key), r.to_device(zw)
        out = Guarded(r, n * 16)
        K = _shade(r, rays, d_key, n, out, "bf16", d_z)
        K32 = _shade(r, rays, d_key, n, out, "fp32", d_z)
    ctx = dict(case=tag, n=n, premise_rows=int(mask.sum()), max_abs_x=float(np.abs(feat[:, :3]).max()))
    M.check_engine(K, ref64, refq, "bf16", bounds=bounds, log=_log("shading_ranges_premise", prec="bf16", bounds=bounds, emulation=shown, **ctx))
    M.check_engine(K32, ref64, ref64, "fp32", bounds=HOST_FEATURE_FP32["fp32"], log=_log("shading_ranges_premise", prec="fp32", **ctx))


# ---- C ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NORM_CASES)
def test_normalisations_through_the_16_bit_front_end(name, tmp_path_factory):
    zf, meta, sc = load_case(name)
    wts = case_weights(meta)
    d = str(tmp_path_factory.mktemp("norm16_" + name))
    O.write_model_dir(d, sc, wts)
    count, off, key, sw, sray, sbin = golden_samples(zf, sc)
    S = min(len(key), 2570)
    n_pos = 3 + 6 * sc.pos_enc[1][0]
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, meta["w"], meta["h"]), precision="fp32") as r:
        r.set_camera(zf["pose"], zf["rot"])
        rays, d_key = r.to_device(golden_ray_records(zf, meta, sc)), r.to_device(key[:S])
        f = r.empty((S, sc.n_in1), np.float32)
        r.shade_features(rays, d_key, S, f)      # the accurate encoding of the device's own positions
        feat = f.numpy()
        out = Guarded(r, S * 16)
        K = {prec: _shade(r, rays, d_key, S, out, prec) for prec in ("bf16", "fp16")}
    ref64 = M.shading_mlp64(feat, wts.net1, n_pos)
    ctx = dict(case=name, normalization=sc.normalization or "(absent)", n=S, max_abs_x=float(np.abs(feat[:, :3]).max()))
    failed = []
    for prec in ("bf16", "fp16"):
        refq = M.shading_mlp64(feat, wts.net1, n_pos, prec)
        bounds, shown = M.emulation_bounds(feat, wts.net1, n_pos, prec, ref64, refq)
        try:
            M.check_engine(K[prec], ref64, refq, prec, bounds=bounds, log=_log("shading_ranges_normalisation", prec=prec, bounds=bounds, emulation=shown, **ctx))
        except AssertionError as e:      # both engines are measured and logged before the test fails
            failed.append(str(e))
    assert not failed, failed


# ---- D ---------------------------------------------------------------------------------------------------------------------------------

N_D = 257
# poisoned samples: the first, the last, both sides of a 32-sample block, of a wave (64) and of the 128- and 256-sample tiles of the kernels
POISON_AT = [0, 31, 32, 63, 64, 127, 128, 255, 256]
NAN, INF = float("nan"), float("inf")
# what is poisoned, in turn: (field of the ray record or "z", component, value)
POISONS = [("o", 0, NAN), ("z", 0, NAN), ("d", 1, INF), ("z", 0, 1.0e6), ("o", 2, -INF), ("z", 0, INF), ("d", 0, NAN), ("z", 0, 1.0e6), ("d", 2, -INF)]
D_CASES = {"fixed_8x256": "fixed_8x256", "staged_w96_d5": "w96_d5_skips1_3"}


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", list(D_CASES))
def test_non_finite_and_out_of_premise_positions(case, prec, base_case, tmp_path_factory):
    """Non-finite values are ordinary data here: a NaN / inf origin, direction or depth makes the position non-finite, the fp64 network
    returns NaN for it, and so must every engine (a ReLU that turns NaN into 0 would hand the compositing a finite colour).  A depth of 1e6
    leaves the position finite but beyond kPosIdentityBound, outside what the bf16 packing's scaling was proved for: bf16 returns NaN there,
    never a clamped value; fp16 and fp32 are not constrained by fp64 there."""
    tag = D_CASES[case]
    depth, width, skips, pe1 = SHADE_CASES[tag]
    # normalisation "None": a depth of 1e6 then IS a position of 1e6 (the scene's own InverseSqrtDistCentered would fold it back to ~340)
    plain = (base_case[0], base_case[1], dataclasses.replace(base_case[2], normalization="None"))
    z, sc, wts, d = shading_model(plain, tmp_path_factory, "poison_" + case, depth, width, skips, pe1, 900 + list(SHADE_CASES).index(tag))
    n_pos = 3 + 6 * pe1[0]
    rng = np.random.default_rng(93)
    with adanerf_amd.NeuralRenderer(adanerf_amd.Settings(d, 64, 64), precision="fp32") as r:
        r.set_camera(z["pose"], z["rot"])
        frame = r.empty((64 * 64, 8), np.float32)
        r.ray_features(0, 64 * 64, None, frame)
        rec = frame.numpy()[rng.choice(64 * 64, N_D, replace=False)]      # one ray per sample
        bins = rng.integers(0, 128, N_D)
        bins[:2] = (0, 127)
        key = (np.arange(N_D, dtype=np.uint32) << 7) | bins.astype(np.uint32)
        zw = O.to_world_depth(((bins + rng.uniform(0.05, 0.95, N_D)) / 128.0).astype(np.float32), sc).astype(np.float32)
        rec_p, zw_p = rec.copy(), zw.copy()
        for i, (what, c, v) in zip(POISON_AT, POISONS):
            if what == "z":
                zw_p[i] = v
            else:
                rec_p[i, (0 if what == "o" else 4) + c] = v
        with np.errstate(all="ignore"):
            feat_p = O.shading_inputs(rec_p[:, 0:3], rec_p[:, 4:7], np.arange(N_D), zw_p, sc)
            ref_p = M.shading_mlp64(feat_p, wts.net1, n_pos)
        must = ~np.isfinite(ref_p)                                          # [n, 4]: where fp64 is non-finite
        amax = np.abs(feat_p[:, :3]).max(axis=1)
        beyond = np.isfinite(amax) & (amax > K_POS_IDENTITY_BOUND)         # finite, out of premise
        poisoned = np.zeros(N_D, bool)
        poisoned[POISON_AT] = True
        assert must[poisoned & ~beyond].all() and not must[~poisoned].any() and beyond.sum() == 2 and not must[beyond].any()
        d_key = r.to_device(key)
        out = Guarded(r, N_D * 16)
        clean = _shade(r, r.to_device(rec), d_key, N_D, out, prec, r.to_device(zw))
        got = _shade(r, r.to_device(rec_p), d_key, N_D, out, prec, r.to_device(zw_p))
        # the entry point without explicit depths: the poisoned ray records alone, depths at the bin centres
        clean_c = _shade(r, r.to_device(rec), d_key, N_D, out, prec)
        got_c = _shade(r, r.to_device(rec_p), d_key, N_D, out, prec)
    ray_poisoned = np.zeros(N_D, bool)
    ray_poisoned[[i for i, p in zip(POISON_AT, POISONS) if p[0] != "z"]] = True
    assert np.isfinite(clean).all() and np.isfinite(clean_c).all()
    finite_where_must_not = np.flatnonzero((must & np.isfinite(got)).any(axis=1))
    finite_c = np.flatnonzero(ray_poisoned & np.isfinite(got_c).any(axis=1))
    clamped = np.flatnonzero(beyond & np.isfinite(got).any(axis=1)) if prec == "bf16" else np.zeros(0, np.int64)
    moved = np.flatnonzero(~poisoned & (got.view(np.uint32) != clean.view(np.uint32)).any(axis=1))
    moved_c = np.flatnonzero(~ray_poisoned & (got_c.view(np.uint32) != clean_c.view(np.uint32)).any(axis=1))
    record("shading_ranges_poison", case=case, prec=prec, n=N_D, poisoned=int(poisoned.sum()), finite_where_fp64_is_not=[int(i) for i in finite_where_must_not],
           finite_ray_poison_bin_centres=[int(i) for i in finite_c], beyond_premise_finite=[int(i) for i in clamped],
           beyond_premise_outputs=[[float(v) for v in got[i]] for i in np.flatnonzero(beyond)], clean_rows_moved=int(moved.size + moved_c.size))
    assert finite_where_must_not.size == 0, "%s %s: samples %s are finite where fp64 is not: %s" % (case, prec, finite_where_must_not, got[finite_where_must_not])
    assert finite_c.size == 0, "%s %s (bin centres): samples %s are finite where fp64 is not" % (case, prec, finite_c)
    assert clamped.size == 0, "%s bf16: samples %s lie beyond kPosIdentityBound and came out finite: %s" % (case, clamped, got[clamped])
    assert moved.size == 0 and moved_c.size == 0, "%s %s: clean samples %s / %s changed next to poisoned ones" % (case, prec, moved, moved_c)
