"""tests/probe_networks.py without a GPU: the probes return their slots bit for bit under the oracle and under every rounding model of
mlp_reference; expected() has the oracle's column order; the scenes fill the conditions the GPU test relies on; and the checker rejects each
planted fault by name (and passes the unplanted values)."""
import dataclasses
import math

import numpy as np
import pytest

import adanerf_oracle as O
import mlp_reference as M
import probe_networks as P
from conftest import load_case

ENCODINGS = {"10-4": ((10, 4), (10, 4)), "2-2": ((2, 2), (10, 4)), "16-1_1-16": ((16, 1), (1, 16)), "6-3_12-2": ((6, 3), (12, 2))}
MODELS = ("exact", "split", "fp16", "bf16")


@pytest.fixture(scope="module")
def base_case():
    return load_case("synthetic_fixed8")


def frame(base_case, sc):
    z = base_case[0]
    return P.frame_inputs(sc, z["pose"], z["rot"])


def shade_rows(base_case, sc, n=P.N_SHADE):
    """(x, d, features) of n samples of the W x H frame as the oracle computes them"""
    u, p, nds, _ = frame(base_case, sc)
    key = P.shade_keys(P.W * P.H, n)
    ray, b = (key >> 7).astype(np.int64), (key & 127).astype(np.int64)
    zw = O.to_world_depth(O.bin_t(b), sc).astype(np.float32)
    feat = O.shading_inputs(p, nds, ray, zw, sc)
    n_pos = 3 + 6 * sc.pos_enc[1][0]
    return feat[:, :3].copy(), feat[:, n_pos:n_pos + 3].copy(), feat


# ---- the probes are exact -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,depth,width,enc,rsi", [("fixed_10_4", 8, 256, "10-4", 0), ("fixed_2_2", 8, 256, "2-2", 0), ("gen_w128_rsi4", 4, 128, "10-4", 4),
                                                     ("gen_w96_16_1", 3, 96, "16-1_1-16", 0), ("wide_w384_6_3", 3, 384, "6-3_12-2", 0)])
def test_sampling_probes_return_their_slots(tag, depth, width, enc, rsi, base_case):
    sc = dataclasses.replace(base_case[2], pos_enc=ENCODINGS[enc], ray_sample_input=rsi)
    feat = frame(base_case, sc)[3]
    assert feat.shape == (P.W * P.H, sc.n_in0)
    groups = P.slot_groups(sc.n_in0, width)
    assert tag != "fixed_10_4" or len(groups) == 1      # one probe covers all 90 inputs of the 10-4 encoding
    assert sorted(c for g in groups for c in g) == list(range(sc.n_in0))
    for gi, slots in enumerate(groups):
        net = P.sampling_probe(sc.n_in0, depth, width, slots, seed=gi)
        assert all(set(np.unique(v)) <= {-1.0, 0.0, 1.0} for k, v in net.items() if k.endswith("weight")) and all(not v.any() for k, v in net.items() if k.endswith("bias"))
        want = feat[:, slots]
        got = O.sampling_mlp(feat, net)
        assert (got[:, :len(slots)] == want).all() and not got[:, len(slots):].any(), (tag, gi, "O.sampling_mlp")
        for model in MODELS:
            got = M.sampling_mlp64(feat, net, model)
            assert np.array_equal(got[:, :len(slots)], P.ROUNDING(want, model)), (tag, gi, model)
            assert not got[:, len(slots):].any()
        assert np.array_equal(P.ROUNDING(want, "exact").astype(np.float32).view(np.uint32) & 0x7FFFFFFF, want.view(np.uint32) & 0x7FFFFFFF)
    neg = P.sampling_probe(sc.n_in0, depth, width, groups[0][:16], seed=7, sign=-1.0)      # the negated copy the two-block kernel's test renders
    for model in MODELS:
        assert np.array_equal(M.sampling_mlp64(feat, neg, model)[:, :16], -P.ROUNDING(feat[:, groups[0][:16]], model)), (tag, "negated", model)


@pytest.mark.parametrize("tag,depth,width,skips,enc,every", [("fixed_8x256", 8, 256, [4], "10-4", 4), ("w96_d5_skips1_3", 5, 96, [1, 3], "10-4", 1),
                                                             ("w96_d5_12_2", 5, 96, [1, 3], "6-3_12-2", 3), ("w257_d3_1_16", 3, 257, [1], "16-1_1-16", 5)])
def test_shading_probes_return_their_slots(tag, depth, width, skips, enc, every, base_case):
    sc = dataclasses.replace(base_case[2], pos_enc=ENCODINGS[enc])
    n_pos, n_dir = 3 + 6 * sc.pos_enc[1][0], 3 + 6 * sc.pos_enc[1][1]
    feat = shade_rows(base_case, sc, 601)[2]
    plan = P.shading_plan(n_pos, n_dir)
    assert enc != "10-4" or len(plan) == 23      # 23 networks cover the 63 + 27 slots
    for i, slots in list(enumerate(plan))[::every]:
        net = P.shading_probe(n_pos, n_dir, depth, width, skips, slots, seed=i)
        assert O.shading_topology(net, n_pos) == (depth, skips)
        want = feat[:, [slots[1], slots[2], slots[3], slots[0]]]      # (r, g, b, alpha)
        assert (O.shading_mlp(feat, net, n_pos) == want).all(), (tag, i, "O.shading_mlp")
        for model in MODELS:
            assert np.array_equal(M.shading_mlp64(feat, net, n_pos, model), P.ROUNDING(want, model)), (tag, i, model)


def test_the_checker_on_a_real_probe_equals_the_checker_on_the_rounding(base_case):
    """check_slots(probe=...) evaluates mlp_reference on the probe network itself, as the bound is defined; the default takes ROUNDING"""
    sc = base_case[2]
    u, p, nds, feat = frame(base_case, sc)
    s, E, truth, bands = P.sampling_expectation(u, p, nds, sc, "accurate")
    slots = P.slot_groups(sc.n_in0, 256)[0]
    net = P.sampling_probe(sc.n_in0, 4, 256, slots)
    rows = slice(0, 997)
    for model in MODELS:
        out = M.sampling_mlp64(feat[rows], net, model)[:, :len(slots)]
        a = P.check_slots(out, s[rows], E[rows], model, bands, truth[rows])
        b = P.check_slots(out, s[rows], E[rows], model, bands, truth[rows], probe=lambda v: M.sampling_mlp64(v, net, model)[:, :len(slots)])
        assert np.array_equal(a["bad"], b["bad"]) and np.array_equal(a["moved"], b["moved"]) and not a["bad"].any(), model


# ---- the column order ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("enc", list(ENCODINGS))
@pytest.mark.parametrize("rsi", [0, 4])
def test_expected_has_the_oracles_columns(enc, rsi, base_case):
    sc = dataclasses.replace(base_case[2], pos_enc=ENCODINGS[enc], ray_sample_input=rsi)
    u, p, nds, feat = frame(base_case, sc)
    s, E, truth, bands = P.sampling_expectation(u, p, nds, sc, "accurate")
    cols = P.sampling_columns(sc)
    ident = np.array([c[2] == "id" for c in cols])
    assert s.shape == feat.shape and (E[:, ident] == 0).all() and (E[:, ~ident] > 0).all() and np.array_equal(bands, [c[3] for c in cols])
    assert np.array_equal(s[:, ident].astype(np.float32).view(np.uint32), feat[:, ident].view(np.uint32)), "identity columns"
    # the oracle's sin / cos are fp32 libm values of the same exact fp32 arguments: within an fp32 ulp of fp64
    assert np.abs(s - feat).max() <= 1.2e-7, (enc, rsi, np.abs(s - feat).max())
    if rsi == 0:
        x, d, sfeat = shade_rows(base_case, sc, 601)
        s1, E1, t1, b1 = P.shading_expectation(x, d, sc, "accurate")
        assert s1.shape == sfeat.shape and np.abs(s1 - sfeat).max() <= 1.2e-7 and np.array_equal(b1, [c[3] for c in P.shading_columns(sc)])
        # the fast form is the same function of x to within the fp32 rounding of the revolution count (half an ulp of r) and of the
        # constant 1 / 2 pi (a relative error that grows with r): 2 pi (ulp(r) / 2 + r |delta|)
        sf = P.shading_expectation(x, d, sc, "fast")[0]
        rmax = max(P.revolutions(x, sc.pos_enc[1][0]).max(), P.revolutions(d, sc.pos_enc[1][1]).max()) + 0.25
        delta = abs(float(P.INV_2PI_F32) * 2.0 * math.pi - 1.0)
        assert np.abs(sf - s1).max() <= 2.0 * math.pi * (np.spacing(np.float32(rmax)) * 0.5 + rmax * delta) * 1.01 + 1e-9


def test_ray_sample_depths_are_read_off_the_identity_columns(base_case):
    """fit_ray_sample_depths finds depths a few ulp from the oracle's exactly, and refuses identity columns no depth reproduces"""
    sc = dataclasses.replace(base_case[2], ray_sample_input=4)
    u, p, nds, feat = frame(base_case, sc)
    zs = (O.ray_sample_depths(sc).view(np.int32) + np.array([-4, 0, 2, -3], np.int32)).view(np.float32)
    xs, d1 = P.ray_sample_points(p, nds, sc, zs)
    ident = (xs * d1).astype(np.float32)
    assert np.array_equal(P.fit_ray_sample_depths(ident, p, nds, sc).view(np.uint32), zs.view(np.uint32))
    ident[2, 17, 1] = np.nextafter(ident[2, 17, 1], np.float32(np.inf))
    with pytest.raises(AssertionError):
        P.fit_ray_sample_depths(ident, p, nds, sc)


def test_fma_with_one_rounding():
    """_fma_f32 against exact rational arithmetic, on products whose sum with 0.25 does not fit a double"""
    from fractions import Fraction
    rng = np.random.default_rng(2)
    a = np.concatenate([(10.0 ** rng.uniform(-12, 6, 4000) * rng.choice([-1.0, 1.0], 4000)), [0.0, 1e-30, -1e-30, 2.0 ** -24 * math.pi]]).astype(np.float32)
    got = P._fma_f32(a, P.INV_2PI_F32, np.float32(0.25))
    for v, g in zip(a, got):
        exact = Fraction(float(v)) * Fraction(float(P.INV_2PI_F32)) + Fraction(1, 4)
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(exact - Fraction(float(g))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi)))), (v, g)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------

def scene_inputs(base, name, pe0=None, pe1=None):
    sc, rots, pose = P.scene_of(base, name, pe0, pe1)
    return sc, [P.frame_inputs(sc, pose, rot) for rot in rots]


@pytest.mark.parametrize("name,pe0", [("near", (10, 4)), ("near", (2, 2)), ("near", (6, 3)), ("near", (16, 1)), ("far", (10, 4)), ("far", (16, 1)),
                                      ("straddle", (10, 4))])
def test_sampling_scenes_fill_their_conditions(name, pe0, base_case):
    sc, frames = scene_inputs(base_case[2], name, pe0=pe0)
    info = P.conditions(name, [f[1] for f in frames], pe0[0])
    if name == "near":      # the directions too
        P.conditions("near", [f[0] for f in frames], pe0[1])
    if name == "far" and pe0[0] == 10:
        assert info["max_rev"] > 256 and min(info["share_beyond_256"][:2]) >= 0.25, info


@pytest.mark.parametrize("name", ["near", "far", "straddle"])
def test_shading_scenes_fill_their_conditions(name, base_case):
    sc, rots, pose = P.scene_of(base_case[2], name)
    xs = []
    key = P.shade_keys(P.W * P.H)
    for rot in rots:
        u, p, nds, _ = P.frame_inputs(sc, pose, rot)
        zw = O.to_world_depth(O.bin_t((key & 127).astype(np.int64)), sc).astype(np.float32)
        xs.append(O.shading_inputs(p, nds, (key >> 7).astype(np.int64), zw, sc)[:, :3])
    P.conditions(name, xs, sc.pos_enc[1][0])


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------

def _far_block(base_case):
    """one 10-band position block of the far scene, both camera rotations: x, and its column table"""
    sc, frames = scene_inputs(base_case[2], "far")
    return np.concatenate([f[1] for f in frames]), P.pe_columns(10)


def _col(cols, kind, band, comp):
    return cols.index((kind, band, comp))


def fault_top_band_zero(x, cols, s, form):
    out = s.copy()
    rev = P.revolutions(x, 10)[:, 9, :]
    for c in range(3):
        for kind in ("sin", "cos"):
            j = _col(cols, kind, 9, c)
            out[rev[:, c] > P.REV_LIMIT, j] = 0.0
    reached = [c for c in range(3) if (rev[:, c] > P.REV_LIMIT).any()]
    assert len(reached) >= 2
    return out, [_col(cols, k, 9, c) for k in ("sin", "cos") for c in reached]


def fault_sin_cos_swapped(x, cols, s, form):
    out = s.copy()
    a, b = _col(cols, "sin", 3, 1), _col(cols, "cos", 3, 1)
    out[:, [a, b]] = s[:, [b, a]]
    return out, [a, b]


def fault_band_off_by_one(x, cols, s, form):
    out = s.copy()
    two = P.expected((x * np.float32(2.0)).astype(np.float32), 10, form)
    js = [_col(cols, k, 5, c) for k in ("sin", "cos") for c in range(3)]
    out[:, js] = two[:, js]
    return out, js


def fault_quarter_turn_dropped(x, cols, s, form):
    out = s.copy()
    js = [j for j, c in enumerate(cols) if c[0] == "cos"]
    out[:, js] = s[:, [j - 3 for j in js]]
    return out, js


def fault_components_exchanged(x, cols, s, form):
    out = s.copy()
    a, b = _col(cols, "sin", 2, 0), _col(cols, "sin", 2, 2)
    out[:, [a, b]] = s[:, [b, a]]
    return out, [a, b]


def fault_quarter_turn_in_radians(x, cols, s, form):
    out = s.copy()
    a = P.arguments(x, 10)
    js = [j for j, c in enumerate(cols) if c[0] == "cos"]
    for j in js:
        out[:, j] = np.sin(a[:, cols[j][1], cols[j][2]] + 0.25)
    return out, js


FAULTS = {"top_band_zero_beyond_256_revolutions": fault_top_band_zero, "sin_and_cos_swapped_on_one_slot": fault_sin_cos_swapped,
          "band_2b_taken_as_2b_plus_1": fault_band_off_by_one, "quarter_turn_dropped": fault_quarter_turn_dropped,
          "two_components_exchanged_in_one_band": fault_components_exchanged, "quarter_turn_added_in_radians": fault_quarter_turn_in_radians}


@pytest.mark.parametrize("model,form", [("exact", "accurate"), ("split", "accurate"), ("fp16", "fast"), ("bf16", "fast")])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_the_checker_rejects_planted_faults(fault, model, form, base_case):
    x, cols = _far_block(base_case)
    s, E, truth, bands = P.block_expectation(x, 10, form)
    clean = P.check_slots(P.ROUNDING(s, model), s, E, model, bands, truth)
    assert not clean["bad"].any() and not clean["moved"].any()
    # a correct kernel anywhere inside the widening passes too
    rng = np.random.default_rng(4)
    assert not P.check_slots(P.ROUNDING(s + E * rng.uniform(-1, 1, s.shape), model), s, E, model, bands, truth)["bad"].any()
    planted, js = FAULTS[fault](x, cols, s, form)
    res = P.check_slots(P.ROUNDING(planted, model), s, E, model, bands, truth)
    hit = res["bad"][:, js]
    assert hit.any(axis=0).all(), "%s under %s: columns %s pass" % (fault, model, [j for j, h in zip(js, hit.any(axis=0)) if not h])
    # not a rare event either: wherever the fault moves a value by more than the model's own resolution it is caught, and it moves a tenth
    # of the values of its columns and more (the zeroed top band: each component is beyond 256 revolutions under one camera of three)
    changed = np.abs(planted[:, js] - s[:, js]) > 2.0 ** -7
    assert hit[changed].mean() >= 0.99 and changed.mean() >= 0.1, (fault, model, hit[changed].mean(), changed.mean())
    others = np.setdiff1d(np.arange(len(cols)), js)
    assert not res["bad"][:, others].any()
    assert sum(v["bad"] for v in res["per_band"].values()) == int(res["bad"].sum())


def test_the_checker_rejects_an_identity_slot_off_by_one_ulp(base_case):
    x, cols = _far_block(base_case)
    s, E, truth, bands = P.block_expectation(x, 10, "accurate")
    out = P.ROUNDING(s, "exact")
    out[:, 1] = np.nextafter(x[:, 1], np.float32(np.inf)).astype(np.float64)
    res = P.check_slots(out, s, E, "exact", bands, truth)
    assert res["bad"][:, 1].all() and not np.delete(res["bad"], 1, axis=1).any() and res["per_band"][-1]["bad"] == len(x)
