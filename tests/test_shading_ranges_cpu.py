"""The two arguments the bf16 shading kernels rest on, CPU side (the GPU side: tests/test_gpu_shading_ranges.py, which takes its networks and
rows from here):

 A. the packer's per-layer powers of two (pack.cpp scale_layer) are exact: a network whose layer outputs are rescaled by powers of two
    (mlp_reference.rescale) packs to the SAME weight and bias bytes, and only the two output exponents move; the +-100 boundary of the
    exponents refuses / floors as documented;
 B. the clamped conversion never cuts a real activation when the packer's premise (|x_i| <= kPosIdentityBound = 4096) is filled: networks with
    non-negative weights on positions up to 4090 bring layer 0's scaled output into [0.5, 1] -- rows on which an exponent one too small
    (fault ("clamp", 0, e)) is rejected by the comparator while the emulated correct kernel passes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import adanerf_oracle as O
import mlp_reference as M
from conftest import load_case
from mfma_emulation import PackedNet, pack_weights, run_shading_net_generic, scale_exponents
from test_gpu_mlp_engines import BASE, SHADE_CASES, shading_model

import adanerf_amd
from adanerf_amd import renderer as R

K_POS_IDENTITY_BOUND = 4096.0      # pack.hpp kPosIdentityBound
K_MAX_SCALE_EXP = 100              # pack.cpp kMaxScaleExp

# ---- A: networks and schedules ---------------------------------------------------------------------------------------------------------

RESCALE_TOPOLOGIES = ["fixed_8x256", "w96_d5_skips1_3", "w512_d2_catchall"]      # the fixed kernels' net, two concatenations, the catch-all layout
SCHEDULES = ["zero", "ramp_up", "ramp_down", "zigzag"]


def schedule(name, depth):
    """Exponents in mlp_reference.shading_layer_names order.  The schedule runs over the depth + 1 ReLU layers (the trunk, views_linears.0);
    a layer without an activation takes the exponent of the layer it reads, as the packer keeps it there -- with any other value the packed
    alpha / rgb rows themselves would carry the difference and the streams could not be byte-identical."""
    k = np.arange(depth + 1)
    relu = {"zero": 0 * k, "ramp_up": 5 * (k + 1), "ramp_down": -5 * (k + 1), "zigzag": np.where(k % 2 == 0, 12, -12)}[name]
    relu = [int(v) for v in relu]
    return relu[:depth] + [relu[depth - 1], relu[depth - 1], relu[depth], relu[depth]]


def out_exponents(E):
    """(Ea, Ec) of a schedule"""
    return int(E[-3]), int(E[-1])


def rescale_model(base_case, tmp_path_factory, tag):
    """(scene, base weights, base model dir, n_pos) of one topology of section A"""
    depth, width, skips, pe1 = SHADE_CASES[tag]
    z, sc, wts, d = shading_model(base_case, tmp_path_factory, "rescale_" + tag, depth, width, skips, pe1, 700 + list(SHADE_CASES).index(tag))
    return sc, wts, d, 3 + 6 * pe1[0]


def write_net1(tmp_path_factory, tag, sc, wts, net1):
    d = str(tmp_path_factory.mktemp(tag))
    O.write_model_dir(d, sc, O.Weights(wts.net0, net1))
    return d


# ---- B: the positive family and the rows that fill the premise ------------------------------------------------------------------------------

POSITIVE_CASES = {"pos_d3_w64": (3, 64, [1], 811), "pos_d5_w128": (5, 128, [1, 3], 812)}      # id: (depth, width, skips, seed); encoding (2, 2)
POSITIVE_PE = (2, 2)


def layer0_bound(net1):
    """pack.cpp scale_layer for pts_linears.0: max over rows of |b| + sum |w| cb, identity columns budgeted for kPosIdentityBound, x 1.03125"""
    w, b = np.abs(net1["pts_linears.0.weight"].astype(np.float64)), np.abs(net1["pts_linears.0.bias"].astype(np.float64))
    cb = np.ones(w.shape[1])
    cb[:3] = K_POS_IDENTITY_BOUND
    return float((w @ cb + b).max() * 1.03125)


def positive_net(depth, width, skips, seed, n_in0):
    """|Kaiming weights|, non-negative biases.  Layer 0 is then multiplied by a factor that is no power of two and brings its activation
    bound to 0.99 x the power of two the packer rounds it up to: the packer's exponent then leaves no slack beyond the bound's own."""
    n = 3 + 6 * POSITIVE_PE[0]
    wts = O.synthetic_weights(seed, n_in0=n_in0, n_in1_pos=n, n_in1_dir=3 + 6 * POSITIVE_PE[1], layers=(8, depth), widths=(256, width),
                              skip1=skips if skips else 99)
    net1 = {k: np.abs(v).astype(np.float32) for k, v in wts.net1.items()}
    b0 = layer0_bound(net1)
    f = np.float32(0.99 * 2.0 ** np.ceil(np.log2(b0)) / b0)
    assert np.log2(float(f)) != np.round(np.log2(float(f)))
    net1["pts_linears.0.weight"] = (net1["pts_linears.0.weight"] * f).astype(np.float32)
    net1["pts_linears.0.bias"] = (net1["pts_linears.0.bias"] * f).astype(np.float32)
    return O.Weights(wts.net0, net1)


def positive_scene(base_case):
    z, meta, sc = base_case
    return dataclasses.replace(sc, pos_enc=(sc.pos_enc[0], POSITIVE_PE), normalization="None")


def premise_rows(sc, seed, n=BASE):
    """n rays with one sample each, as (origins [n,3], directions [n,3], depths [n], premise mask): origins inside the view cell, unit
    directions.  About a third of the samples are pushed to the premise by their depth: max_i |x_i| in [3000, 4090], half of them along a
    near-diagonal direction (all three components large), the first 96 of those in the positive octant, where non-negative weights give the
    largest activations; the rest stay of order 1."""
    rng = np.random.default_rng(seed)
    o = (np.array(sc.view_cell_center) + rng.uniform(-0.5, 0.5, (n, 3)) * np.array(sc.view_cell_size)).astype(np.float32)
    d = rng.standard_normal((n, 3))
    far = np.flatnonzero(rng.uniform(size=n) < 1.0 / 3.0)
    diag = far[::2]
    d[diag] = (1.0 + rng.uniform(-0.15, 0.15, (diag.size, 3))) * np.where(rng.uniform(size=(diag.size, 3)) < 0.5, -1.0, 1.0)
    d[diag[:96]] = np.abs(d[diag[:96]])
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    zw = rng.uniform(0.5, 8.0, n)
    k = np.argmax(np.abs(d[far]), axis=1)
    t = rng.uniform(3000.0, 4085.0, far.size)
    t[:96:2] = rng.uniform(4060.0, 4085.0, t[:96:2].size)      # far[::2] = diag: some of the positive-octant rows close to the bound
    dk, ok = d[far, k].astype(np.float64), o[far, k].astype(np.float64)
    zw[far] = (t - np.sign(dk) * ok) / np.abs(dk)              # the dominant component reaches sign(d_k) t
    mask = np.zeros(n, bool)
    mask[far] = True
    return o, d, zw.astype(np.float32), mask


def positive_case(base_case, tag):
    """(scene, weights, n_pos, origins, directions, depths, premise mask, host feature rows) of one case of section B"""
    depth, width, skips, seed = POSITIVE_CASES[tag]
    sc = positive_scene(base_case)
    wts = positive_net(depth, width, skips, seed, sc.n_in0)
    o, d, zw, mask = premise_rows(sc, seed + 50)
    feat = O.shading_inputs(o, d, np.arange(o.shape[0]), zw, sc)
    amax = np.abs(feat[:, :3]).max(axis=1)
    assert (amax[mask] >= 3000.0).all() and (amax[mask] <= 4090.0).all() and (amax[~mask] < 16.0).all(), (amax[mask].min(), amax.max())
    assert 0.25 < mask.mean() < 0.42
    return sc, wts, 3 + 6 * POSITIVE_PE[0], o, d, zw, mask, feat


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    adanerf_amd.build_library()
    return R.load_library()


@pytest.fixture(scope="module")
def base_case():
    return load_case("synthetic_fixed8")


@pytest.fixture(scope="module")
def packed_base(lib, base_case, tmp_path_factory):
    """per topology of section A: (scene, weights, n_pos, the base net's bf16 packing), packed once"""
    cache = {}

    def get(tag):
        if tag not in cache:
            sc, wts, d, n_pos = rescale_model(base_case, tmp_path_factory, tag)
            cache[tag] = (sc, wts, n_pos, pack_weights(lib, d, 1, 0))
        return cache[tag]
    return get


def _pack_rc(lib, d, prec=0):
    f = lib.adanerf_host_pack_weights
    f.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_int32)]
    f.restype = C.c_int
    wb, bf, nl = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    rc = f(d.encode(), 1, prec, None, C.byref(wb), None, C.byref(bf), None, C.byref(nl))
    return rc, (lib.adanerf_last_error(None) or b"").decode()


# ---- A ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", RESCALE_TOPOLOGIES)
def test_rescale_is_the_base_network_times_two_powers_of_two(tag, base_case, tmp_path_factory):
    """mlp_reference.rescale with an independent exponent for EVERY layer (the layers without an activation too): in fp64 the outputs are
    the base network's with rgb x 2^Ec and alpha x 2^Ea -- the scaling is by exact powers of two, so to the last few ulp."""
    sc, wts, d, n_pos = rescale_model(base_case, tmp_path_factory, tag)
    rng = np.random.default_rng(3)
    names = M.shading_layer_names(wts.net1)
    x = rng.uniform(-1.0, 1.0, (96, sc.n_in1)).astype(np.float32)
    ref = M.shading_mlp64(x, wts.net1, n_pos)
    for trial in range(3):
        E = rng.integers(-12, 13, len(names))
        got = M.shading_mlp64(x, M.rescale(wts.net1, n_pos, E), n_pos)
        Ea, Ec = out_exponents(E)
        want = np.ldexp(ref, [Ec, Ec, Ec, Ea])
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (tag, trial, E)


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("tag", RESCALE_TOPOLOGIES)
def test_rescaled_networks_pack_to_the_same_bytes(tag, sched, lib, packed_base, tmp_path_factory):
    """adanerf_host_pack_weights at bf16: the weight stream and the bias stream of the rescaled network are the base network's byte for
    byte (the packer's exponents absorb the rescaling exactly), every layer record is unchanged, and the record of the two output
    exponents moves by exactly (Ea, Ec)."""
    sc, wts, n_pos, (w0, b0, lay0) = packed_base(tag)
    depth = SHADE_CASES[tag][0]
    E = schedule(sched, depth)
    d = write_net1(tmp_path_factory, "rs_%s_%s" % (tag, sched), sc, wts, M.rescale(wts.net1, n_pos, E))
    w, b, lay = pack_weights(lib, d, 1, 0)
    assert int(lay0[-1][3]) == -1 and int(lay[-1][3]) == -1
    assert w.tobytes() == w0.tobytes(), "%s %s: %d weight bytes differ" % (tag, sched, int((w != w0).sum()) if w.size == w0.size else -1)
    assert b.tobytes() == b0.tobytes(), "%s %s: bias stream differs" % (tag, sched)
    assert np.array_equal(lay[:-1], lay0[:-1])
    Ea, Ec = out_exponents(E)
    assert (int(lay[-1][0]) - int(lay0[-1][0]), int(lay[-1][1]) - int(lay0[-1][1])) == (Ea, Ec), (lay[-1], lay0[-1], Ea, Ec)
    assert int(lay[-1][2]) == int(lay0[-1][2])


def _bf16_finite(w):
    return bool(np.isfinite((w.view(np.uint16).astype(np.uint32) << 16).view(np.float32)).all())


def _push(names, layer, k):
    """the schedule that moves ONE ReLU layer's output by 2^k (the layers without an activation behind it follow, as in `schedule`)"""
    E = [0] * len(names)
    E[names.index(layer)] = k
    if layer.startswith("pts_linears.") and names.index(layer) == len(names) - 5:
        E[names.index("feature_linear")] = E[names.index("alpha_linear")] = k
    if layer == "views_linears.0":
        E[names.index("rgb_linear")] = k
    return E


@pytest.mark.parametrize("which", ["last_trunk_layer", "views_linears.0"])
@pytest.mark.parametrize("tag", ["w96_d5_skips1_3", "w512_d2_catchall"])
def test_scale_exponent_boundary(tag, which, lib, packed_base, tmp_path_factory):
    """pack.cpp scale_layer at +-kMaxScaleExp, one layer pushed there by an exact power of two (the record of the output exponents shows that
    layer's exponent: alpha carries the last trunk layer's, rgb the view layer's): +100 packs, to the base network's bytes; +101 is refused
    with kScaleRefused naming the layer; a layer whose bound wants an exponent below -100 packs with the exponent floored at -100 and
    finite streams, and so does an all-zero layer (bound 0: exponent 0)."""
    sc, wts, n_pos, (w0, b0, lay0) = packed_base(tag)
    names = M.shading_layer_names(wts.net1)
    depth = len(names) - 4
    layer, col = ("pts_linears.%d" % (depth - 1), 0) if which == "last_trunk_layer" else ("views_linears.0", 1)
    e0 = int(lay0[-1][col])
    assert abs(e0) < 40      # a Kaiming net: far from the boundary by itself
    d = write_net1(tmp_path_factory, "edge_p100", sc, wts, M.rescale(wts.net1, n_pos, _push(names, layer, K_MAX_SCALE_EXP - e0)))
    w, b, lay = pack_weights(lib, d, 1, 0)
    assert int(lay[-1][col]) == K_MAX_SCALE_EXP and int(lay[-1][1 - col]) == int(lay0[-1][1 - col])
    assert w.tobytes() == w0.tobytes() and b.tobytes() == b0.tobytes()
    d = write_net1(tmp_path_factory, "edge_p101", sc, wts, M.rescale(wts.net1, n_pos, _push(names, layer, K_MAX_SCALE_EXP + 1 - e0)))
    rc, msg = _pack_rc(lib, d)
    assert rc != 0 and "activation bound" in msg and "2^100" in msg and msg.rstrip().endswith("layer " + layer), (rc, msg)
    assert _pack_rc(lib, d, 1)[0] == 0 and _pack_rc(lib, d, 4)[0] == 0, "fp16 and the unscaled bf16 packing still take it"
    # a near-zero layer whose bound wants -110: floored at -100 (its activations then stay below 2^-10 of the clamp).  fp32 has no room to
    # keep the rest of the network in step (rescale would refuse), so only this layer is scaled down, into the subnormals
    tiny = dict(wts.net1)
    for part in (".weight", ".bias"):
        tiny[layer + part] = np.ldexp(tiny[layer + part], -K_MAX_SCALE_EXP - 10 - e0).astype(np.float32)
    assert np.count_nonzero(tiny[layer + ".weight"]) > 0.9 * tiny[layer + ".weight"].size
    d = write_net1(tmp_path_factory, "edge_m110", sc, wts, tiny)
    w, b, lay = pack_weights(lib, d, 1, 0)
    assert int(lay[-1][col]) == -K_MAX_SCALE_EXP and abs(int(lay[-1][1 - col])) <= K_MAX_SCALE_EXP, lay[-1]
    assert np.isfinite(b).all() and _bf16_finite(w)
    # an all-zero layer
    zero = dict(wts.net1)
    zero[layer + ".weight"] = np.zeros_like(zero[layer + ".weight"])
    zero[layer + ".bias"] = np.zeros_like(zero[layer + ".bias"])
    d = write_net1(tmp_path_factory, "edge_zero", sc, wts, zero)
    w, b, lay = pack_weights(lib, d, 1, 0)
    assert -K_MAX_SCALE_EXP <= int(lay[-1][col]) <= 0 and abs(int(lay[-1][1 - col])) <= K_MAX_SCALE_EXP, lay[-1]
    assert np.isfinite(b).all() and _bf16_finite(w)


# ---- B ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", list(POSITIVE_CASES))
def test_positive_networks_fill_the_premise_and_the_clamp_fault_is_rejected(tag, lib, base_case, tmp_path_factory):
    """Conditions on the inputs of section B (not measurements): on the rows of premise_rows the packed bf16 net's layer 0 reaches a scaled
    maximum in [0.5, 1] (numpy replay of the packed blob; no layer exceeds 1: asserted inside the replay), the emulated correct kernel passes
    check_engine under the bounds the GPU test uses, and an exponent one too small at layer 0 -- its ReLU output cut at half the packer's
    power of two -- is rejected under the same bounds."""
    depth, width, skips, seed = POSITIVE_CASES[tag]
    sc, wts, n_pos, o, dirs, zw, mask, feat = positive_case(base_case, tag)
    d = write_net1(tmp_path_factory, tag, sc, wts, wts.net1)
    ws, bs, ls = pack_weights(lib, d, 1, 0)
    wu, bu, lu = pack_weights(lib, d, 1, 4)
    scaled, plain = PackedNet(ws, bs, ls, 0), PackedNet(wu, bu, lu, 0)
    assert scaled.scaled and scaled.lay[0][2] == 56       # the 16-band catch-all layout
    exps = scale_exponents(scaled, plain)
    e0 = exps[0]
    assert e0 == int(np.ceil(np.log2(layer0_bound(wts.net1))))
    x, dpe = feat[:, 0:3], feat[:, n_pos:n_pos + 3]
    out = run_shading_net_generic(scaled, x, dpe, depth, width, skips, fp=16, fd=16)
    m0 = scaled.max_relu_out_of[0]
    assert 0.5 <= m0 <= 1.0, (tag, m0)
    assert all(0.0 < v <= 1.0 for v in scaled.max_relu_out_of.values()), scaled.max_relu_out_of
    # the replay of the scaled blob is the replay of the unscaled one, bit for bit, on these rows too
    assert np.array_equal(out, run_shading_net_generic(plain, x, dpe, depth, width, skips, fp=16, fd=16))
    ref64 = M.shading_mlp64(feat, wts.net1, n_pos)
    refq = M.shading_mlp64(feat, wts.net1, n_pos, "bf16")
    bounds, shown = M.emulation_bounds(feat, wts.net1, n_pos, "bf16", ref64, refq)
    M.check_engine(M.shading_mlp64(feat, wts.net1, n_pos, "bf16", f32=True), ref64, refq, "bf16", bounds=bounds)
    M.check_engine(out, ref64, refq, "bf16", bounds=bounds)      # and so does the replay of the packed blob
    cut = M.shading_mlp64(feat, wts.net1, n_pos, "bf16", fault=("clamp", 0, e0), f32=True)
    with pytest.raises(AssertionError):
        M.check_engine(cut, ref64, refq, "bf16", bounds=bounds)
    # the reason fp16 is left out of the GPU test: the fp64 trunk leaves the fp16 range
    assert M.shading_hidden_max(feat, wts.net1, n_pos) > 65504.0
